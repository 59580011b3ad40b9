"""CPU companion of tests/test_closed_loop_gpu.py: its case tables cover every compiled class (read from the sources, so a newly instantiated class
cannot arrive without a closed-loop case), and every case's inputs meet the conditions the GPU tests rely on, on the oracle's loop alone."""
import re
from pathlib import Path

import numpy as np
import pytest

import test_closed_loop_gpu as G
from helpers import closed_loop_conditions, oracle_closed_loop, ref_at

CSRC = Path(__file__).resolve().parents[1] / "accelerated-tinympc_amd" / "csrc"


def _macro(file, name):
    """the X(...) tuples of `#define name(X) ...` (the fullest definition where a developer switch offers a shorter one)"""
    lines = re.findall(rf"#define {name}\(X\)(.*)", (CSRC / file).read_text())
    assert lines, (file, name)
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([\d,\s]+)\)", max(lines, key=len))]


def _have(cases, kernel=None):
    return {(c["dims"], c["arith"]) for c in cases if kernel is None or c["name"].startswith(kernel + "<")}


def test_tables_list_the_compiled_classes():
    rowlane = _macro("tinympc_internal.h", "TINY_FOR_EACH_ROWLANE")
    assert len(rowlane) == 8 and set(rowlane) == set(G.ROWLANE), rowlane
    assert [n for (n,) in _macro("admm_quadlane.hip", "TINY_FOR_EACH_QUADLANE")] == G.QUADLANE
    assert sorted(n for (n,) in _macro("admm_tile16.hip", "TINY_FOR_EACH_TILE16")) == sorted(G.TILE16)
    assert set(_macro("tinympc_internal.h", "TINY_FOR_EACH_ROWDIMS")) == {d[:2] for d in G.ROWLOOP}
    assert set(_macro("tinympc_internal.h", "TINY_FOR_EACH_WAVEDIMS")) == {d[:2] for d in G.WAVE}
    assert set(_macro("f64_internal.h", "TINY_FOR_EACH_F64DIMS")) == {d[:2] for d in G.F64}
    assert set(_macro("f64_internal.h", "TINY_FOR_EACH_F64ROWS")) == G.F64_ROWS_UNROLLED
    assert set(_macro("f64_internal.h", "TINY_FOR_EACH_F64DIMS")) - set(_macro("f64_internal.h", "TINY_FOR_EACH_F64ROWS_RT")) == G.F64_NO_ROWS
    import test_parity_gpu as P
    assert set(P.GENERIC_DIMS) | {(12, 4, 35)} == set(G.GENERIC)


def test_every_compiled_class_has_a_closed_loop_case():
    both = lambda dims: {(d, a) for d in dims for a in G.ARITH}
    assert _have(G.ROWLANE_CASES, "rowlane") == both(G.ROWLANE)
    assert _have(G.ROWLANE_CASES, "quadlane") == both([(4, 1, N) for N in G.QUADLANE])
    assert _have(G.TILE16_CASES, "tile16") == both([(12, 4, N) for N in G.TILE16])
    assert {c["ref"] for c in G.TILE16_CASES} == {"window", "shared"}
    for arith in G.ARITH:
        rl = [c for c in G.ROWLANE_CASES if c["arith"] == arith]
        assert {c["B"] for c in rl} == {1, 3, 37, 130}
        assert {c["adv"] for c in rl if c["ref"] == "window"} == {0, 1, 2}
        assert any(c.get("near_end") for c in rl) and any(c.get("near_end") for c in G.TILE16_CASES if c["arith"] == arith)
        assert {c["B"] for c in G.TILE16_CASES if c["arith"] == arith} == {17, 65, 130}
    assert {d for d, a in _have(G.ROWLOOP_CASES, "rowloop") if a == "exact"} == set(G.ROWLOOP)
    assert sum(a == "fast" for _, a in _have(G.ROWLOOP_CASES)) == 3
    assert {c["name"] for c in G.ROWSTREAM_CASES} == {"rowstream<12,4,exact>", "rowstream<8,4,exact>"}
    for k in ("wavestream", "waveres"):
        assert {d for d, a in _have(G.WAVE_CASES, k) if a == "exact"} == set(G.WAVE)
    assert _have(G.WAVE_CASES, "tile48") == both([d for d in G.WAVE if d[:2] == (32, 16)])
    assert ((16, 8, 10), "fast") in _have(G.WAVE_CASES, "waveres")
    assert {c["dims"] for c in G.GENERIC_CASES} == set(G.GENERIC) and all(c["variant"] == 4 and c["B"] == 37 for c in G.GENERIC_CASES)
    assert {c["name"] for c in G.STREAM_CASES} == {"stream<3,1>", "stream<2,1>"}
    for dims, row in (((12, 4, 30), 1), ((12, 4, 17), 2), ((4, 1, 10), 1)):
        got = {(c["arith"], c["storage"]) for c in G.FP16_CASES if c["dims"] == dims and c["row"] == row}
        assert got == {(a, s) for a in G.ARITH for s in ((16, None), (16, 16))}, dims
    for d in G.F64:
        assert {c["variant"] for c in G.F64_CASES if c["dims"] == d} == ({1} if d[:2] in G.F64_NO_ROWS else {1, 2}), d
        assert d[2] in (9, 10, 33)
    assert all(c["B"] == 130 for c in G.F64_CASES)
    for fam in (G.ROWLANE_CASES, G.TILE16_CASES, G.ROWLOOP_CASES, G.WAVE_CASES, G.GENERIC_CASES, G.FP16_CASES, G.F64_CASES):
        assert any(c["settings"].get("max_iter") == 1 for c in fam), fam[0]["fam"]
    assert all(G.STEPS in range(8, 13) and dict(G.BASE, **c["settings"])["max_iter"] <= 40 for c in G.ALL_CASES)


@pytest.mark.parametrize("family", ["rowlane", "tile16", "rowloop", "rowstream", "wave", "generic", "stream", "fp16", "f64"])
def test_inputs_meet_the_conditions(tinympc, oracle_mod, family):
    """Over the steps of every case some instance runs out of iterations, some converges early, some input bound is active and the state stays finite
    (what the GPU tests assert again before they compare)."""
    O, pr = oracle_mod, tinympc.problems
    for c in G.ALL_CASES:
        if c["fam"] != family:
            continue
        prob, settings, x0, ref, bnds = G.case_inputs(pr, O, c)
        out = oracle_closed_loop(O, prob, np.float64 if family == "f64" else np.float32, settings, x0, ref, bnds, G.STEPS, c["adv"])
        closed_loop_conditions(out, bnds, settings, c["id"])
        if c.get("near_end"):  # the windows do reach the clamp
            assert int(ref[1].max()) + (G.STEPS - 1) * c["adv"] + prob["N"] > len(ref[0]), c["id"]
            assert ref_at(ref, G.STEPS - 1, c["adv"], prob["N"], c["B"]).shape == (c["B"], prob["N"], prob["nx"])
