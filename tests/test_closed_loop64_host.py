"""CPU companion of tests/test_closed_loop64_gpu.py: the C-ABI of the fp64 closed-loop run is declared, bound and mirrored, and the inputs of every
row of the GPU table meet the conditions the GPU tests rely on, on the oracle's loop alone."""
import re
from pathlib import Path

import pytest

import test_closed_loop64_gpu as G

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("tiny_batch64_set_xref_window", "tiny_batch64_mpc_run", "tiny_batch64_mpc_run_traj", "tiny_batch64_get_xref_start",
         "tiny_batch64_closed_loop_kernel_name")
METHODS = ("set_xref_window", "mpc_run", "mpc_run_traj", "xref_start", "closed_loop_kernel_name")


def test_header_declares_the_closed_loop_calls(tinympc):
    header = (ROOT / "include" / "tinympc_batch64.h").read_text()
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert n in tinympc.exported_symbols(), n
    assert re.search(r"int\s+tiny_batch64_mpc_run_traj\s*\(\s*TinyBatch64\s*\*\s*tb\s*,\s*int\s+steps\s*,\s*int\s+window_advance\s*,\s*double\s*\*", header)
    assert re.search(r"const\s+char\s*\*\s*tiny_batch64_closed_loop_kernel_name\s*\(", header)


def test_solver_binds_the_closed_loop_calls(tinympc):
    """the prototypes solver.load_library() declares (read from its source: the library itself is not needed for this)"""
    src = (ROOT / "accelerated-tinympc_amd" / "solver.py").read_text()
    table = src[src.index("sig64 = {"):]
    table = table[:table.index("_lib = lib")]
    for n in NAMES:
        assert re.search(rf'"{n}"\s*:|lib\.{n}\.argtypes', table), n
    for m in METHODS:
        assert callable(getattr(tinympc.TinyBatchSolver64, m, None)), m


def test_rows_are_the_issue_s_table():
    assert len(G.ROWS) == 11 and [r["seed"] for r in G.ROWS] == list(range(6400, 6411))
    assert sum(r["name"].endswith(",mpc>") for r in G.ROWS) == 8
    assert {r["name"] for r in G.ROWS if not r["name"].endswith(",mpc>")} == {"rows64<12,4,n<=64>", "thread64<16,4>", "thread64<12,4>"}
    assert G.STEPS == 8 and all(r["B"] <= 130 for r in G.ROWS)


@pytest.mark.parametrize("row", G.ROWS, ids=[r["id"] for r in G.ROWS])
def test_inputs_meet_the_conditions(tinympc, oracle_mod, row):
    """some instance runs out of iterations, some converges early, some input bound is active in u.col(0), everything is finite"""
    prob, settings, x0, ref, bnds, want = G.row_reference(tinympc.problems, oracle_mod, row)
    assert want["u0"].shape == (G.STEPS, row["B"], prob["nu"])
    if row.get("near_end"):  # the windows do reach the clamp
        assert int(ref[1].max()) + (G.STEPS - 1) * row["adv"] + prob["N"] > len(ref[0]), row["id"]
