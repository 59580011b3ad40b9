"""CPU companion of tests/test_models64_gpu.py: the C-ABI of the fp64 per-instance models is declared, bound and mirrored, the new translation units
are registered, and every row's inputs are checked on the fp64 oracle alone: (a) some instance ends at max_iter and, where max_iter > 1, some
instance converges earlier; (b) some input bound is active; (c) everything is finite; (d) EVERY instance whose model is not model 0 gets different
bits in u when it is solved with model 0's data instead — a kernel that ignored the instance's offset into the records cannot pass.  For the
closed-loop rows without a plant, x after the first plant step differs from the step with model 0's Adyn / Bdyn for every such instance.  These are
conditions on the inputs, not tolerances; no instance is masked out."""
import re
from pathlib import Path

import numpy as np
import pytest

import test_models64_gpu as M
from helpers import STATE_ORDER, closed_loop_conditions

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("tiny_batch64_set_models", "tiny_batch64_set_models_device", "tiny_batch64_clear_models", "tiny_batch64_models_per_instance", "tiny_batch64_set_systems")
METHODS = ("set_models", "set_systems", "clear_models", "models_per_instance")
UNITS = {"admm_f64_rows_pm.hip": "admm_f64_rows.hip", "admm_f64_rowsim_pm.hip": "admm_f64_rows.hip", "admm_f64_thread_pm.hip": "admm_f64_thread.hip"}


def test_the_interface_is_declared_bound_and_exported(tinympc):
    header = (ROOT / "include" / "tinympc_batch64.h").read_text()
    src = (ROOT / "accelerated-tinympc_amd" / "solver.py").read_text()
    table = src[src.index("sig64 = {"):]
    table = table[:table.index("_lib = lib")]
    lib = tinympc.load_library()
    for n in SYMBOLS:
        assert re.search(rf"\bint\s+{n}\s*\(\s*TinyBatch64\s*\*", header), n
        assert n in tinympc.exported_symbols() and hasattr(lib, n), n
        assert re.search(rf'"{n}"\s*:', table), n
    for m in METHODS:
        assert callable(getattr(tinympc.TinyBatchSolver64, m, None)), m
    for n in SYMBOLS[2:4]:  # (a NULL handle is refused before anything touches a device)
        assert getattr(lib, n)(None) == M.EINVAL


def test_the_new_units_are_registered(tinympc):
    B = tinympc.build
    for unit, included in UNITS.items():
        assert unit.startswith("admm_f64_") and unit in B.SOURCES and B.INCLUDED_SOURCES[unit] == [included], unit
        assert (B.CSRC / unit).exists()
    assert B.KERNEL_SOURCES["rows64"] == "admm_f64_rows.hip" and B.KERNEL_SOURCES["thread64"] == "admm_f64_thread.hip"


def test_rows_are_the_issue_s_table():
    S, L = M.SOLVE_ROWS, M.LOOP_ROWS
    assert [(r["name"], r["dims"], r["B"], r["nm"]) for r in S[:10]] == [
        ("rows64<12,4,10,pm>", (12, 4, 10), 130, 7), ("rows64<12,4,30,pm>", (12, 4, 30), 9, 4), ("rows64<12,4,20,pm>", (12, 4, 20), 5, 5),
        ("rows64<4,1,10,pm>", (4, 1, 10), 130, 7), ("rows64<8,4,9,pm>", (8, 4, 9), 5, 3), ("rows64<12,2,n<=32,pm>", (12, 2, 13), 37, 5),
        ("rows64<4,4,n<=32,pm>", (4, 4, 32), 5, 3), ("rows64<12,4,n<=64,pm>", (12, 4, 40), 5, 3), ("thread64<16,4,pm>", (16, 4, 10), 130, 7),
        ("thread64<12,4,pm>", (12, 4, 10), 65, 4)]
    assert S[1]["pib"] and S[3]["settings"] == dict(check_termination=3) and S[9]["kernel"] == 1
    assert [r["settings"] for r in S[10:]] == [dict(max_iter=1)] and all(r["settings"] == dict(max_iter=0) for r in M.ZERO_ITER_ROWS)
    assert [(r["name"], r["dims"], r["B"], r["plant"], r["w"]) for r in L] == [
        ("rows64<12,4,10,mpc,pm>", (12, 4, 10), 130, None, False), ("rows64<12,4,10,sim,pm>", (12, 4, 10), 5, "inst", True),
        ("rows64<12,4,30,sim,pm>", (12, 4, 30), 5, "shared", True), ("rows64<4,1,10,mpc,pm>", (4, 1, 10), 130, None, False),
        ("rows64<8,4,9,mpc,pm>", (8, 4, 9), 3, None, True), ("rows64<12,2,n<=32,mpc,pm>", (12, 2, 13), 37, None, False),
        ("rows64<12,4,n<=64,pm>", (12, 4, 40), 5, None, True), ("thread64<16,4,pm>", (16, 4, 10), 130, None, False)]
    assert (L[0]["ref"], L[0]["adv"]) == ("window", 1) and L[2].get("near_end") and L[3]["ref"] == "shared" and M.STEPS == 8


def _others(inp):
    other = np.nonzero(inp["model"] != 0)[0]
    assert other.size and (inp["model"] == 0).any()
    return other


def _differs(a, b, idx):
    """per instance of idx: some bit of a differs from b"""
    return np.array([not M.same_bits(a[i], b[i]) for i in idx])


@pytest.mark.parametrize("row", M.SOLVE_ROWS, ids=[r["id"] for r in M.SOLVE_ROWS])
def test_one_solve_inputs_meet_the_conditions(tinympc, oracle_mod, row):
    O, r = oracle_mod, row
    inp = M.row_inputs(tinympc.problems, O, r)
    first, second = M.two_solves(O, inp)
    mi = inp["settings"]["max_iter"]
    for what, st in (("cold", first), ("warm", second)):
        assert all(np.isfinite(st[k]).all() for k in STATE_ORDER) and np.isfinite(st["residuals"]).all(), f"{r['id']} {what}: not finite"   # (c)
    st = first
    assert ((st["status"] == 11) & (st["iter"] == mi)).any(), f"{r['id']}: no instance ends at max_iter"                                    # (a)
    if mi > 1:
        assert ((st["status"] == 1) & (st["iter"] < mi)).any(), f"{r['id']}: no instance converges before max_iter"
    umn, umx = inp["bnds"][2], inp["bnds"][3]
    assert ((st["u"] <= umn) | (st["u"] >= umx)).any(), f"{r['id']}: no input bound is active"                                              # (b)
    other = _others(inp)
    for what, got, base in zip(("cold", "warm"), (first, second), M.two_solves(O, inp, model=np.zeros_like(inp["model"]))):                # (d)
        d = _differs(got["u"], base["u"], other)
        assert d.all(), f"{r['id']} {what}: u of instances {other[~d]} is what model 0's data gives"
    print(f"{r['id']}: {len(set(first['iter']))} distinct iteration counts, {(first['status'] == 1).sum()} solved / {(first['status'] == 11).sum()} at max_iter, "
          f"u differs with model 0's data in {other.size} of {other.size}")


def test_zero_iterations_compute_nothing(tinympc, oracle_mod):
    for r in M.ZERO_ITER_ROWS:
        inp = M.row_inputs(tinympc.problems, oracle_mod, r)
        first, second = M.two_solves(oracle_mod, inp)
        for st in (first, second):
            assert (st["status"] == 11).all() and (st["iter"] == 1).all() and all((st[k] == 0).all() for k in STATE_ORDER if k != "x")


@pytest.mark.parametrize("row", M.LOOP_ROWS, ids=[r["id"] for r in M.LOOP_ROWS])
def test_closed_loop_inputs_meet_the_conditions(tinympc, oracle_mod, row):
    O, r = oracle_mod, row
    inp = M.row_inputs(tinympc.problems, O, r)
    out = M.models_oracle_loop(O, inp, r)
    closed_loop_conditions(out, inp["bnds"], inp["settings"], r["id"])                                                                      # (a) (b) (c)
    assert out["xs"].shape == (M.STEPS, r["B"], r["dims"][0]) and np.isfinite(out["xs"]).all()
    if r.get("near_end"):  # the windows do reach the clamp
        assert int(inp["ref"][1].max()) + (M.STEPS - 1) * r["adv"] + r["dims"][2] > len(inp["ref"][0]), r["id"]
    other = _others(inp)
    base = M.models_oracle_loop(O, inp, r, steps=1, model=np.zeros_like(inp["model"]))
    d = _differs(out["u0"][0], base["u0"][0], other)                                                                                        # (d)
    assert d.all(), f"{r['id']}: u.col(0) of instances {other[~d]} is what model 0's data gives at step 0"
    if inp["plant"] is None:  # the plant step is the instance's own model's
        x1 = M.own_plant_step(O, inp["probs"], np.zeros_like(inp["model"]), np.asarray(inp["x0"], np.float64), out["u0"][0])
        if inp["w"] is not None:
            x1 = x1 + inp["w"][0]
        d = _differs(out["xs"][0], x1, other)
        assert d.all(), f"{r['id']}: x after the first plant step of instances {other[~d]} is what model 0's Adyn / Bdyn give"
