"""CPU companion of tests/test_sim_loop64_gpu.py: the C-ABI of the fp64 simulated closed loop is declared, bound and mirrored, and every row's inputs
are checked on the fp64 oracle's loop alone — the conditions the GPU tests rely on (helpers.closed_loop_conditions), that the plant and the
disturbance move u.col(0) away from the nominal loop's by the second step (a kernel that ignored either cannot pass), and that the model as plant
without a disturbance is helpers.oracle_closed_loop bit for bit."""
import re
from pathlib import Path

import numpy as np
import pytest

import test_sim_loop64_gpu as S
from helpers import SCALAR_ORDER, STATE_ORDER, oracle_closed_loop, closed_loop_conditions, same_bits

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("tiny_batch64_set_plant", "tiny_batch64_clear_plant", "tiny_batch64_plant_mode", "tiny_batch64_mpc_step_sim", "tiny_batch64_mpc_run_sim")
METHODS = ("set_plant", "clear_plant", "plant_mode", "mpc_step_sim", "mpc_run_sim")


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
    assert re.search(r"tiny_batch64_mpc_run_sim\s*\(\s*TinyBatch64\s*\*\s*tb\s*,\s*int\s+steps\s*,\s*int\s+window_advance\s*,\s*const\s+double\s*\*\s*w[^,]*,\s*double\s*\*\s*u0_traj[^,]*,"
                     r"\s*double\s*\*\s*x_traj", header)
    for m in METHODS:
        assert callable(getattr(tinympc.TinyBatchSolver64, m, None)), m
    B = tinympc.build
    assert "admm_f64_rowsim.hip" in B.SOURCES and B.INCLUDED_SOURCES["admm_f64_rowsim.hip"] == ["admm_f64_rows.hip"]
    assert B.KERNEL_SOURCES["rows64"] == "admm_f64_rows.hip"


def test_rows_are_the_issue_s_table():
    R = S.ROWS
    assert len(R) == 12 and S.STEPS == 8 and S.K1 == 3
    assert [(r["dims"], r["B"]) for r in R] == [((12, 4, 10), 130), ((12, 4, 10), 5), ((12, 4, 10), 5), ((12, 4, 30), 5), ((12, 4, 20), 5), ((4, 1, 10), 130),
                                               ((8, 4, 9), 3), ((12, 2, 13), 37), ((4, 4, 32), 5), ((12, 4, 40), 5), ((16, 4, 10), 130), ((12, 4, 10), 1)]
    assert [r["plant"] for r in R] == ["inst", "shared", None, "inst", "inst", "shared", "inst", "shared", "inst", "inst", "shared", "inst"]
    assert [r["w"] for r in R] == [True, True, True, True, False, True, True, True, False, True, True, True]
    assert [(r["ref"], r["adv"]) for r in R] == [("window", 1), ("window", 1), ("window", 1), ("window", 2), ("inst", 0), ("shared", 0), ("window", 1), ("window", 1),
                                                 ("inst", 0), ("window", 1), ("window", 1), ("shared", 0)]
    assert R[3].get("near_end") and R[4]["settings"] == dict(max_iter=1) and R[5]["settings"] == dict(check_termination=3) and R[11]["kernel"] == 1
    assert sum(r["name"].endswith(",sim>") for r in R) == 8 and R[2]["name"] == "rows64<12,4,10,mpc>" and len(S.ONCHIP) == 9
    assert [r["name"] for r in R[9:]] == ["rows64<12,4,n<=64>", "thread64<16,4>", "thread64<12,4>"]


@pytest.mark.parametrize("row", S.ROWS, ids=[r["id"] for r in S.ROWS])
def test_inputs_meet_the_conditions_and_leave_the_nominal_loop(tinympc, oracle_mod, row):
    O, r = oracle_mod, row
    inp = S.row_inputs(tinympc.problems, O, r)
    assert inp["plant"] is not None or inp["w"] is not None
    assert (inp["w"] is None) == (not r["w"])
    out = S.row_oracle(O, r, inp)
    closed_loop_conditions(out, inp["bnds"], inp["settings"], r["id"])
    assert out["xs"].shape == (S.STEPS, r["B"], r["dims"][0]) and out["xs"].dtype == np.float64 and np.isfinite(out["xs"]).all()
    assert same_bits(out["xs"][-1], out["x"])
    if r.get("near_end"):  # the windows do reach the clamp
        assert int(inp["ref"][1].max()) + (S.STEPS - 1) * r["adv"] + inp["prob"]["N"] > len(inp["ref"][0]), r["id"]
    nominal = S.row_oracle(O, r, inp, nominal=True)
    for k in (1, S.STEPS - 1):  # (rows 5 and 9 have no disturbance: the plant alone moves them)
        same = np.all(out["u0"][k] == nominal["u0"][k], axis=-1)
        assert not same.any(), f"{r['id']}: u.col(0) of instances {np.nonzero(same)[0]} is the nominal loop's at step {k}"
    p = inp["prob"]
    ref = oracle_closed_loop(O, p, np.float64, inp["settings"], inp["x0"], inp["ref"], inp["bnds"], S.STEPS, r["adv"])
    as_plant = S.sim_oracle_loop(O, p, inp["settings"], inp["x0"], inp["ref"], inp["bnds"], S.STEPS, r["adv"],
                                 plant=(np.asarray(p["Adyn"], np.float64), np.asarray(p["Bdyn"], np.float64)), w=np.full((S.STEPS, r["B"], p["nx"]), -0.0))
    for got in (nominal, as_plant):
        for k in ("u0", "iter", "status", "x"):
            assert same_bits(got[k], ref[k]), (r["id"], k)
        for k in STATE_ORDER + SCALAR_ORDER:
            assert same_bits(got["st"][k], ref["st"][k]), (r["id"], k)
