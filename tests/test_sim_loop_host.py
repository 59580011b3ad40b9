"""CPU companion of tests/test_sim_loop_gpu.py: the reference loop of a simulated closed-loop run is built from the oracle alone, and every case's
inputs are checked on it — the conditions the GPU tests rely on (helpers.closed_loop_conditions), that the plant and the disturbance move u.col(0)
of every instance away from the nominal loop's (a kernel that ignored either cannot pass), and that the model as plant without a disturbance is
helpers.oracle_closed_loop bit for bit.  The C-ABI and the Python methods must exist."""
import numpy as np
import pytest

import test_sim_loop_gpu as S
from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_conditions, oracle_closed_loop, same_bits

SYMBOLS = ("tiny_batch_set_plant", "tiny_batch_clear_plant", "tiny_batch_plant_mode", "tiny_batch_mpc_step_sim_async", "tiny_batch_mpc_run_sim_async",
           "tiny_batch_mpc_run_sim")


@pytest.fixture(autouse=True)
def the_interface_is_declared(tinympc):
    """the cases below are the gate of a feature: without its C-ABI they gate nothing"""
    missing = [n for n in SYMBOLS if n not in tinympc.exported_symbols()]
    assert not missing, f"include/tinympc_batch.h does not declare {missing}"


def test_the_interface_is_declared_and_exported(tinympc):
    lib = tinympc.load_library()
    for n in SYMBOLS:
        assert n in tinympc.exported_symbols() and hasattr(lib, n), n
    for m in ("set_plant", "clear_plant", "plant_mode", "mpc_step_sim", "mpc_run_sim"):
        assert callable(getattr(tinympc.TinyBatchSolver, m)), m
    assert "admm_rowsim.hip" in tinympc.build.SOURCES and tinympc.build.INCLUDED_SOURCES["admm_rowsim.hip"] == ["admm_rowlane.hip"]


def test_the_cases_cover_what_the_paths_can_get_wrong():
    on = S.ONCHIP_CASES
    assert {c["plant"] for c in on} == {None, "shared", "inst"} and any(c.get("pm") for c in on) and any(c["dims"][0] < 8 for c in on)
    assert any(c["dims"] == (12, 4, 30) and c["settings"] == dict(max_iter=1) for c in on)
    assert any(not c["w"] for c in on) and all(c["B"] == 5 and c["onchip"] for c in on)
    rp = S.REPLAY_CASES
    assert any(c["B"] > 128 for c in rp) and any(c["dims"][0] >= 8 and c["dims"][1] >= 8 for c in rp) and any(c.get("storage") for c in rp)
    assert {c["name"].split("<")[0] for c in rp} == {"rowloop", "waveres", "quadlane", "rowlane"} and not any(c["onchip"] for c in rp)
    assert S.HANDOVER_CASE["B"] == 17 and S.HANDOVER_CASE["row"] == 5


@pytest.mark.parametrize("case", S.ALL_CASES, ids=S._ids(S.ALL_CASES))
def test_inputs_meet_the_conditions_and_leave_the_nominal_loop(tinympc, oracle_mod, case):
    O = oracle_mod
    inp = S.case_inputs(tinympc.problems, O, case)
    assert inp["plant"] is not None or inp["w"] is not None
    out = S.case_oracle(O, case, inp)
    closed_loop_conditions(out, inp["bnds"], inp["settings"], case["id"])
    assert out["xs"].shape == (S.STEPS, case["B"], case["dims"][0]) and np.isfinite(out["xs"]).all() and same_bits(out["xs"][-1], out["x"])
    nominal = S.case_oracle(O, case, inp, nominal=True)
    for k in (1, S.STEPS - 1):
        same = np.all(out["u0"][k] == nominal["u0"][k], axis=-1)
        assert not same.any(), f"{case['id']}: u.col(0) of instances {np.nonzero(same)[0]} is the nominal loop's at step {k}"
    if not case.get("pm"):   # the loop without a plant or a disturbance is the helper's
        p = inp["probs"][0]
        ref = oracle_closed_loop(O, p, np.float32, inp["settings"], inp["x0"], inp["ref"], inp["bnds"], S.STEPS, case["adv"])
        as_plant = S.sim_oracle_loop(O, inp["probs"], inp["model"], inp["settings"], inp["x0"], inp["ref"], inp["bnds"], S.STEPS, case["adv"],
                                     plant=(np.asarray(p["Adyn"], np.float32), np.asarray(p["Bdyn"], np.float32)))
        for got in (nominal, as_plant):
            for k in ("u0", "iter", "status", "x"):
                assert same_bits(got[k], ref[k]), (case["id"], k)
            for k in STATE_ORDER + SCALAR_ORDER:
                assert same_bits(got["st"][k], ref["st"][k]), (case["id"], k)


def test_the_montecarlo_example_compiles_against_the_c_abi(tinympc, tmp_path):
    """examples/quadrotor_tracking_montecarlo.cpp uses nothing but include/tinympc_batch.h: plain g++ must build it, as the other examples"""
    import shutil
    import subprocess
    from pathlib import Path
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = Path(__file__).resolve().parents[1]
    tinympc.build.build()
    lib_dir = root / "accelerated-tinympc_amd" / "lib"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{root / 'include'}", str(root / "examples" / "quadrotor_tracking_montecarlo.cpp"),
                        f"-L{lib_dir}", "-ltinympc_hip", f"-Wl,-rpath,{lib_dir}", "-o", str(tmp_path / "montecarlo")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
