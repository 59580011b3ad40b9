"""The per-step solver log of the closed-loop runs (tiny_batch_mpc_run_log_async, tiny_batch_mpc_run_log, tiny_batch64_mpc_run_log): two int arrays
[steps][batch], row k = work.iter / work.status of every instance after the solve of MPC step k.  Every entry is compared for equality, no mask:

 1. with the reference's own closed-loop traces (tests/golden/closed_loop_traces.npz, quad_hover_f64_N10.npz) over their full step counts, on the
    on-chip loops that store the rows themselves (16-lane, quad-lane) and on kernels that copy them per step (the matrix-core kernel, which with a
    log is replayed; rolled-loop, streaming; the fp64 library, whose runs with a log are launch sequences);
 2. with get_status after each step of a step-by-step loop on a second handle, one case per path, six steps each; u.col(0), x0 and the final
    workspace are bitwise equal too;
 3. a run with NULL logs, a run with logs and tiny_batch_mpc_run_sim leave the same bits and the same kernel name;
 4. the edges: one step, one log alone, max_iter reached at step 0, one captured graph for equal calls, log / no log by turns;
 5. guard zones around logs sized exactly [steps][B].
tests/test_run_log_host.py shows on the CPU that the fixtures can carry 1 (both status values, pairwise distinct rows)."""
import ctypes as C

import numpy as np
import pytest

import test_sim_loop64_gpu as S64
import test_sim_loop_gpu as S
from helpers import GOLDEN, SCALAR_ORDER, STATE_ORDER, bounds_of, closed_loop_case, load_fixture, same_bits

pytestmark = pytest.mark.gpu

TWIN_STEPS = 6
IP = C.POINTER(C.c_int)
FP = C.POINTER(C.c_float)


@pytest.fixture(autouse=True)
def the_interface_is_exported(tinympc):
    """without the feature every test of this file fails here, at the missing symbol"""
    lib = tinympc.load_library()
    for n in ("tiny_batch_mpc_run_log_async", "tiny_batch_mpc_run_log", "tiny_batch64_mpc_run_log"):
        assert hasattr(lib, n), f"{n} is not exported"


@pytest.fixture(scope="module")
def traces():
    return np.load(GOLDEN / "closed_loop_traces.npz")


def _ip(a):
    return None if a is None else a.ctypes.data_as(IP)


def _fp(a):
    return None if a is None else a.ctypes.data_as(FP)


def _raw_run_log(s, steps, adv, w=None, u0=True, x=False, it=True, st=True):
    """tiny_batch_mpc_run_log with any of its arrays left NULL"""
    out = dict(u0=np.zeros((steps, s.B, s.nu), np.float32) if u0 else None, x=np.zeros((steps, s.B, s.nx), np.float32) if x else None,
               iter=np.full((steps, s.B), -7, np.int32) if it else None, status=np.full((steps, s.B), -7, np.int32) if st else None)
    wa = None if w is None else np.ascontiguousarray(w, np.float32)
    rc = s.lib.tiny_batch_mpc_run_log(s._h, steps, adv, _fp(wa), _fp(out["u0"]), _fp(out["x"]), _ip(out["iter"]), _ip(out["status"]))
    assert rc == 0, s.lib.tiny_batch_last_error()
    return out


# ---- 1: the reference's traces -----------------------------------------------------------------------------------------------------------------

# (scenario, set_row_kernel's family, B, the kernel a run launches, on chip: no graph is captured)
TRACE_CASES = [(name, 1, B, "rowlane<12,4,30,exact>", True) for name in ("hover", "track") for B in (1, 3, 37)]   # lone, partial wave, several workgroups
TRACE_CASES += [("cartpole", 4, B, "quadlane<4,1,10,exact>", True) for B in (5, 64)]
TRACE_CASES += [("track", 5, B, "tile16<12,4,30,exact>", False) for B in (17, 64)]   # a padding tile, full tiles; with a log the matrix-core kernel is replayed
TRACE_CASES += [("hover", 2, 37, "rowloop<12,4,exact>", False), ("hover", 3, 37, "rowstream<12,4,exact>", False), ("dims837", 2, 20, "rowloop<8,3,exact>", False)]


def _trace_handle(T, O, z, name, row, B):
    prob, x0, fn, steps, settings, table, start = closed_loop_case(T.problems, O, z, name)
    s = T.TinyBatchSolver(prob, B, settings=settings)
    s.select_kernel(2); s.set_row_kernel(row)
    s.set_bounds(*T.problems.bounds_arrays(prob))
    if table is not None:
        s.set_xref_window(table, start[:B])
    else:
        s.set_xref(fn(0))
    s.set_x0(x0[:B])
    return s, steps, 1 if table is not None else 0


@pytest.mark.parametrize("name,row,B,kernel,onchip", TRACE_CASES, ids=[f"{c[0]}-{c[3].split('<')[0]}-B{c[2]}" for c in TRACE_CASES])
def test_log_equals_the_reference_trace(tinympc, oracle_mod, traces, name, row, B, kernel, onchip):
    z = traces
    s, steps, adv = _trace_handle(tinympc, oracle_mod, z, name, row, B)
    assert s.closed_loop_kernel_name() == kernel, s.closed_loop_kernel_name()
    out = s.mpc_run_log(steps, adv)
    assert s.closed_loop_kernel_name() == kernel
    assert s.lib.tiny_batch_debug_graph_captures(s._h) == (0 if onchip else 1)
    it, st, _ = s.get_status()
    s.close()
    assert out["x"] is None and out["iter"].shape == out["status"].shape == (steps, B) and out["iter"].dtype == np.int32
    assert np.array_equal(out["iter"], z[f"{name}_iter"][:, :B]), f"iter differs from step {S.G._first_diff(out['iter'], z[f'{name}_iter'][:, :B])} on"
    assert np.array_equal(out["status"], z[f"{name}_status"][:, :B]), f"status differs from step {S.G._first_diff(out['status'], z[f'{name}_status'][:, :B])} on"
    assert same_bits(out["u0"], z[f"{name}_u0"][:, :B])
    assert np.array_equal(it, out["iter"][-1]) and np.array_equal(st, out["status"][-1]), "the last row is the workspace's iter / status"
    if name == "hover":
        assert (out["status"][0] == 11).all() and (out["iter"][0] == 100).all(), "max_iter is reached at step 0"


@pytest.mark.parametrize("kernel,name", [(0, "rows64<12,4,10,mpc>"), (1, "thread64<12,4>")])
def test_fp64_log_equals_the_as_shipped_hover_trace(tinympc, kernel, name):
    meta, prob, solves, z = load_fixture("quad_hover_f64_N10")
    s = tinympc.TinyBatchSolver64(prob, 1, settings=solves[0]["settings"])
    s.select_kernel(kernel)
    s.set_bounds(*bounds_of(prob, np.float64)); s.set_xref(solves[0]["xref"])
    s.set_state(solves[0]["pre"])
    assert s.closed_loop_kernel_name() == name, s.closed_loop_kernel_name()
    out = s.mpc_run_log(70)
    s.close()
    assert np.array_equal(out["iter"][:, 0], z["trace_iter"]) and np.array_equal(out["status"][:, 0], z["trace_status"])
    assert same_bits(out["u0"][:, 0], z["trace_u0"])
    assert set(np.unique(out["status"])) == {1, 11} and out["iter"][0, 0] == 100 and out["iter"][69, 0] == 2


# ---- 2: the step-by-step twin ------------------------------------------------------------------------------------------------------------------

TWIN_CASES = [
    S._case("rowlane<12,4,10,exact>", (12, 4, 10), 5, "window", None, False),
    S._case("rowlane<12,4,10,fast>", (12, 4, 10), 5, "window", None, False, arith="fast", quadrotor=True),
    S.ONCHIP_CASES[6],                                                                                   # per-instance models
    S.ONCHIP_CASES[1],                                                                                   # a plant per instance, a disturbance, x_traj
    S._case("waveres<16,8,exact>", (16, 8, 10), 5, "shared", "shared", True, row=7, onchip=False),
    S.REPLAY_CASES[4],                                                                                   # fp16 storage
]


@pytest.mark.parametrize("case", TWIN_CASES, ids=[c["id"] for c in TWIN_CASES])
def test_log_equals_get_status_of_a_step_by_step_loop(tinympc, oracle_mod, case):
    T = tinympc
    inp = S.case_inputs(T.problems, oracle_mod, case)
    w = None if inp["w"] is None else inp["w"][:TWIN_STEPS]
    simulated = inp["plant"] is not None or w is not None
    a, b = S._handle(T, case, inp), S._handle(T, case, inp)
    name = a.closed_loop_kernel_name()
    out = a.mpc_run_log(TWIN_STEPS, case["adv"], w, record_x=simulated)
    assert a.closed_loop_kernel_name() == name
    onchip = case["onchip"] and not case.get("pm")   # with per-instance models a run that asks for a log is replayed
    assert a.lib.tiny_batch_debug_graph_captures(a._h) == (0 if onchip else 1), case["id"]
    for k in range(TWIN_STEPS):
        b.mpc_step_sim(case["adv"], None if w is None else w[k])
        it, st, _ = b.get_status()
        assert np.array_equal(out["iter"][k], it) and np.array_equal(out["status"][k], st), f"{case['id']}: the log differs at step {k}"
        assert same_bits(out["u0"][k], b.get_u()[:, 0]), (case["id"], k)
        if simulated:
            assert same_bits(out["x"][k], b.get_x0()), (case["id"], k)
    sa, sb = a.get_state(), b.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(sa[k], sb[k]), f"{case['id']}: {k} differs after the last step"
    assert same_bits(a.get_x0(), b.get_x0())
    assert len(np.unique(out["iter"])) > 1, "a log of one value shows nothing"
    a.close(); b.close()


def _models64(prob, B):
    """set_models' arrays: every instance the class's model (the ',pm' kernels read one record per instance whatever it holds)"""
    rep = lambda a: np.broadcast_to(np.asarray(a, np.float64), (B,) + np.asarray(a).shape).copy()
    return dict(rho=np.full(B, prob["rho"]), **{k: rep(prob[k]) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn", "Q")})


@pytest.mark.parametrize("pm", [False, True], ids=["sim", "pm"])
def test_fp64_log_equals_get_status_of_a_step_by_step_loop(tinympc, oracle_mod, pm):
    T = tinympc
    r = S64.ROWS[5]   # rows64<4,1,10,sim>: 130 instances, a shared plant, a disturbance, check_termination = 3; no window to slide between single steps
    assert r["adv"] == 0 and r["name"] == "rows64<4,1,10,sim>"
    inp = S64.row_inputs(T.problems, oracle_mod, r)
    w = inp["w"][:TWIN_STEPS]
    hs = [S64._handle(T, r, inp) for _ in range(2)]
    if pm:
        for h in hs:
            h.set_models(_models64(inp["prob"], r["B"]))
            assert h.closed_loop_kernel_name() == "rows64<4,1,10,sim,pm>", h.closed_loop_kernel_name()
    a, b = hs
    out = a.mpc_run_log(TWIN_STEPS, 0, w, record_x=True)
    for k in range(TWIN_STEPS):
        b.mpc_step_sim(w[k])
        it, st, _ = b.get_status()
        assert np.array_equal(out["iter"][k], it) and np.array_equal(out["status"][k], st), f"the log differs at step {k}"
        x, u = b.first_columns()
        assert same_bits(out["x"][k], x), k
        assert same_bits(out["u0"][k], u), k
    sa, sb = a.get_state(), b.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(sa[k], sb[k]), f"{k} differs after the last step"
    assert set(np.unique(out["status"])) == {1, 11}
    a.close(); b.close()


# ---- 3: no behaviour change --------------------------------------------------------------------------------------------------------------------

SAME_CASES = [
    S.ONCHIP_CASES[1],                                                                                   # the SIM loop of the 16-lane kernel
    S._case("rowlane<12,4,10,exact>", (12, 4, 10), 5, "window", None, False),                            # its nominal loop
    S._case("tile16<12,4,30,exact>", (12, 4, 30), 17, "window", None, False, row=5),                     # on chip without a log, replayed with one
    S._case("quadlane<4,1,10,exact>", (4, 1, 10), 5, "shared", None, False, row=0),
    S.REPLAY_CASES[0],
]
for _c in SAME_CASES[1:4]:
    _c["id"] += "-nominal"


@pytest.mark.parametrize("case", SAME_CASES, ids=[c["id"] for c in SAME_CASES])
def test_a_log_changes_nothing(tinympc, oracle_mod, case):
    T = tinympc
    inp = S.case_inputs(T.problems, oracle_mod, case)
    w = None if inp["w"] is None else inp["w"][:TWIN_STEPS]
    got = {}
    for way in ("sim", "null logs", "logs"):
        s = S._handle(T, case, inp)
        name = s.closed_loop_kernel_name()
        if way == "sim":
            u0, _ = s.mpc_run_sim(TWIN_STEPS, case["adv"], w, record_x=False)
        else:
            u0 = _raw_run_log(s, TWIN_STEPS, case["adv"], w, it=way == "logs", st=way == "logs")["u0"]
        assert s.closed_loop_kernel_name() == name == case.get("loop", case["name"]), (way, s.closed_loop_kernel_name())
        got[way] = (u0, s.get_state(), s.get_x0(), s.lib.tiny_batch_debug_graph_captures(s._h))
        s.close()
    for way in ("null logs", "logs"):
        assert same_bits(got[way][0], got["sim"][0]), f"{way}: u0_traj"
        for k in STATE_ORDER + SCALAR_ORDER:
            assert same_bits(got[way][1][k], got["sim"][1][k]), f"{way}: {k}"
        assert same_bits(got[way][2], got["sim"][2]), f"{way}: x0"
    assert got["null logs"][3] == got["sim"][3], "NULL logs take the path the run always took"


# ---- 4: the edges ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [SAME_CASES[1], SAME_CASES[4]], ids=["rowlane", "rowloop"])
def test_one_step_one_log_and_turns(tinympc, oracle_mod, case):
    T = tinympc
    inp = S.case_inputs(T.problems, oracle_mod, case)
    w, adv, n = inp["w"], case["adv"], S.STEPS
    s = S._handle(T, case, inp)
    whole = _raw_run_log(s, n, adv, w)
    s.close()
    # one step: the first row of the longer run, and what get_status says
    s = S._handle(T, case, inp)
    one = _raw_run_log(s, 1, adv, None if w is None else w[:1])
    it, st, _ = s.get_status()
    s.close()
    assert np.array_equal(one["iter"], whole["iter"][:1]) and np.array_equal(one["status"], whole["status"][:1]) and same_bits(one["u0"], whole["u0"][:1])
    assert np.array_equal(one["iter"][0], it) and np.array_equal(one["status"][0], st)
    # one of the two logs alone
    for keep in ("iter", "status"):
        s = S._handle(T, case, inp)
        got = _raw_run_log(s, n, adv, w, u0=False, it=keep == "iter", st=keep == "status")
        s.close()
        assert np.array_equal(got[keep], whole[keep]), keep
    # log / no log / log: the rows of the whole run, the run in between included in what follows
    s = S._handle(T, case, inp)
    cut = lambda a, b: None if w is None else w[a:b]
    first = _raw_run_log(s, 3, adv, cut(0, 3))
    mid = _raw_run_log(s, 2, adv, cut(3, 5), it=False, st=False)
    last = _raw_run_log(s, n - 5, adv, cut(5, n))
    s.close()
    for k in ("iter", "status"):
        assert np.array_equal(first[k], whole[k][:3]) and np.array_equal(last[k], whole[k][5:]), k
    assert same_bits(np.concatenate([first["u0"], mid["u0"], last["u0"]]), whole["u0"])


def test_equal_blocking_calls_replay_one_graph(tinympc, oracle_mod):
    T, case = tinympc, S.REPLAY_CASES[0]
    inp = S.case_inputs(T.problems, oracle_mod, case)
    s = S._handle(T, case, inp)
    a = s.mpc_run_log(4, case["adv"], inp["w"][:4])
    assert s.lib.tiny_batch_debug_graph_captures(s._h) == 1
    b = s.mpc_run_log(4, case["adv"], inp["w"][4:8])
    assert s.lib.tiny_batch_debug_graph_captures(s._h) == 1, "the staging buffers of the logs stay on the handle: one captured graph"
    s.close()
    s = S._handle(T, case, inp)
    whole = s.mpc_run_log(8, case["adv"], inp["w"])
    s.close()
    for k in ("iter", "status"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k


# ---- 5: guard zones ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 17, 37])
def test_guard_zones_stay_intact(tinympc, oracle_mod, traces, B):
    """one run per kernel that stores the log rows itself, and the matrix-core kernel's replay; logs sized exactly [steps][B]"""
    T = tinympc
    T.solver.debug_guards(True)
    try:
        for name, row, kernel in (("track", 1, "rowlane<12,4,30,exact>"), ("cartpole", 4, "quadlane<4,1,10,exact>"), ("track", 5, "tile16<12,4,30,exact>")):
            s, _, adv = _trace_handle(T, oracle_mod, traces, name, row, B)
            assert s.closed_loop_kernel_name() == kernel
            out = s.mpc_run_log(5, adv)
            assert T.solver.debug_check() == 0, (kernel, B)
            assert np.array_equal(out["iter"], traces[f"{name}_iter"][:5, :B]) and np.array_equal(out["status"], traces[f"{name}_status"][:5, :B]), (kernel, B)
            s.close()
    finally:
        T.solver.debug_guards(False)
