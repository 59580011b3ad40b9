"""Per-instance settings (tiny_batch_set_instance_settings): every instance its own tolerances, iteration budget, check_termination and bound flags, on
the ",ps" instantiations of the unrolled 16-lane kernel (admm_rowlane_ps.hip) and of the streaming row kernel and the termination step
(admm_steps_ps.hip).  Everything is compared bit for bit — the 12 work arrays, the 4 residuals, iter, status, the signs of zeros — with the oracle run
once per distinct settings tuple (settings_cases.per_group).  tests/test_settings_host.py shows on the CPU that the draw is not vacuous."""
import numpy as np
import pytest

import settings_cases as SC
from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_inputs, oracle_closed_loop, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def the_interface_is_exported(tinympc):
    """without the feature every test of this file fails here, at the missing symbol"""
    lib = tinympc.load_library()
    for n in ("tiny_batch_set_instance_settings", "tiny_batch_clear_instance_settings", "tiny_batch_settings_per_instance"):
        assert hasattr(lib, n), f"{n} is not exported"


def assert_same(got, want, what):
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {int((np.asarray(got[k]) != np.asarray(want[k])).sum())} elements (or in the sign of a zero)"


def ps_name(dims, arith="exact", storage=""):
    nx, nu, N = dims
    return f"rowstream<{nx},{nu},{arith}{storage},ps>" if N == 13 or storage else f"rowlane<{nx},{nu},{N},{arith},ps>"


def handle(T, prob, x0, xref, bnds, settings=SC.BASE):
    s = T.TinyBatchSolver(prob, len(x0), settings=settings)
    s.set_bounds(*bnds); s.set_xref(xref)
    s.reset_workspace(); s.set_x0(x0)   # a cold start: reset_workspace() is folded into the launch
    return s


# ---- 1: a heterogeneous batch against the oracle, cold then warm with other settings --------------------------------------------------------------

HET = [(d, b, B) for d in SC.CLASSES for b in ("shared", "inst") for B in SC.BATCHES]


@pytest.mark.parametrize("dims,bounds,B", HET, ids=[f"{'x'.join(map(str, d))}-{b}-B{B}" for d, b, B in HET])
def test_heterogeneous_batch_equals_the_oracle_per_instance(tinympc, oracle_mod, dims, bounds, B):
    T, O = tinympc, oracle_mod
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, bounds)
    s = handle(T, prob, x0, xref, bnds)
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    for k, what in enumerate(("cold", "warm, other settings")):
        per = SC.draw(B, SC.SEED + k)
        s.set_instance_settings(**per)
        assert s.settings_per_instance() and s.kernel_name() == ps_name(dims), s.kernel_name()
        rc = s.solve()
        assert s.dispatch_applied() == 0
        n_unsolved = SC.oracle_solve(O, prob, np.float32, per, st, bnds, xref)
        assert_same(s.get_state(), st, f"{dims} {bounds} B={B} {what}")
        assert rc == (1 if n_unsolved else 0), "tiny_batch_solve returns 1 iff some instance did not converge within its own budget"
    s.close()


# ---- 2: fma arithmetic ---------------------------------------------------------------------------------------------------------------------------

def test_fma_arithmetic_equals_the_fma_oracle(tinympc, oracle_mod):
    T, O, dims, B = tinympc, oracle_mod, (12, 4, 10), 67
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    s = handle(T, prob, x0, xref, bnds)
    s.select_kernel(3)
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    for k in range(2):
        per = SC.draw(B, SC.SEED + k)
        s.set_instance_settings(**per)
        assert s.kernel_name() == "rowlane<12,4,10,fast,ps>", s.kernel_name()
        s.solve()
        SC.oracle_solve(O, prob, np.float32, per, st, bnds, xref, arith="fma")
        assert_same(s.get_state(), st, f"fma, solve {k}")
    s.close()


# ---- 3: uniform arrays are the shared path, clear is the parent ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (4, 1, 10), (12, 4, 13)], ids=lambda d: "x".join(map(str, d)))
def test_uniform_arrays_equal_the_shared_settings_and_clear_restores_them(tinympc, oracle_mod, dims):
    T, B = tinympc, 21
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, dims, B, "shared")
    settings = dict(SC.BASE, max_iter=9, check_termination=2, abs_pri_tol=3e-2, abs_dua_tol=2e-2)
    s = handle(T, prob, x0, xref, bnds, settings)

    def two_solves():
        s.reset_workspace(); s.set_x0(x0)
        s.solve(); s.solve()
        return s.get_state()
    parent_name = s.kernel_name()
    assert not parent_name.endswith(",ps>") and not s.settings_per_instance()
    want = two_solves()
    assert (want["status"] == 1).any() and (want["status"] == 11).any()
    s.set_instance_settings(**{k: np.full(B, settings[k]) for k in SC.FIELDS})
    assert s.kernel_name() == ps_name(dims), s.kernel_name()
    assert_same(two_solves(), want, "uniform per-instance arrays")
    s.set_instance_settings(max_iter=9)   # a scalar broadcasts, NULL fields keep the batch's values
    assert_same(two_solves(), want, "one broadcast field, the rest NULL")
    s.clear_instance_settings()
    assert s.kernel_name() == parent_name and not s.settings_per_instance()
    assert_same(two_solves(), want, "after clear")
    s.close()


# ---- 4: bound flags per instance ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (12, 4, 13)], ids=lambda d: "x".join(map(str, d)))
def test_bound_flags_per_instance_fold_into_the_table(tinympc, oracle_mod, dims):
    """shared bound inputs, state and input bounds on for every other instance; neighbours 2k, 2k + 1 start from the same x0"""
    T, O, B = tinympc, oracle_mod, 18
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    x0[1::2] = x0[0::2]; xref[1::2] = xref[0::2]
    on = (np.arange(B) % 2 == 0).astype(np.int32)
    per = dict(en_state_bound=on, en_input_bound=on, max_iter=np.full(B, 12, np.int32))
    s = handle(T, prob, x0, xref, bnds)
    s.set_instance_settings(**per)
    assert s.kernel_name() == ps_name(dims), s.kernel_name()
    s.solve()
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    SC.oracle_solve(O, prob, np.float32, per, st, bnds, xref)
    got = s.get_state()
    assert_same(got, st, "alternating bound flags")
    lo, hi = bnds[2][0, 0], bnds[3][0, 0]
    z = got["znew"].reshape(B, -1)
    binds, beyond = ((z == lo) | (z == hi)).any(1), ((z < lo) | (z > hi)).any(1)
    assert not beyond[0::2].any()
    assert (binds[0::2] & beyond[1::2]).any(), "no pair whose first instance sits on its box while its neighbour, unbounded, goes beyond"
    # update_slack sees the flags through the same table
    s.update_slack()
    SC.oracle_step(O, prob, np.float32, per, st, bnds, xref, "update_slack")
    assert_same(s.get_state(), st, "update_slack under per-instance bound flags")
    # uniform flag arrays keep the shared table, and switch the bounds off for everyone
    s.set_instance_settings(en_state_bound=0, en_input_bound=0, max_iter=12)
    s.reset_workspace(); s.set_x0(x0); s.solve()
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    SC.oracle_solve(O, prob, np.float32, dict(en_state_bound=0 * on, en_input_bound=0 * on, max_iter=per["max_iter"]), st, bnds, xref)
    assert_same(s.get_state(), st, "uniform flags, all off")
    s.close()


# ---- 5: the closed loop -------------------------------------------------------------------------------------------------------------------------

STEPS = 5


def _loop_case(T, O):
    dims, B = (12, 4, 10), 19
    prob = SC.problem(T.problems, O, dims)
    x0, ref, bnds = closed_loop_inputs(prob, B, "window", SC.SEED)
    per = SC.draw(B)
    per["max_iter"] = np.maximum(per["max_iter"], 1)   # a run needs a budget for every instance
    return dims, B, prob, x0, ref, bnds, per


def _loop_handle(T, prob, x0, ref, bnds, per):
    s = T.TinyBatchSolver(prob, len(x0), settings=SC.BASE)
    s.set_bounds(*bnds); s.set_xref_window(*ref); s.set_x0(x0)
    s.set_instance_settings(**per)
    return s


def test_closed_loop_on_chip_equals_steps_and_the_oracle_loop(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    dims, B, prob, x0, ref, bnds, per = _loop_case(T, O)
    # the oracle's closed loop, one per settings group
    want = dict(u0=np.zeros((STEPS, B, 4), np.float32), iter=np.zeros((STEPS, B), np.int32), status=np.zeros((STEPS, B), np.int32), x=np.zeros((B, 12), np.float32))
    groups = {}
    for b in range(B):
        groups.setdefault(tuple(SC.settings_of(per, b).items()), []).append(b)
    for key, idx in groups.items():
        idx = np.array(idx)
        out = oracle_closed_loop(O, prob, np.float32, dict(key), x0[idx], (ref[0], ref[1][idx]), bnds, STEPS, 1)
        for k in ("u0", "iter", "status"):
            want[k][:, idx] = out[k]
        want["x"][idx] = out["x"]
    assert len(set(want["iter"][0])) > 3 and (want["status"] == 1).any() and (want["status"] == 11).any()
    a = _loop_handle(T, prob, x0, ref, bnds, per)
    assert a.closed_loop_kernel_name() == "rowlane<12,4,10,exact,ps>", a.closed_loop_kernel_name()
    got = a.mpc_run_log(STEPS, 1)
    assert a.lib.tiny_batch_debug_graph_captures(a._h) == 0, "the run stays on chip"
    for k in ("u0", "iter", "status"):
        assert same_bits(got[k], want[k]), f"on-chip run: {k} differs from the oracle's loop"
    assert same_bits(a.get_x0(), want["x"])
    b = _loop_handle(T, prob, x0, ref, bnds, per)
    for k in range(STEPS):
        b.mpc_step_async(1)
        it, stt, _ = b.get_status()
        assert same_bits(b.get_u()[:, 0], want["u0"][k]) and np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"step {k}"
    assert same_bits(b.get_x0(), want["x"])
    assert_same(a.get_state(), b.get_state(), "on-chip run against the step-by-step loop")
    a.close(); b.close()


def test_closed_loop_with_a_plant_and_a_disturbance_is_replayed(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    dims, B, prob, x0, ref, bnds, per = _loop_case(T, O)
    rng = np.random.default_rng(SC.SEED + 2)
    Ap = (np.asarray(prob["Adyn"], np.float64) * (1 + 0.05 * rng.standard_normal((12, 12)))).astype(np.float32)
    Bp = (np.asarray(prob["Bdyn"], np.float64) * (1 + 0.05 * rng.standard_normal((12, 4)))).astype(np.float32)
    w = (0.01 * rng.standard_normal((STEPS, B, 12))).astype(np.float32)
    # the oracle's loop against the plant: per step y = g = 0, tiny_solve per settings group, x = (A_p x + B_p u0) + w
    plant = O.Oracle(dict(prob, Adyn=Ap, Bdyn=Bp), np.float32).plant_step
    st = O.new_state(B, *dims)
    x = x0.copy()
    want = dict(u0=[], iter=[], status=[], x=[])
    for k in range(STEPS):
        st["x"][:, 0] = x; st["y"][:] = 0; st["g"][:] = 0
        xr = np.ascontiguousarray(ref[0][np.minimum(ref[1][:, None] + k + np.arange(10)[None], len(ref[0]) - 1)])
        SC.oracle_solve(O, prob, np.float32, per, st, bnds, xr)
        x = plant(x, st["u"][:, 0]) + w[k]
        want["u0"].append(st["u"][:, 0].copy()); want["iter"].append(st["iter"].copy()); want["status"].append(st["status"].copy()); want["x"].append(x.copy())
    a = _loop_handle(T, prob, x0, ref, bnds, per)
    a.set_plant(Ap, Bp)
    assert a.closed_loop_kernel_name() == "rowlane<12,4,10,exact,ps>", a.closed_loop_kernel_name()
    got = a.mpc_run_log(STEPS, 1, w, record_x=True)
    assert a.lib.tiny_batch_debug_graph_captures(a._h) == 1, "a simulated run with per-instance settings is a replayed launch sequence"
    for k in ("u0", "iter", "status", "x"):
        assert same_bits(got[k], np.array(want[k])), f"replayed run with a plant: {k} differs from the oracle's loop"
    a.close()


# ---- 6: termination_condition -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", [32, 16])
def test_termination_condition_reads_the_instance_record(tinympc, oracle_mod, storage):
    T, O, dims, B = tinympc, oracle_mod, (12, 4, 10), 37
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    R = O.round_h16 if storage == 16 else (lambda a: a)
    dt = "h16" if storage == 16 else np.float32
    x0, xref, bnds = R(x0), R(xref), tuple(R(b) for b in bnds)
    s = T.TinyBatchSolver(prob, B, settings=SC.BASE)
    if storage == 16:
        s.set_storage(16, 16)
    s.set_bounds(*bnds); s.set_xref(xref); s.reset_workspace(); s.set_x0(x0)
    s.set_instance_settings(max_iter=5)
    s.solve()   # a workspace with residuals of every size
    st = s.get_state()
    per = SC.draw(B, SC.SEED + 3)
    per["abs_pri_tol"][::3] = 10.0; per["abs_dua_tol"][::3] = 10.0   # a third converges whenever its check is due
    st["iter"] = np.arange(1, B + 1, dtype=np.int32)                  # iter % check_termination: due for some, not for others
    s.set_state(st)
    s.set_instance_settings(**per)
    conv = s.termination_condition()
    want = SC.oracle_step(O, prob, dt, per, st, bnds, xref, "termination_condition")
    due = st["iter"] % per["check_termination"] == 0
    assert (want & due).any() and (~want & due).any() and (~due).any()
    assert np.array_equal(conv, want)
    assert_same(s.get_state(), st, "termination_condition")
    s.close()


# ---- 7: fp16 storage ----------------------------------------------------------------------------------------------------------------------------

def test_fp16_storage_goes_to_the_streaming_kernel_and_equals_the_h16_oracle(tinympc, oracle_mod):
    T, O, dims, B = tinympc, oracle_mod, (12, 4, 10), 37
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "inst")
    x0, xref, bnds = O.round_h16(x0), O.round_h16(xref), tuple(O.round_h16(b) for b in bnds)
    s = T.TinyBatchSolver(prob, B, settings=SC.BASE)
    s.set_storage(16)
    s.set_bounds(*bnds); s.set_xref(xref); s.reset_workspace(); s.set_x0(x0)
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    for k in range(2):
        per = SC.draw(B, SC.SEED + k)
        s.set_instance_settings(**per)
        assert s.kernel_name() == "rowstream<12,4,exact,h16,ps>", s.kernel_name()
        s.solve()
        SC.oracle_solve(O, prob, "h16", per, st, bnds, xref)
        assert_same(s.get_state(), st, f"fp16 storage, solve {k}")
    s.close()


# ---- 8: refusals and recovery -------------------------------------------------------------------------------------------------------------------

def test_check_termination_below_one_names_the_first_index(tinympc, oracle_mod):
    T = tinympc
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, (12, 4, 10), 9, "shared")
    s = handle(T, prob, x0, xref, bnds)
    ct = np.ones(9, np.int32)
    ct[3] = 0; ct[7] = -2
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-1: check_termination\[3\] = 0"):
        s.set_instance_settings(check_termination=ct)
    assert not s.settings_per_instance() and s.kernel_name() == "rowlane<12,4,10,exact>"
    s.close()


def _refused(T, s, x0, what):
    """with per-instance settings installed the handle's solve is TINY_BATCH_EUNSUPPORTED with a text; after clear it solves as before"""
    s.reset_workspace(); s.set_x0(x0); s.solve()
    want, name = s.get_state(), s.kernel_name()
    s.set_instance_settings(max_iter=np.arange(len(x0)) % 5 + 1)
    assert s.kernel_name() == "unsupported", (what, s.kernel_name())
    s.reset_workspace(); s.set_x0(x0)
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-3: .*per-instance.{10,}") as e:
        s.solve()
    print(what, "->", e.value)
    s.clear_instance_settings()
    assert s.kernel_name() == name
    s.reset_workspace(); s.set_x0(x0); s.solve()
    assert_same(s.get_state(), want, f"{what}: after clear")
    s.close()


def test_a_wave_class_is_refused(tinympc, oracle_mod):
    T, B = tinympc, 6
    prob = T.problems.random_system(32, 16, 10, seed=3216, riccati=oracle_mod.riccati)
    x0, xref, bnds = closed_loop_inputs(prob, B, "inst", 5)
    _refused(T, handle(T, prob, x0, xref, bnds), x0, "nx + nu = 48")


def test_per_instance_models_are_refused(tinympc, oracle_mod):
    T, B = tinympc, 6
    fam = T.problems.model_family("quadrotor", 3, B, seed=3)
    mods = T.problems.family_caches(fam)
    prob = dict(mods["probs"][0], N=10, u_min=-0.5, u_max=0.5, x_min=-5.0, x_max=5.0)
    x0, xref, bnds = closed_loop_inputs(prob, B, "inst", 5)
    s = handle(T, prob, x0, xref, bnds)
    s.set_models(mods)
    _refused(T, s, x0, "per-instance models")


@pytest.mark.parametrize("dims,family,name", [((12, 4, 10), 2, "rowloop"), ((4, 1, 10), 4, "quadlane"), ((12, 4, 30), 5, "tile16")])
def test_a_forced_family_without_a_ps_form_is_refused(tinympc, oracle_mod, dims, family, name):
    T, B = tinympc, 18
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, dims, B, "shared")
    s = handle(T, prob, x0, xref[0], bnds)   # (one shared reference: tile16 serves it)
    s.set_row_kernel(family)
    assert s.kernel_name().startswith(name + "<"), s.kernel_name()
    _refused(T, s, x0, f"forced {name}")


def test_a_run_with_a_zero_budget_is_refused(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    dims, B, prob, x0, ref, bnds, per = _loop_case(T, O)
    per["max_iter"][4] = 0
    s = _loop_handle(T, prob, x0, ref, bnds, per)
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-1: .*max_iter > 0 for every instance"):
        s.mpc_run_log(STEPS, 1)
    s.mpc_step_async(1)   # one step is a solve: the instance without a budget keeps its workspace
    it, stt, _ = s.get_status()
    assert it[4] == 1 and stt[4] == 11 and not s.get_array("vnew")[4].any()
    s.close()


# ---- 9: guard zones -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 17, 203])
def test_ps_kernels_stay_inside_their_allocations(tinympc, oracle_mod, B):
    T, O = tinympc, oracle_mod
    T.solver.debug_guards(True)
    try:
        for dims, bounds, run in (((12, 4, 10), "shared", False), ((12, 4, 10), "inst", False), ((12, 4, 10), "shared", True), ((12, 4, 13), "inst", False)):
            prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, bounds)
            per = SC.draw(B, flags=not run and bounds == "shared")
            s = handle(T, prob, x0, xref, bnds)
            if run:
                per["max_iter"] = np.maximum(per["max_iter"], 1)
            s.set_instance_settings(**per)
            if run:
                assert s.closed_loop_kernel_name().endswith(",ps>")
                out = s.mpc_run_log(3)
                assert np.isfinite(out["u0"]).all()
            else:
                assert s.kernel_name().endswith(",ps>")
                s.solve()
                s.termination_condition()
            st = s.get_state()
            assert all(np.isfinite(st[k]).all() for k in STATE_ORDER + ("residuals",)), (dims, bounds, run)
            assert T.solver.debug_check() == 0, (dims, bounds, run, B)
            s.close()
    finally:
        T.solver.debug_guards(False)
