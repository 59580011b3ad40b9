"""Per-instance settings of the fp64 library (tiny_batch64_set_instance_settings): every instance its own tolerances, iteration budget,
check_termination and bound flags, on the ",ps" instantiations of the sixteen-lane kernel (admm_f64_rows_ps.hip, admm_f64_rowloop_ps.hip), of the
thread-per-instance kernel and of the two step functions that read a setting (admm_f64_thread_ps.hip).  Everything is compared bit for bit — the 12
work arrays, the 4 residuals, iter, status, the signs of zeros — with the fp64 oracle run once per distinct settings tuple (settings64_cases.per_group).
tests/test_settings64_host.py shows on the CPU that the draw is not vacuous."""
import numpy as np
import pytest

import settings64_cases as SC
from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_inputs, same_bits

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, ENOTREADY = -1, -3, -4


@pytest.fixture(autouse=True)
def the_interface_is_exported(tinympc):
    """without the feature every test of this file fails here, at the missing symbol"""
    lib = tinympc.load_library()
    for n in ("tiny_batch64_set_instance_settings", "tiny_batch64_clear_instance_settings", "tiny_batch64_settings_per_instance"):
        assert hasattr(lib, n), f"{n} is not exported"


def test_the_error_codes_are_the_header_s(tinympc):
    import re
    txt = (tinympc.solver.PKG.parent / "include" / "tinympc_batch.h").read_text()
    for name, v in (("EINVAL", EINVAL), ("ENOTREADY", ENOTREADY), ("EUNSUPPORTED", EUNSUPPORTED)):
        assert int(re.search(rf"TINY_BATCH_{name}\s*=\s*(-?\d+)", txt).group(1)) == v


def assert_same(got, want, what):
    for k in STATE_ORDER + SCALAR_ORDER:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert same_bits(g, w), f"{what}: {k} differs in {int((g != w).sum())} elements (or in the sign of a zero)"


def handle(T, prob, x0, xref, bnds, settings=SC.BASE):
    """a cold handle: the workspace of a new TinyBatchSolver64 is all zero"""
    s = T.TinyBatchSolver64(prob, len(x0), settings=settings)
    s.set_bounds(*bnds)
    if isinstance(xref, tuple):
        s.set_xref_window(*xref)
    else:
        s.set_xref(xref)
    s.set_x0(x0)
    return s


def cold_state(O, dims, x0):
    st = O.new_state(len(x0), *dims, SC.DT)
    st["x"][:, 0] = x0
    return st


# ---- 1: a heterogeneous batch against the oracle, cold then warm under a second draw -------------------------------------------------------------

HET = [(d, b, B) for d in SC.CLASSES for b in ("shared", "inst") for B in SC.BATCHES]


@pytest.mark.parametrize("dims,bounds,B", HET, ids=[f"{'x'.join(map(str, d))}-{b}-B{B}" for d, b, B in HET])
def test_heterogeneous_batch_equals_the_oracle_per_instance(tinympc, oracle_mod, dims, bounds, B):
    T, O = tinympc, oracle_mod
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, bounds)
    s = handle(T, prob, x0, xref, bnds)
    st = cold_state(O, dims, x0)
    for k, what in enumerate(("cold", "warm, other settings")):
        per = SC.draw(B, SC.SEED + k)
        s.set_instance_settings(**per)
        assert s.settings_per_instance() and s.kernel_name() == SC.kernel_name(dims), s.kernel_name()
        rc = s.solve()
        n_unsolved = SC.oracle_solve(O, prob, per, st, bnds, xref)
        assert_same(s.get_state(), st, f"{dims} {bounds} B={B} {what}")
        assert rc == (1 if n_unsolved else 0), "tiny_batch64_solve returns 1 iff some instance did not converge within its own budget"
    s.close()


# ---- 2: the thread-per-instance kernel by choice -------------------------------------------------------------------------------------------------

def test_forced_thread_kernel_gives_the_bits_of_the_sixteen_lanes(tinympc, oracle_mod):
    T, O, dims, B = tinympc, oracle_mod, (12, 4, 10), 67
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "inst")
    got = {}
    for which, name in ((1, "thread64<12,4,ps>"), (0, "rows64<12,4,10,ps>"), (2, "rows64<12,4,10,ps>")):
        s = handle(T, prob, x0, xref, bnds)
        s.select_kernel(which)
        for k in range(2):
            s.set_instance_settings(**SC.draw(B, SC.SEED + k))
            assert s.kernel_name() == name, s.kernel_name()
            s.solve()
        got[which] = s.get_state()
        s.close()
    st = cold_state(O, dims, x0)
    for k in range(2):
        SC.oracle_solve(O, prob, SC.draw(B, SC.SEED + k), st, bnds, xref)
    for which in got:
        assert_same(got[which], st, f"select_kernel({which})")


# ---- 3: an instance without a budget keeps every byte of its workspace, beside neighbours that solve ---------------------------------------------

def random_warm_state(O, dims, B, seed):
    """every array random with signed zeros sprinkled in, random residuals, iter and status"""
    rng = np.random.default_rng(seed)
    st = O.new_state(B, *dims, SC.DT)
    for k in STATE_ORDER:
        a = 0.05 * rng.standard_normal(st[k].shape)
        z = rng.random(a.shape)
        a[z < 0.08] = 0.0
        a[z < 0.04] = -0.0
        st[k][:] = a
    st["residuals"][:] = rng.random((B, 4))
    st["iter"][:] = rng.integers(2, 30, size=B)
    st["status"][:] = rng.choice([1, 11], size=B)
    return st


@pytest.mark.parametrize("dims", [(12, 4, 10), (12, 4, 30), (12, 2, 11), (4, 2, 40), (16, 4, 10)], ids=lambda d: "x".join(map(str, d)))
def test_zero_budget_writes_status_and_iter_only(tinympc, oracle_mod, dims):
    T, O, B = tinympc, oracle_mod, 67
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    per = SC.draw(B, SC.SEED + 5)
    zero = np.flatnonzero(per["max_iter"] == 0)
    waves = {int(b) // 4 for b in zero}
    assert len(zero) >= 3 and any(sum(int(b) // 4 == w for b in zero) < 4 for w in waves), "some wave holds a budget-0 row beside rows that solve"
    up = random_warm_state(O, dims, B, SC.SEED + dims[2])
    s = handle(T, prob, x0, xref, bnds)
    s.set_state(up)
    s.set_instance_settings(**per)
    assert s.kernel_name() == SC.kernel_name(dims), s.kernel_name()
    st = {k: v.copy() for k, v in up.items()}
    rc = s.solve()
    assert rc == 1
    SC.oracle_solve(O, prob, per, st, bnds, xref)
    got = s.get_state()
    for k in STATE_ORDER + ("residuals",):
        assert got[k][zero].tobytes() == up[k][zero].tobytes(), f"{k} of a budget-0 instance is not byte for byte what was uploaded"
    assert (got["status"][zero] == 11).all() and (got["iter"][zero] == 1).all()
    assert_same(got, st, f"{dims}: the whole batch, the neighbours of the budget-0 rows included")
    s.close()


# ---- 4: uniform arrays are the shared path, clear is the parent ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (4, 1, 10), (12, 2, 11), (4, 2, 40), (16, 4, 10)], ids=lambda d: "x".join(map(str, d)))
def test_uniform_arrays_equal_the_shared_settings_and_clear_restores_them(tinympc, oracle_mod, dims):
    T, B = tinympc, 21
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, dims, B, "shared")
    settings = dict(SC.BASE, max_iter=9, check_termination=2, abs_pri_tol=3e-2, abs_dua_tol=2e-2)
    s = handle(T, prob, x0, xref, bnds, settings)
    zero = {k: np.zeros_like(v) for k, v in s.get_state().items()}

    def two_solves():
        s.set_state(zero); s.set_x0(x0)
        s.solve(); s.solve()
        return s.get_state()
    parent_name = s.kernel_name()
    assert parent_name == SC.kernel_name(dims, ps=False) and not s.settings_per_instance()
    want = two_solves()
    assert (want["status"] == 1).any() and (want["status"] == 11).any()
    s.set_instance_settings(**{k: np.full(B, settings[k]) for k in SC.FIELDS})
    assert s.kernel_name() == SC.kernel_name(dims), s.kernel_name()
    assert_same(two_solves(), want, "uniform per-instance arrays")
    s.set_instance_settings(max_iter=9)   # a scalar broadcasts, NULL fields keep the batch's values
    assert_same(two_solves(), want, "one broadcast field, the rest NULL")
    # a later set_settings moves the NULL fields with it: the tolerances of BASE end nobody early
    s.set_settings(**dict(settings, abs_pri_tol=1e-9, abs_dua_tol=1e-9))
    moved = two_solves()
    assert (moved["status"] == 11).all() and (moved["iter"] == 9).all()
    s.set_settings(**settings)
    assert_same(two_solves(), want, "set_settings back")
    s.clear_instance_settings()
    assert s.kernel_name() == parent_name and not s.settings_per_instance()
    assert_same(two_solves(), want, "after clear")
    s.close()


# ---- 5: bound flags per instance -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (12, 2, 11), (16, 4, 10)], ids=lambda d: "x".join(map(str, d)))
def test_bound_flags_per_instance(tinympc, oracle_mod, dims):
    """state and input bounds on for every other instance; neighbours 2k, 2k + 1 start from the same x0"""
    T, O, B = tinympc, oracle_mod, 18
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    x0[1::2] = x0[0::2]; xref[1::2] = xref[0::2]
    on = (np.arange(B) % 2 == 0).astype(np.int32)
    per = dict(en_state_bound=on, en_input_bound=on, max_iter=np.full(B, 12, np.int32))
    s = handle(T, prob, x0, xref, bnds)
    s.set_instance_settings(**per)
    assert s.kernel_name() == SC.kernel_name(dims), s.kernel_name()
    s.solve()
    st = cold_state(O, dims, x0)
    SC.oracle_solve(O, prob, per, st, bnds, xref)
    got = s.get_state()
    assert_same(got, st, "alternating bound flags")
    lo, hi = bnds[2][0, 0], bnds[3][0, 0]
    z = got["znew"].reshape(B, -1)
    binds, beyond = ((z == lo) | (z == hi)).any(1), ((z < lo) | (z > hi)).any(1)
    assert not beyond[0::2].any()
    assert (binds[0::2] & beyond[1::2]).any(), "no pair whose first instance sits on its box while its neighbour, unbounded, goes beyond"
    # update_slack reads the flags from the same records; the state flag alone, then the input flag alone
    for fx, fu in ((on, 1 - on), (1 - on, on)):
        per = dict(en_state_bound=fx, en_input_bound=fu)
        s.set_instance_settings(**per)
        s.update_slack()
        SC.oracle_step(O, prob, per, st, bnds, xref, "update_slack")
        assert_same(s.get_state(), st, "update_slack under per-instance bound flags")
    s.close()


# ---- 6: termination_condition --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (16, 4, 10)], ids=lambda d: "x".join(map(str, d)))
def test_termination_condition_reads_the_instance_record(tinympc, oracle_mod, dims):
    T, O, B = tinympc, oracle_mod, 37
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    s = handle(T, prob, x0, xref, bnds)
    s.set_instance_settings(max_iter=5)
    s.solve()   # a workspace with residuals of every size
    st = s.get_state()
    per = SC.draw(B, SC.SEED + 3)
    per["abs_pri_tol"][::3] = 10.0; per["abs_dua_tol"][::3] = 10.0   # a third converges whenever its check is due
    st["iter"] = np.arange(1, B + 1, dtype=np.int32)                  # iter % check_termination: due for some, not for others
    st["residuals"] = np.random.default_rng(3).random((B, 4))         # and where it is not due the residual fields stay
    s.set_state(st)
    s.set_instance_settings(**per)
    conv = s.termination_condition()
    want = SC.oracle_step(O, prob, per, st, bnds, xref, "termination_condition")
    due = st["iter"] % per["check_termination"] == 0
    assert (want & due).any() and (~want & due).any() and (~due).any()
    assert np.array_equal(conv, want)
    assert_same(s.get_state(), st, "termination_condition")
    s.close()


# ---- 7: the closed loop --------------------------------------------------------------------------------------------------------------------------

STEPS = 3
LOOPS = {(12, 4, 10): ("window", 1), (4, 1, 10): ("inst", 0), (12, 2, 11): ("window", 1)}   # a sliding window table; an array reference; capacity 32
_LOOP_CASES = {}


def loop_case(T, O, dims):
    """inputs and the oracle's nominal loop of a class, computed once and shared; nobody writes to it"""
    if dims not in _LOOP_CASES:
        B = 19
        refmode, adv = LOOPS[dims]
        prob = SC.problem(T.problems, O, dims)
        x0, ref, bnds = closed_loop_inputs(prob, B, refmode, SC.SEED, dtype=SC.DT)
        per = SC.draw(B)
        per["max_iter"] = np.maximum(per["max_iter"], 1)   # BUDGETS without the zero
        want = SC.oracle_loop(O, prob, per, x0, ref, bnds, STEPS, adv)
        assert len(set(want["iter"][0])) > 3 and (want["status"] == 1).any() and (want["status"] == 11).any()
        _LOOP_CASES[dims] = dict(B=B, adv=adv, prob=prob, x0=x0, ref=ref, bnds=bnds, per=per, want=want)
    return _LOOP_CASES[dims]


def loop_handle(T, c, per=None):
    s = handle(T, c["prob"], c["x0"], c["ref"], c["bnds"])
    s.set_instance_settings(**(per or c["per"]))
    return s


def check_loop_end(s, c, want, what):
    assert_same(s.get_state(), want["st"], what)
    assert same_bits(s.first_columns()[0], want["x"]), f"{what}: x.col(0) after the last plant step"
    if isinstance(c["ref"], tuple):
        assert np.array_equal(s.xref_start(), c["ref"][1] + STEPS * c["adv"]), f"{what}: the window starts after the run"


@pytest.mark.parametrize("dims", list(LOOPS), ids=lambda d: "x".join(map(str, d)))
def test_closed_loop_on_chip_equals_steps_and_the_oracle_loop(tinympc, oracle_mod, dims):
    T, O = tinympc, oracle_mod
    c = loop_case(T, O, dims)
    want, adv = c["want"], c["adv"]
    a = loop_handle(T, c)
    assert a.closed_loop_kernel_name() == SC.kernel_name(dims, mpc=True) and a.closed_loop_kernel_name().endswith(",mpc,ps>"), a.closed_loop_kernel_name()
    traj = a.mpc_run_traj(STEPS, adv)
    assert same_bits(traj, want["u0"]), "on-chip run: u.col(0) differs from the oracle's loop"
    it, stt, _ = a.get_status()
    assert np.array_equal(it, want["iter"][-1]) and np.array_equal(stt, want["status"][-1])
    check_loop_end(a, c, want, f"{dims} on-chip run")
    # step by step: tiny_batch64_mpc_step advances no window, so the window of step k is set before it
    b = loop_handle(T, c)
    assert b.kernel_name() == SC.kernel_name(dims)
    for k in range(STEPS):
        if isinstance(c["ref"], tuple):
            b.set_xref_window(c["ref"][0], c["ref"][1] + k * adv)
        rc = b.mpc_step()
        it, stt, _ = b.get_status()
        assert same_bits(b.get_u()[:, 0], want["u0"][k]) and np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"step {k}"
        assert rc == int((want["status"][k] != 1).any())
    assert_same(b.get_state(), want["st"], f"{dims} step by step")
    assert_same(a.get_state(), b.get_state(), "on-chip run against the step-by-step loop")
    a.close(); b.close()


@pytest.mark.parametrize("dims", list(LOOPS), ids=lambda d: "x".join(map(str, d)))
def test_closed_loop_with_a_log_is_a_sequence_with_the_same_bits(tinympc, oracle_mod, dims):
    T, O = tinympc, oracle_mod
    c = loop_case(T, O, dims)
    want = c["want"]
    a = loop_handle(T, c)
    got = a.mpc_run_log(STEPS, c["adv"])
    for k in ("u0", "iter", "status"):
        assert same_bits(got[k], want[k]), f"logged run: {k} differs from the oracle's loop (= step-by-step get_status)"
    check_loop_end(a, c, want, f"{dims} logged run")
    a.close()


@pytest.mark.parametrize("dims", list(LOOPS), ids=lambda d: "x".join(map(str, d)))
def test_closed_loop_with_a_plant_and_a_disturbance_is_replayed(tinympc, oracle_mod, dims):
    T, O = tinympc, oracle_mod
    c = loop_case(T, O, dims)
    prob, B, (nx, nu, N) = c["prob"], c["B"], dims
    rng = np.random.default_rng(SC.SEED + 2)
    Ap = np.asarray(prob["Adyn"], np.float64) * (1 + 0.05 * rng.standard_normal((nx, nx)))
    Bp = np.asarray(prob["Bdyn"], np.float64) * (1 + 0.05 * rng.standard_normal((nx, nu)))
    w = 0.01 * rng.standard_normal((STEPS, B, nx))
    want = SC.oracle_loop(O, prob, c["per"], c["x0"], c["ref"], c["bnds"], STEPS, c["adv"], plant=O.Oracle(dict(prob, Adyn=Ap, Bdyn=Bp), SC.DT).plant_step, w=w)
    a = loop_handle(T, c)
    a.set_plant(Ap, Bp)
    assert a.closed_loop_kernel_name() == SC.kernel_name(dims), "with a plant the run is the launch sequence of the ps solve kernel"
    u0, xs = a.mpc_run_sim(STEPS, c["adv"], w)
    assert same_bits(u0, want["u0"]) and same_bits(xs, want["xs"]), "replayed run with a plant: u0 / x_traj differ from the oracle's loop"
    check_loop_end(a, c, want, f"{dims} run with a plant")
    # without a plant, a call that passes w is a sequence too, under the name the handle alone gives
    a.clear_plant()
    assert a.closed_loop_kernel_name().endswith(",mpc,ps>")
    want = SC.oracle_loop(O, prob, c["per"], xs[-1], c["ref"], c["bnds"], STEPS, 0, w=w)
    if isinstance(c["ref"], tuple):
        a.set_xref_window(*c["ref"])
    a.set_state({k: np.zeros_like(v) for k, v in a.get_state().items()})   # a cold workspace again
    a.set_x0(xs[-1])
    u0, xs2 = a.mpc_run_sim(STEPS, 0, w)
    assert same_bits(u0, want["u0"]) and same_bits(xs2, want["xs"]), "run with w alone"
    a.close()


@pytest.mark.parametrize("dims", list(LOOPS), ids=lambda d: "x".join(map(str, d)))
def test_a_run_with_a_zero_budget_is_a_sequence(tinympc, oracle_mod, dims):
    T, O = tinympc, oracle_mod
    c = loop_case(T, O, dims)
    per = dict(c["per"], max_iter=c["per"]["max_iter"].copy())
    per["max_iter"][4] = 0
    want = SC.oracle_loop(O, c["prob"], per, c["x0"], c["ref"], c["bnds"], STEPS, c["adv"])
    assert (want["status"][:, 4] == 11).all() and (want["iter"][:, 4] == 1).all()
    a = loop_handle(T, c, per)
    assert a.closed_loop_kernel_name() == SC.kernel_name(dims), a.closed_loop_kernel_name()
    got = a.mpc_run_log(STEPS, c["adv"])
    for k in ("u0", "iter", "status"):
        assert same_bits(got[k], want[k]), f"run with a budget of 0: {k} differs from the oracle's loop"
    assert (got["status"][:, 4] == 11).all() and (got["iter"][:, 4] == 1).all()
    check_loop_end(a, c, want, f"{dims} run with a budget of 0")
    a.close()


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_check_termination_below_one_names_the_first_index(tinympc, oracle_mod):
    T = tinympc
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, (12, 4, 10), 9, "shared")
    s = handle(T, prob, x0, xref, bnds)
    ct = np.ones(9, np.int32)
    ct[3] = 0; ct[7] = -2
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-1: check_termination\[3\] = 0"):
        s.set_instance_settings(check_termination=ct)
    assert not s.settings_per_instance() and s.kernel_name() == "rows64<12,4,10>"
    s.close()


def test_set_instance_settings_needs_set_settings_first(tinympc):
    import ctypes as C
    lib = tinympc.load_library()
    h = C.c_void_p()
    assert lib.tiny_batch64_create(C.byref(h), 12, 4, 10, 5, 0) == 0
    mi = np.full(5, 3, np.int32)
    assert lib.tiny_batch64_set_instance_settings(h, None, None, mi.ctypes.data_as(C.POINTER(C.c_int)), None, None, None) == ENOTREADY
    assert b"set_settings" in lib.tiny_batch64_last_error() and lib.tiny_batch64_settings_per_instance(h) == 0
    lib.tiny_batch64_destroy(h)


@pytest.mark.parametrize("order", ["models first", "settings first"])
def test_per_instance_models_with_settings_are_refused_and_nothing_is_launched(tinympc, oracle_mod, order):
    T, O, B, dims = tinympc, oracle_mod, 6, (12, 4, 10)
    fam = T.problems.model_family("random", 3, B, seed=19, dims=dims[:2])
    mods = T.problems.family_caches(fam, riccati=O.riccati)
    prob = dict(mods["probs"][0], N=dims[2], u_min=-0.5, u_max=0.5, x_min=-5.0, x_max=5.0)
    x0, xref, bnds = closed_loop_inputs(prob, B, "inst", 5, dtype=SC.DT)
    s = handle(T, prob, x0, xref, bnds)
    up = random_warm_state(O, dims, B, 77)
    s.set_state(up)
    mi = np.arange(B, dtype=np.int32) % 5 + 1
    if order == "models first":
        s.set_models(mods); s.set_instance_settings(max_iter=mi)
    else:
        s.set_instance_settings(max_iter=mi); s.set_models(mods)
    assert s.kernel_name() == "unsupported" and s.closed_loop_kernel_name() == "unsupported"
    for call in (s.solve, s.mpc_step, lambda: s.mpc_run(2), s.update_slack, s.termination_condition):
        with pytest.raises(T.solver.TinyBatchError, match=r"rc=-3: per-instance settings together with per-instance models") as e:
            call()
    print(order, "->", e.value)
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert got[k].tobytes() == up[k].tobytes(), f"{k} was written by a refused call"
    # either clear brings a path back
    s.clear_instance_settings()
    assert s.kernel_name() == "rows64<12,4,10,pm>"
    s.set_instance_settings(max_iter=mi); s.clear_models()
    assert s.kernel_name() == "rows64<12,4,10,ps>"
    s.solve()
    s.close()
