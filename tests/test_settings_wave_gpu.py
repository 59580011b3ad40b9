"""Per-instance settings (tiny_batch_set_instance_settings) on the two wave kernels: admm_waveres_ps_kernel and admm_wavestream_ps_kernel, reached with
tiny_batch_set_row_kernel(tb, 7) / (tb, 6) for the classes with 16 < nx + nu <= 64.  One wavefront is one instance there, so an instance's record is a
wave-uniform value and the iteration loop runs to the instance's own budget.

Exact arithmetic is compared bit for bit — the 12 work arrays, the 4 residuals, iter, status, the signs of zeros — with the oracle run once per
distinct settings tuple (settings_cases.per_group).  fma arithmetic (waveres only) has no bitwise oracle for these classes: its reference is the
unchanged batch-shared waveres<...,fast> kernel, run once per settings tuple on that tuple's instances.  tests/test_settings_wave_host.py shows on the
CPU that the draw is not vacuous for these classes."""
import numpy as np
import pytest

import settings_cases as SC
from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_inputs, oracle_closed_loop, same_bits

pytestmark = pytest.mark.gpu

FAMILY = {7: "waveres", 6: "wavestream"}


def wave_handle(T, prob, x0, xref, bnds, family, variant=0, settings=SC.BASE):
    s = T.TinyBatchSolver(prob, len(x0), settings=settings)
    s.set_bounds(*bnds); s.set_xref(xref)
    s.reset_workspace(); s.set_x0(x0)   # a cold start: reset_workspace() is folded into the launch
    s.set_row_kernel(family); s.select_kernel(variant)
    return s


@pytest.fixture(scope="module")
def routed_name(tinympc, oracle_mod):
    """what a forced family 7 reports under per-instance settings"""
    T = tinympc
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, (16, 4, 3), 2, "shared")
    s = wave_handle(T, prob, x0, xref, bnds, 7)
    s.set_instance_settings(max_iter=np.array([1, 2], np.int32))
    name = s.kernel_name()
    s.close()
    return name


@pytest.fixture(autouse=True)
def the_routing_is_there(routed_name):
    """without the feature every test of this file fails here: the forced wave family is "unsupported" under per-instance settings"""
    assert routed_name == "waveres<16,4,exact,ps>", routed_name


def assert_same(got, want, what):
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {int((np.asarray(got[k]) != np.asarray(want[k])).sum())} elements (or in the sign of a zero)"


def two_solves_against_the_oracle(T, O, dims, B, bounds, family, variant):
    """a cold solve under draw(B, SEED), then a warm solve under draw(B, SEED + 1) from the state the first settings left"""
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, bounds)
    s = wave_handle(T, prob, x0, xref, bnds, family, variant)
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    for k, what in enumerate(("cold", "warm, other settings")):
        per = SC.draw(B, SC.SEED + k)
        s.set_instance_settings(**per)
        assert s.settings_per_instance() and s.kernel_name() == f"{FAMILY[family]}<{dims[0]},{dims[1]},exact,ps>", s.kernel_name()
        rc = s.solve()
        assert s.dispatch_applied() == 0
        n_unsolved = SC.oracle_solve(O, prob, np.float32, per, st, bnds, xref)
        assert_same(s.get_state(), st, f"{dims} {bounds} B={B} {what}")
        assert rc == (1 if n_unsolved else 0), "tiny_batch_solve returns 1 iff some instance did not converge within its own budget"
    s.close()


# ---- 1: waveres, exact arithmetic ---------------------------------------------------------------------------------------------------------------
# the (16, 4) horizons are the edges of StepRegs (the 32-register vector, the 16-register vector, the two scalars); (16, 8): the GEMV orders

WAVERES = [(16, 4, 3), (16, 4, 10), (16, 4, 34), (16, 4, 50), (16, 8, 10), (24, 4, 10), (32, 16, 50)]
WAVERES_CASES = [(d, B) for d in WAVERES for B in (1, 37)]


@pytest.mark.parametrize("case", WAVERES_CASES, ids=[f"{'x'.join(map(str, d))}-B{B}" for d, B in WAVERES_CASES])
def test_waveres_ps_equals_the_oracle_per_instance(tinympc, oracle_mod, case):
    dims, B = case
    i = WAVERES_CASES.index(case)
    two_solves_against_the_oracle(tinympc, oracle_mod, dims, B, ("shared", "inst")[(i // 2 + i) % 2], 7, (0, 2)[i % 2])


# ---- 2: wavestream ------------------------------------------------------------------------------------------------------------------------------
# N = 51 is a horizon beyond waveres; 2 051 instances reach the (1, 3) shape and more than one round of the chip

WAVESTREAM_CASES = [(16, 4, 10, 37), (16, 4, 51, 37), (32, 16, 50, 5), (16, 4, 10, 2051)]


@pytest.mark.parametrize("case", WAVESTREAM_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-B{c[3]}" for c in WAVESTREAM_CASES])
def test_wavestream_ps_equals_the_oracle_per_instance(tinympc, oracle_mod, case):
    i = WAVESTREAM_CASES.index(case)
    two_solves_against_the_oracle(tinympc, oracle_mod, case[:3], case[3], ("inst", "shared")[i % 2], 6, (2, 0)[i % 2])


# ---- 3: waveres, fma arithmetic -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(16, 4, 34), (32, 16, 50)], ids=lambda d: "x".join(map(str, d)))
def test_waveres_ps_fma_equals_the_shared_fma_kernel_per_settings_tuple(tinympc, oracle_mod, dims):
    """the reference: waveres<...,fast> with one set of settings, forced family 7, once per settings tuple on that tuple's instances, started from the
    state the previous solve left them in.  An instance without a budget is compared with its untouched state: status 11 and iter 1 only"""
    T, O, B = tinympc, oracle_mod, 37
    bounds = "inst" if dims[0] == 16 else "shared"
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, bounds)
    s = wave_handle(T, prob, x0, xref, bnds, 7, 3)
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    for k in range(2):
        per = SC.draw(B, SC.SEED + k)
        s.set_instance_settings(**per)
        assert s.kernel_name() == f"waveres<{dims[0]},{dims[1]},fast,ps>", s.kernel_name()
        rc = s.solve()
        groups = {}
        for b in range(B):
            groups.setdefault(tuple(SC.settings_of(per, b).items()), []).append(b)
        for key, idx in groups.items():
            idx, settings = np.array(idx), dict(key)
            if settings["max_iter"] == 0:
                st["status"][idx] = 11; st["iter"][idx] = 1
                continue
            r = wave_handle(T, prob, x0[idx], xref[idx], tuple(a[idx] if a.ndim == 3 else a for a in bnds), 7, 3, settings)
            assert r.kernel_name() == f"waveres<{dims[0]},{dims[1]},fast>", r.kernel_name()
            if k:
                r.set_state({n: np.ascontiguousarray(v[idx]) for n, v in st.items()})   # (a warm solve: nothing is pending any more)
            r.solve()
            sub = r.get_state()
            r.close()
            for n in st:
                st[n][idx] = sub[n]
        assert_same(s.get_state(), st, f"{dims} fma, solve {k}")
        assert rc == (1 if (st["status"] != 1).any() else 0)
        assert all(np.isfinite(st[n]).all() for n in STATE_ORDER + ("residuals",))
    s.close()


# ---- 4: uniform arrays are the shared kernel, clear is the parent ---------------------------------------------------------------------------------

@pytest.mark.parametrize("family,variant,name", [(7, 2, "waveres<16,8,exact{}>"), (7, 3, "waveres<16,8,fast{}>"), (6, 2, "wavestream<16,8,exact{}>")],
                         ids=["waveres-exact", "waveres-fma", "wavestream"])
def test_uniform_settings_equal_the_shared_kernel_and_clear_restores_it(tinympc, oracle_mod, family, variant, name):
    T, B, dims = tinympc, 21, (16, 8, 10)
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, dims, B, "shared")
    settings = dict(SC.BASE, max_iter=9, check_termination=2, abs_pri_tol=3e-2, abs_dua_tol=2e-2)
    s = wave_handle(T, prob, x0, xref, bnds, family, variant, settings)

    def two_solves():
        s.reset_workspace(); s.set_x0(x0)
        s.solve(); s.solve()
        return s.get_state()
    assert s.kernel_name() == name.format("") and not s.settings_per_instance(), s.kernel_name()
    want = two_solves()
    assert (want["status"] == 1).any() and (want["status"] == 11).any()
    s.set_instance_settings(**{k: np.full(B, settings[k]) for k in SC.FIELDS})
    assert s.kernel_name() == s.closed_loop_kernel_name() == name.format(",ps"), s.kernel_name()
    assert_same(two_solves(), want, "uniform per-instance arrays")
    s.set_instance_settings(max_iter=9)   # a scalar broadcasts, NULL fields keep the batch's values
    assert s.kernel_name() == name.format(",ps"), s.kernel_name()
    assert_same(two_solves(), want, "one broadcast field, the rest NULL")
    s.clear_instance_settings()
    assert s.kernel_name() == name.format("") and not s.settings_per_instance()
    assert_same(two_solves(), want, "after clear")
    s.close()


# ---- 5: bound flags per instance ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", [7, 6], ids=["waveres", "wavestream"])
def test_bound_flags_per_instance_fold_into_the_table(tinympc, oracle_mod, family):
    """shared bound inputs, state and input bounds on for every other instance: the {lo, hi} table becomes per instance at row width 64; neighbours
    2k, 2k + 1 start from the same x0 and reference"""
    T, O, B, dims = tinympc, oracle_mod, 18, (16, 4, 10)
    prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, "shared")
    x0[1::2] = x0[0::2]; xref[1::2] = xref[0::2]
    on = (np.arange(B) % 2 == 0).astype(np.int32)
    per = dict(en_state_bound=on, en_input_bound=on, max_iter=np.full(B, 12, np.int32))
    s = wave_handle(T, prob, x0, xref, bnds, family)
    s.set_instance_settings(**per)
    assert s.kernel_name() == f"{FAMILY[family]}<16,4,exact,ps>", s.kernel_name()
    s.solve()
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    SC.oracle_solve(O, prob, np.float32, per, st, bnds, xref)
    got = s.get_state()
    assert_same(got, st, "alternating bound flags")
    differ = np.zeros(B // 2, bool)
    for k in STATE_ORDER:
        differ |= (got[k][0::2] != got[k][1::2]).reshape(B // 2, -1).any(1)
    assert differ.any(), "no pair of neighbours that differs: the bounds bind nowhere"
    # uniform flag arrays keep the shared table, and switch the bounds off for everyone
    s.set_instance_settings(en_state_bound=0, en_input_bound=0, max_iter=12)
    s.reset_workspace(); s.set_x0(x0); s.solve()
    st = O.new_state(B, *dims)
    st["x"][:, 0] = x0
    SC.oracle_solve(O, prob, np.float32, dict(en_state_bound=0 * on, en_input_bound=0 * on, max_iter=per["max_iter"]), st, bnds, xref)
    assert_same(s.get_state(), st, "uniform flags, all off")
    s.close()


# ---- 6: the closed loop -------------------------------------------------------------------------------------------------------------------------

STEPS = 3
LOOP_CASES = [((16, 4, 10), 7), ((24, 4, 10), 6)]
_loops = {}


def _loop_case(T, O, dims):
    """(prob, x0, ref, bnds, per, the oracle's loop per settings tuple): computed once per class, shared by the tests and left unchanged"""
    if dims not in _loops:
        B = 37
        prob = SC.problem(T.problems, O, dims)
        x0, ref, bnds = closed_loop_inputs(prob, B, "window", SC.SEED)
        per = SC.draw(B)
        per["max_iter"] = np.maximum(per["max_iter"], 1)   # a run needs a budget for every instance
        nx, nu, N = dims
        total = STEPS + 2
        want = dict(u0=np.zeros((total, B, nu), np.float32), iter=np.zeros((total, B), np.int32), status=np.zeros((total, B), np.int32), x=np.zeros((2, B, nx), np.float32),
                    st=[O.new_state(B, *dims), O.new_state(B, *dims)])
        groups = {}
        for b in range(B):
            groups.setdefault(tuple(SC.settings_of(per, b).items()), []).append(b)
        for key, idx in groups.items():
            idx = np.array(idx)
            out = oracle_closed_loop(O, prob, np.float32, dict(key), x0[idx], (ref[0], ref[1][idx]), bnds, STEPS, 1)
            for k in ("u0", "iter", "status"):
                want[k][:STEPS, idx] = out[k]
            want["x"][0, idx] = out["x"]
            for k in want["st"][0]:
                want["st"][0][k][idx] = out["st"][k]
            more = oracle_closed_loop(O, prob, np.float32, dict(key), out["x"], (ref[0], ref[1][idx] + STEPS), bnds, 2, 1, st=out["st"])   # a second run continues
            for k in ("u0", "iter", "status"):
                want[k][STEPS:, idx] = more[k]
            want["x"][1, idx] = more["x"]
            for k in want["st"][1]:
                want["st"][1][k][idx] = more["st"][k]
        _loops[dims] = (prob, x0, ref, bnds, per, want)
    return _loops[dims]


def _loop_handle(T, prob, x0, ref, bnds, per, family):
    s = T.TinyBatchSolver(prob, len(x0), settings=SC.BASE)
    s.set_bounds(*bnds); s.set_xref_window(*ref); s.set_x0(x0)
    s.set_row_kernel(family)
    s.set_instance_settings(**per)
    return s


@pytest.mark.parametrize("dims,family", LOOP_CASES, ids=["16x4x10-waveres", "24x4x10-wavestream"])
def test_closed_loop_equals_the_oracle_loop_per_settings_tuple(tinympc, oracle_mod, dims, family):
    T, O = tinympc, oracle_mod
    prob, x0, ref, bnds, per, want = _loop_case(T, O, dims)
    assert len(set(want["iter"][0])) > 3 and (want["status"] == 1).any() and (want["status"] == 11).any()
    name = f"{FAMILY[family]}<{dims[0]},{dims[1]},exact,ps>"
    a = _loop_handle(T, prob, x0, ref, bnds, per, family)
    assert a.closed_loop_kernel_name() == name, a.closed_loop_kernel_name()
    for k in range(STEPS):
        a.mpc_step_async(1)
        it, stt, _ = a.get_status()
        assert same_bits(a.get_u()[:, 0], want["u0"][k]) and np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"step {k}"
    assert same_bits(a.get_x0(), want["x"][0])
    assert_same(a.get_state(), want["st"][0], "step by step")
    a.close()
    b = _loop_handle(T, prob, x0, ref, bnds, per, family)
    b.mpc_run_async(STEPS, 1)
    assert same_bits(b.get_x0(), want["x"][0]), "mpc_run_async: final x0"
    assert_same(b.get_state(), want["st"][0], "mpc_run_async")
    assert b.lib.tiny_batch_debug_graph_captures(b._h) == 1, "the run is one captured graph of (solve, plant kernel) x steps"
    b.mpc_run_async(2, 1)
    assert same_bits(b.get_x0(), want["x"][1]), "second mpc_run_async: final x0"
    assert_same(b.get_state(), want["st"][1], "second mpc_run_async")
    b.close()
    c = _loop_handle(T, prob, x0, ref, bnds, per, family)
    assert same_bits(c.mpc_run_traj(STEPS, 1), want["u0"][:STEPS]), "mpc_run_traj: u0 trajectory"
    assert same_bits(c.get_x0(), want["x"][0])
    c.close()
    d = _loop_handle(T, prob, x0, ref, bnds, per, family)
    got = d.mpc_run_log(STEPS, 1)
    for k in ("u0", "iter", "status"):
        assert same_bits(got[k], want[k][:STEPS]), f"mpc_run_log: {k} differs from the oracle's loop"
    assert_same(d.get_state(), want["st"][0], "mpc_run_log")
    d.close()


@pytest.mark.parametrize("case,plant", [(0, "inst"), (1, "shared")], ids=["16x4x10-waveres-plant-per-instance", "24x4x10-wavestream-shared-plant"])
def test_closed_loop_against_a_plant_with_a_disturbance(tinympc, oracle_mod, case, plant):
    """mpc_run_sim with one plant for the batch or a plant per instance, a disturbance and the state trajectory: per step y = g = 0, tiny_solve per
    settings tuple, x = (A_p x + B_p u0) + w with the instance's plant"""
    T, O = tinympc, oracle_mod
    dims, family = LOOP_CASES[case]
    nx, nu, N = dims
    prob, x0, ref, bnds, per, _ = _loop_case(T, O, dims)
    B = len(x0)
    rng = np.random.default_rng(SC.SEED + 2 + case)
    lead = (B,) if plant == "inst" else ()
    Ap = (np.asarray(prob["Adyn"], np.float64) * (1 + 0.05 * rng.standard_normal(lead + (nx, nx)))).astype(np.float32)
    Bp = (np.asarray(prob["Bdyn"], np.float64) * (1 + 0.05 * rng.standard_normal(lead + (nx, nu)))).astype(np.float32)
    w = (0.01 * rng.standard_normal((STEPS, B, nx))).astype(np.float32)
    if plant == "inst":
        plants = [O.Oracle(dict(prob, Adyn=a, Bdyn=b), np.float32) for a, b in zip(Ap, Bp)]
        step = lambda x, u0: np.concatenate([o.plant_step(x[b:b + 1], u0[b:b + 1]) for b, o in enumerate(plants)])
    else:
        step = O.Oracle(dict(prob, Adyn=Ap, Bdyn=Bp), np.float32).plant_step
    st = O.new_state(B, *dims)
    x, u0s, xs = x0.copy(), [], []
    for k in range(STEPS):
        st["x"][:, 0] = x; st["y"][:] = 0; st["g"][:] = 0
        xr = np.ascontiguousarray(ref[0][np.minimum(ref[1][:, None] + k + np.arange(N)[None], len(ref[0]) - 1)])
        SC.oracle_solve(O, prob, np.float32, per, st, bnds, xr)
        u0 = st["u"][:, 0].copy()
        x = (step(x, u0) + w[k]).astype(np.float32)
        u0s.append(u0); xs.append(x.copy())
    st["x"][:, 0] = x
    s = _loop_handle(T, prob, x0, ref, bnds, per, family)
    s.set_plant(Ap, Bp)
    assert s.closed_loop_kernel_name() == f"{FAMILY[family]}<{nx},{nu},exact,ps>", s.closed_loop_kernel_name()
    u, xt = s.mpc_run_sim(STEPS, 1, w)
    assert s.lib.tiny_batch_debug_graph_captures(s._h) == 1, "a simulated run on a wave kernel is a replayed launch sequence"
    assert same_bits(u, np.array(u0s)) and same_bits(xt, np.array(xs))
    assert same_bits(s.get_x0(), x)
    assert_same(s.get_state(), st, "mpc_run_sim")
    s.close()


@pytest.mark.parametrize("dims,family", LOOP_CASES, ids=["16x4x10-waveres", "24x4x10-wavestream"])
def test_a_run_with_a_zero_budget_is_refused_and_writes_nothing(tinympc, oracle_mod, dims, family):
    T, O = tinympc, oracle_mod
    prob, x0, ref, bnds, per, _ = _loop_case(T, O, dims)
    per = dict(per, max_iter=per["max_iter"].copy())
    per["max_iter"][4] = 0
    s = _loop_handle(T, prob, x0, ref, bnds, per, family)
    before = s.get_state()
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-1: .*max_iter > 0 for every instance"):
        s.mpc_run_log(STEPS, 1)
    assert_same(s.get_state(), before, "a refused run")
    assert same_bits(s.get_x0(), x0)
    s.close()


# ---- 7: routing and refusals --------------------------------------------------------------------------------------------------------------------

def test_names_of_every_combination_served(tinympc, oracle_mod):
    T = tinympc
    for dims in ((16, 4, 10), (32, 16, 50)):
        nx, nu, _ = dims
        prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, dims, 5, "shared")
        s = wave_handle(T, prob, x0, xref, bnds, 7)
        s.set_instance_settings(max_iter=np.arange(5, dtype=np.int32) + 1)
        for family, variant, name in ((7, 0, "waveres<{},{},exact,ps>"), (7, 2, "waveres<{},{},exact,ps>"), (7, 3, "waveres<{},{},fast,ps>"),
                                      (6, 0, "wavestream<{},{},exact,ps>"), (6, 2, "wavestream<{},{},exact,ps>")):
            s.select_kernel(0); s.set_row_kernel(family); s.select_kernel(variant)
            assert s.kernel_name() == s.closed_loop_kernel_name() == name.format(nx, nu), (family, variant, s.kernel_name())
            assert s.arithmetic() == ("fma" if variant == 3 else "exact")
        s.close()


def _refused(T, s, x0, what, text=r"rc=-3: .*per-instance.{10,}"):
    """with per-instance settings installed the handle's solve is TINY_BATCH_EUNSUPPORTED with a text; after clear it solves as before"""
    s.reset_workspace(); s.set_x0(x0); s.solve()
    want, name = s.get_state(), s.kernel_name()
    s.set_instance_settings(max_iter=np.arange(len(x0)) % 5 + 1)
    assert s.kernel_name() == s.closed_loop_kernel_name() == "unsupported", (what, s.kernel_name())
    s.reset_workspace(); s.set_x0(x0)
    with pytest.raises(T.solver.TinyBatchError, match=text) as e:
        s.solve()
    print(what, "->", e.value)
    s.clear_instance_settings()
    assert s.kernel_name() == name
    s.reset_workspace(); s.set_x0(x0); s.solve()
    assert_same(s.get_state(), want, f"{what}: after clear")
    s.close()


def _handle_32_16_10(T, O, B=6):
    prob = T.problems.random_system(32, 16, 10, seed=3216, riccati=O.riccati)
    x0, xref, bnds = closed_loop_inputs(prob, B, "inst", 5)
    s = T.TinyBatchSolver(prob, B, settings=SC.BASE)
    s.set_bounds(*bnds); s.set_xref(xref)
    return s, x0


def test_the_automatic_choice_stays_refused_and_points_to_the_wave_families(tinympc, oracle_mod):
    s, x0 = _handle_32_16_10(tinympc, oracle_mod)
    _refused(tinympc, s, x0, "nx + nu = 48, no forced family", r"rc=-3: .*per-instance.{10,}tiny_batch_set_row_kernel\(tb, 6 or 7\)")


def test_forced_tile48_is_refused(tinympc, oracle_mod):
    s, x0 = _handle_32_16_10(tinympc, oracle_mod)
    s.set_row_kernel(8)
    assert s.kernel_name() == "tile48<32,16,10,exact>", s.kernel_name()
    _refused(tinympc, s, x0, "forced tile48", r"rc=-3: the forced row kernel tile48 .*has no per-instance-settings form.{10,}")


@pytest.mark.parametrize("variant,name", [(1, "stream<8,4>"), (4, "generic<32,16,exact>")])
def test_the_mfma_streaming_and_the_run_time_dimension_variant_are_refused(tinympc, oracle_mod, variant, name):
    s, x0 = _handle_32_16_10(tinympc, oracle_mod)
    s.set_row_kernel(7)
    s.select_kernel(variant)
    assert s.kernel_name() == name, s.kernel_name()
    _refused(tinympc, s, x0, f"variant {variant} under a forced wave family", rf"rc=-3: per-instance settings are implemented by the row variants only.*variant {variant} holds")


def test_fma_on_the_streaming_wave_kernel_is_refused(tinympc, oracle_mod):
    """family 6 under variant 3 keeps the text it has without settings; the variant is selected on family 7, where it exists"""
    T = tinympc
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, (16, 4, 10), 6, "shared")
    s = wave_handle(T, prob, x0, xref, bnds, 7, 3)
    s.solve()
    want = s.get_state()
    s.set_instance_settings(max_iter=np.arange(6) % 5 + 1)
    assert s.kernel_name() == "waveres<16,4,fast,ps>"
    s.set_row_kernel(6)
    assert s.kernel_name() == "unsupported"
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-3: fma arithmetic for 16 < nx \+ nu <= 64 needs the state-on-chip wave kernel"):
        s.solve()
    s.set_row_kernel(7)
    s.clear_instance_settings()
    assert s.kernel_name() == "waveres<16,4,fast>"
    s.reset_workspace(); s.set_x0(x0); s.solve()
    assert_same(s.get_state(), want, "after clear")
    s.close()


@pytest.mark.parametrize("family", [7, 6])
def test_the_optional_terms_stay_refused_on_a_forced_wave_family(tinympc, oracle_mod, family):
    """no wave kernel reads coeff_d2p or Uref: such a handle is refused without settings, and installing settings does not turn that into a solve"""
    T = tinympc
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, (16, 4, 10), 6, "shared")
    s = wave_handle(T, prob, x0, xref, bnds, family)
    s.solve()
    want, name = s.get_state(), s.kernel_name()
    s.set_optional_terms(en_coeff_d2p=True)
    s.set_coeff_d2p(np.full((16, 4), 0.01, np.float32))
    text = r"rc=-3: the optional Uref / coeff_d2p terms \(tiny_batch_set_optional_terms\) are implemented by the row kernels for nx \+ nu <= 16 only"
    for settings in (False, True):
        if settings:
            s.set_instance_settings(max_iter=np.arange(6) % 5 + 1)
        assert s.kernel_name() == s.closed_loop_kernel_name() == "unsupported", (settings, s.kernel_name())
        s.reset_workspace(); s.set_x0(x0)
        with pytest.raises(T.solver.TinyBatchError, match=text):
            s.solve()
    s.set_optional_terms()
    assert s.kernel_name() == name[:-1] + ",ps>", s.kernel_name()   # the terms off: the settings are served again
    s.clear_instance_settings()
    assert s.kernel_name() == name
    s.reset_workspace(); s.set_x0(x0); s.solve()
    assert_same(s.get_state(), want, "after the terms are off and the settings cleared")
    s.close()


def test_waveres_is_refused_beyond_its_horizon_as_without_settings(tinympc, oracle_mod):
    T = tinympc
    prob, x0, xref, bnds = SC.inputs(T.problems, oracle_mod, (16, 4, 51), 6, "shared")
    s = T.TinyBatchSolver(prob, 6, settings=SC.BASE)
    s.set_bounds(*bnds); s.set_xref(xref)
    s.reset_workspace(); s.set_x0(x0); s.solve()
    want, name = s.get_state(), s.kernel_name()
    s.set_instance_settings(max_iter=np.arange(6) % 5 + 1)
    with pytest.raises(T.solver.TinyBatchError, match="row kernel 7 has no instantiation"):
        s.set_row_kernel(7)
    assert s.kernel_name() == "unsupported"   # no family is forced: the automatic choice stays refused
    with pytest.raises(T.solver.TinyBatchError, match=r"rc=-3: .*per-instance.{10,}"):
        s.solve()
    s.clear_instance_settings()
    assert s.kernel_name() == name
    s.reset_workspace(); s.set_x0(x0); s.solve()
    assert_same(s.get_state(), want, "after clear")
    s.close()


@pytest.mark.parametrize("family", [7, 6])
def test_models_together_with_settings_are_refused(tinympc, oracle_mod, family):
    T, B = tinympc, 6
    fam = T.problems.model_family("random", 3, B, seed=500, dims=(16, 4))
    mods = T.problems.family_caches(fam)
    prob = dict(mods["probs"][0], N=10, u_min=-0.5, u_max=0.5, x_min=-2.0, x_max=2.0)
    x0, xref, bnds = closed_loop_inputs(prob, B, "inst", 5)
    s = T.TinyBatchSolver(prob, B, settings=SC.BASE)
    s.set_models(mods)
    s.set_bounds(*bnds); s.set_xref(xref)
    s.set_row_kernel(family)
    assert s.kernel_name() == f"{FAMILY[family]}<16,4,exact,pm>", s.kernel_name()
    _refused(T, s, x0, f"models + settings on forced family {family}")


# ---- 8: guard zones -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 37])
def test_ps_wave_kernels_stay_inside_their_allocations(tinympc, oracle_mod, B):
    """both ps kernels (waveres in both arithmetic forms), the per-instance bounds table at row width 64 and a replayed run under
    tiny_batch_debug_guards(1): nothing outside the instance's own rows and the settings records is written"""
    T, O, dims = tinympc, oracle_mod, (16, 4, 10)
    T.solver.debug_guards(True)
    try:
        for family, variant, bounds, flags in ((7, 2, "shared", True), (7, 3, "inst", False), (6, 2, "shared", True), (6, 0, "inst", False)):
            prob, x0, xref, bnds = SC.inputs(T.problems, O, dims, B, bounds)
            s = wave_handle(T, prob, x0, xref, bnds, family, variant)
            s.set_instance_settings(**SC.draw(B, flags=flags))
            assert s.kernel_name().endswith(",ps>")
            s.solve()
            per = SC.draw(B, SC.SEED + 1)
            per["max_iter"] = np.maximum(per["max_iter"], 1)
            s.set_instance_settings(**per)
            s.mpc_run_async(2, 0)
            st = s.get_state()
            assert all(np.isfinite(st[k]).all() for k in STATE_ORDER + ("residuals",)), (family, variant, bounds)
            assert T.solver.debug_check() == 0, (family, variant, bounds, B)
            s.close()
    finally:
        T.solver.debug_guards(False)
