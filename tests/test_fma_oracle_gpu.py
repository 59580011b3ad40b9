"""The fma-arithmetic kernels of the row family and tile16 against the fma-order mode of the CPU oracle (Oracle(..., arith="fma"), itself checked
without a GPU in tests/test_fma_oracle_host.py): BIT FOR BIT, signs of zeros included — all twelve work arrays, the four residual fields, iter,
status and the return code of solve, of every instance; no mask over instances whose iteration count changed, no share of allowed changes.

Fma arithmetic is a fully determined sequence of IEEE operations ("Fma arithmetic, operation by operation"), and fmaf is correctly rounded
on the CPU, so the plain-C restatement is a second statement of the same numbers.  Every case asserts the name of the kernel it runs on first, so that
a routing change cannot quietly move it to another kernel.

Out of scope here: quadlane, waveres, tile48, stream with the padded classes it serves, and the per-instance-model records sum in orders of their
own, which a restatement in C does not follow.  tests/test_fma_values_gpu.py holds them to the EXACT oracle by value instead, on rounding-free
inputs in which every term of every product is observable (proven in tests/test_fma_oracle_host.py); beyond those inputs they keep the yardstick
bar of tests/test_parity_gpu.py, unchanged.
"""
import numpy as np
import pytest

from helpers import STATE_ORDER, closed_loop_inputs, projection_problem, ref_at, rounding_free_case, same_bits
from test_parity_gpu import SCALARS, assert_bitwise

pytestmark = pytest.mark.gpu

# the settings rows: (id, settings over the defaults, bounds, reference); bounds "inst" = per-instance tables, reference "shared" / "inst" / "window"
ROWS = [("defaults", {}, "shared", "shared"), ("sparse_checks", dict(check_termination=3, max_iter=24), "shared", "shared"),
        ("one_iteration", dict(max_iter=1), "shared", "shared"), ("no_iteration", dict(max_iter=0), "shared", "shared"),
        ("bounds_off", dict(en_state_bound=0, en_input_bound=0, max_iter=30), "shared", "shared"),
        ("per_instance", dict(max_iter=40), "inst", "inst"), ("window", dict(max_iter=40), "shared", "window")]
SHARED_ROWS = [r for r in ROWS if r[2] == "shared"]


def _problem(pr, O, nx, nu, N):
    return projection_problem(pr, O, nx, nu, N)


def _inputs(pr, prob, B, seed, bmode, rmode, R=lambda a: a):
    """x0 as the fma tests of tests/test_parity_gpu.py draw it (and two instances at -0 and +0), boxes tight enough to bind, and the reference of the row"""
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx)).astype(np.float32)
    if B >= 4:   # two instances start at a zero of either sign
        x0[0], x0[1] = -0.0, 0.0
    shared = tuple(a * s for a, s in zip(pr.bounds_arrays(prob), (0.2, 0.2, 0.3, 0.3)))
    bnds = shared if bmode == "shared" else tuple((a[None] * rng.uniform(0.1, 1.0, size=(B,) + a.shape)).astype(np.float32) for a in shared)
    if rmode == "window":
        rows = N + 24
        table = (0.1 * rng.standard_normal((rows, nx))).astype(np.float32)
        start = rng.integers(0, rows - N + 1, size=B).astype(np.int32)
        ref = (R(table), start)
    else:
        ref = R((rng.standard_normal((N, nx) if rmode == "shared" else (B, N, nx)) * 0.1).astype(np.float32))
    return R(x0), tuple(R(b) for b in bnds), ref


def _warm_state(O, rng, B, nx, nu, N, R=lambda a: a, dual=lambda a: a):
    """a random workspace with 10 % +0 and 10 % -0 entries, as test_fp64_vs_oracle builds it; from four instances on, instance 0 is all -0, instance 1
    all +0 and instance 2 zeros of random signs: where every product of a chain is a zero, its sign tells a chain that starts with a plain product
    from one that starts with an fma on +0"""
    st = O.new_state(B, nx, nu, N)
    for k in STATE_ORDER:
        st[k][:] = (dual if k in ("g", "y") else R)((rng.standard_normal(st[k].shape) * 0.3).astype(np.float32))
    for k in ("x", "d", "v", "z", "g", "y"):
        st[k][rng.random(st[k].shape) < 0.1] = 0.0
        st[k][rng.random(st[k].shape) < 0.1] = -0.0
    if B >= 4:
        for k in STATE_ORDER:
            st[k][0], st[k][1], st[k][2] = -0.0, 0.0, np.copysign(0.0, rng.standard_normal(st[k][2].shape)).astype(np.float32)
    st["residuals"][:] = rng.random((B, 4)).astype(np.float32); st["iter"][:] = 3; st["status"][:] = 11
    return st


def _handle(T, prob, B, settings, select, family, bnds, ref, name, storage=None, models=None):
    """models: the dict set_models takes, one model per instance (prob then only gives the dimensions)"""
    sol = T.TinyBatchSolver(prob, B, settings={k: v for k, v in settings.items() if k not in ("en_uref", "en_coeff_d2p")})
    if models is not None:
        sol.set_models(models)
    if models is not None and family == 7:   # under models the row variants exist through the forced wave family only: the family first
        sol.set_row_kernel(family); sol.select_kernel(select)
    else:
        sol.select_kernel(select); sol.set_row_kernel(family)
    if storage:
        sol.set_storage(*storage)
    sol.set_bounds(*bnds)
    if isinstance(ref, tuple):
        sol.set_xref_window(*ref)
    else:
        sol.set_xref(ref)
    return sol


def _named(sol, name):
    got = sol.kernel_name()
    assert got.startswith(name) if isinstance(name, str) else name(got), f"the case runs on {got}"
    assert sol.arithmetic() == "fma", got


def _chain(T, O, prob, B, settings, family, name, bmode="shared", rmode="shared", seed=0, storage=None, dtype=np.float32, terms=None, what=""):
    """A cold solve, two warm solves with reset duals, then a solve from a random warm state with signed zeros and live duals: the kernel against the
    fma oracle, whose chain continues from its own state (by then the kernel's)."""
    pr = T.problems
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    h16 = isinstance(dtype, str)
    R = O.round_h16 if h16 else (lambda a: a)
    x0, bnds, ref = _inputs(pr, prob, B, seed, bmode, rmode, R)
    settings = dict(O.DEFAULT_SETTINGS, **settings)
    sol = _handle(T, prob, B, settings, 3, family, bnds, ref, name, storage)
    orc = O.Oracle(prob, dtype, settings, arith="fma")
    if terms is not None:
        sol.set_optional_terms(bool(settings.get("en_uref")), bool(settings.get("en_coeff_d2p")))
        sol.set_input_cost(prob["R"]); sol.set_coeff_d2p(prob["coeff_d2p"]); sol.set_uref(terms)
        orc.set_uref(terms)
    sol.set_x0(x0)
    _named(sol, name)
    xref = pr.expand_windows(*ref, N) if isinstance(ref, tuple) else ref
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = x0
    rng = np.random.default_rng(seed + 1000)
    for k in range(4):
        if k in (1, 2):
            st["y"][:] = 0; st["g"][:] = 0
            sol.reset_dual_variables()
        if k == 3:
            st = _warm_state(O, rng, B, nx, nu, N, R, dual=(lambda a: a) if dtype == "h16d" else R)
            sol.set_state(st)
        rc_ref = orc.solve(st, *bnds, xref, nthreads=8)
        rc = sol.solve()
        _named(sol, name)
        assert_bitwise(sol.get_state(), st, f"{what} {sol.kernel_name()} B={B} {settings} bounds {bmode} reference {rmode} solve {k}")
        assert rc == (1 if rc_ref else 0), (what, k, rc, rc_ref)
    iters = st["iter"]
    sol.close()
    return iters


def _rows(T, O, dims, family, name, rows, B=37, b1=True):
    prob = _problem(T.problems, O, *dims)
    for j, (rid, over, bmode, rmode) in enumerate(rows):
        _chain(T, O, prob, B, over, family, name, bmode, rmode, seed=j + dims[2], what=rid)
    if b1:
        _chain(T, O, prob, 1, {}, family, name, seed=77, what="B=1")


# ---- the fused solves -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (4, 1, 10), (8, 3, 7)])
def test_rowlane_fma_equals_the_fma_oracle(tinympc, oracle_mod, dims):
    """rowlane<nx,nu,N,fast> (set_row_kernel(1)): every settings row at B = 37 — ragged against the four instances of a wave — and B = 1"""
    _rows(tinympc, oracle_mod, dims, 1, "rowlane<{},{},{},fast".format(*dims), ROWS)


def test_rowlane_fma_long_horizon(tinympc, oracle_mod):
    """rowlane<12,4,30,fast>, once: the defaults and the sparse checks"""
    _rows(tinympc, oracle_mod, (12, 4, 30), 1, "rowlane<12,4,30,fast", ROWS[:2], b1=False)


@pytest.mark.parametrize("dims", [(12, 4, 17), (8, 4, 9), (2, 2, 3)])
def test_rowloop_fma_equals_the_fma_oracle(tinympc, oracle_mod, dims):
    """rowloop<nx,nu,fast> (set_row_kernel(2)), the classes of ROWLOOP_FMA in tests/test_closed_loop_gpu.py"""
    _rows(tinympc, oracle_mod, dims, 2, "rowloop<{},{},fast".format(*dims[:2]), ROWS)


def test_rowstream_fma_equals_the_fma_oracle(tinympc, oracle_mod):
    """the any-horizon row kernel with its state in HBM, where the automatic choice puts N = 65"""
    _rows(tinympc, oracle_mod, (12, 4, 65), 0, lambda n: n.startswith("rowstream<12,4") and "fast" in n, ROWS)


@pytest.mark.parametrize("N,B", [(10, 17), (10, 37), (30, 33)])
def test_tile16_fma_equals_the_fma_oracle(tinympc, oracle_mod, N, B):
    """tile16<12,4,N,fast> (set_row_kernel(5)) against the oracle directly, not through its tie to the row kernel: one live column beside a full tile,
    a second tile with five, a third with one"""
    _rows(tinympc, oracle_mod, (12, 4, N), 5, f"tile16<12,4,{N},fast>", SHARED_ROWS if N == 10 else SHARED_ROWS[:3], B=B, b1=(B == 37))


def test_tile16_fma_per_instance_tables_equal_the_fma_oracle(tinympc, oracle_mod):
    """tile16<12,4,10,fast,pi>: bounds and reference per instance, bounds alone, the reference alone"""
    T, O = tinympc, oracle_mod
    prob = _problem(T.problems, O, 12, 4, 10)
    for j, (over, bmode, rmode) in enumerate(((dict(max_iter=40), "inst", "inst"), ({}, "inst", "shared"), (dict(max_iter=24, check_termination=3), "shared", "inst"),
                                              (dict(max_iter=1), "inst", "window"))):
        _chain(T, O, prob, 37, over, 5, "tile16<12,4,10,fast,pi>", bmode, rmode, seed=40 + j, what="pi")
    _chain(T, O, prob, 1, {}, 5, "tile16<12,4,10,fast,pi>", "inst", "inst", seed=50, what="pi B=1")


@pytest.mark.parametrize("dual_bits", [16, 32])
def test_fp16_storage_fma_equals_the_fma_oracle(tinympc, oracle_mod, dual_bits):
    """fp16 storage with fma arithmetic, the 16-bit and the 32-bit duals, against the _h16 / _h16d fma oracle"""
    T, O = tinympc, oracle_mod
    prob = _problem(T.problems, O, 12, 4, 10)
    dtype, tag = ("h16", ",h16>") if dual_bits == 16 else ("h16d", ",h16d>")
    name = lambda n: n.startswith("rowlane<12,4,10,fast") and n.endswith(tag)
    for j, (rid, over, bmode, rmode) in enumerate(SHARED_ROWS[:3]):
        _chain(T, O, prob, 37, over, 1, name, seed=60 + j, storage=(16, dual_bits), dtype=dtype, what=f"fp16 storage {rid}")
    _chain(T, O, prob, 1, {}, 1, name, seed=70, storage=(16, dual_bits), dtype=dtype, what="fp16 storage B=1")


@pytest.mark.parametrize("case", ["uref", "coeff_d2p", "both"])
def test_optional_terms_fma_equal_the_fma_oracle(tinympc, oracle_mod, case):
    """The Uref term (quadrotor), the coeff_d2p term (cartpole) and both ((8,3,7)) on the `opt` instantiations of the unrolled kernel"""
    T, O = tinympc, oracle_mod
    dims = dict(uref=(12, 4, 10), coeff_d2p=(4, 1, 10), both=(8, 3, 7))[case]
    prob = dict(_problem(T.problems, O, *dims))
    nx, nu, N = dims
    rng = np.random.default_rng(nx * 7 + nu)
    prob["coeff_d2p"] = (rng.standard_normal((nx, nu)) * 0.02).astype(np.float32)
    prob["R"] = rng.uniform(0.5, 2.0, nu).astype(np.float32)
    B = 37
    uref = (rng.uniform(-0.3, 0.3, (B, N - 1, nu)) * prob["u_max"]).astype(np.float32)
    over = dict(max_iter=30, check_termination=2, en_uref=int(case != "coeff_d2p"), en_coeff_d2p=int(case != "uref"))
    _chain(T, O, prob, B, over, 1, "rowlane<{},{},{},fast".format(*dims), seed=80, terms=uref, what=f"optional terms {case}")
    _chain(T, O, prob, B, dict(over, max_iter=1), 1, "rowlane<{},{},{},fast".format(*dims), seed=81, terms=uref[0], what=f"optional terms {case}, shared Uref")


# ---- the six step functions -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(12, 4, 10), (4, 1, 10), (8, 3, 7)])
def test_step_functions_fma_equal_the_fma_oracle(tinympc, oracle_mod, dims):
    """Each fma step function of admm_steps.hip from the SAME random workspace against Oracle.step in fma mode — one sweep in isolation — then one
    iteration composed of the six.  check_termination = 2 with iter drawn from 1 .. 8: termination_condition must skip the odd ones."""
    T, O, pr = tinympc, oracle_mod, tinympc.problems
    prob = _problem(pr, O, *dims)
    nx, nu, N = dims
    B = 23
    rng = np.random.default_rng(7 + nx)
    settings = dict(O.DEFAULT_SETTINGS, check_termination=2, abs_pri_tol=0.5, abs_dua_tol=5.0)
    x0, bnds, xref = _inputs(pr, prob, B, 5, "inst", "inst")
    st0 = _warm_state(O, rng, B, nx, nu, N)
    for k in STATE_ORDER:   # every instance at its own magnitude, so that the tolerances separate them
        st0[k] *= rng.permutation(np.geomspace(0.02, 1.0, B)).astype(np.float32)[:, None, None]
    st0["iter"][:] = rng.integers(1, 9, size=B)
    assert (st0["iter"] % 2 == 1).any() and (st0["iter"] % 2 == 0).any()
    sol = T.TinyBatchSolver(prob, B, settings=settings)
    sol.select_kernel(3)
    sol.set_bounds(*bnds); sol.set_xref(xref)
    assert sol.arithmetic() == "fma", sol.kernel_name()
    orc = O.Oracle(prob, np.float32, settings, arith="fma")

    def check(st, what):
        got = sol.get_state()
        for k in STATE_ORDER + ("residuals", "iter", "status"):
            assert same_bits(got[k], st[k]), f"{dims} {what}: {k} differs"

    for fn in O.Oracle.STEP_FUNCTIONS:
        st = O.copy_state(st0)
        sol.set_state(st)
        ref_rv = orc.step(fn, st, *bnds, xref)
        rv = getattr(sol, fn)()
        if fn == "termination_condition":
            assert np.array_equal(rv, ref_rv), dims
            assert ref_rv.any() and not ref_rv.all(), "the tolerances of this case separate nothing"
        check(st, fn)
    st = O.copy_state(st0)
    sol.set_state(st)
    for fn in ("forward_pass", "update_slack", "update_dual", "update_linear_cost", "termination_condition"):
        orc.step(fn, st, *bnds, xref); getattr(sol, fn)()
    st["v"][:] = st["vnew"]; st["z"][:] = st["znew"]
    sol.set_array("v", sol.get_array("vnew")); sol.set_array("z", sol.get_array("znew"))
    orc.step("backward_pass_grad", st, *bnds, xref); sol.backward_pass_grad()
    check(st, "composed iteration")
    sol.close()


# ---- the closed loop on chip -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,name", [(1, "rowlane<12,4,10,fast>"), (5, "tile16<12,4,10,fast>")])
@pytest.mark.parametrize("sim", [False, True])
def test_closed_loop_fma_equals_the_fma_oracle_loop(tinympc, oracle_mod, family, name, sim):
    """mpc_run on chip, 6 steps of 17 instances over a window reference that advances by one row: per step {fma oracle solve; the reference's
    plant step; slide the window}.  sim: against a plant of its own (set_plant) with a disturbance per step (mpc_run_sim; tile16 hands such a run
    over to the 16-lane kernel).  u.col(0) of every step, the state after every plant step, the final workspace and x0 in bits."""
    T, O, pr = tinympc, oracle_mod, tinympc.problems
    prob = _problem(pr, O, 12, 4, 10)
    B, N, steps = 17, 10, 6
    settings = dict(O.DEFAULT_SETTINGS, max_iter=30)
    x0, ref, bnds = closed_loop_inputs(prob, B, "window", seed=11)
    rng = np.random.default_rng(12)
    plant = w = None
    if sim:
        plant = ((np.asarray(prob["Adyn"]) * (1 + 0.01 * rng.standard_normal((12, 12)))).astype(np.float32),
                 (np.asarray(prob["Bdyn"]) * (1 + 0.02 * rng.standard_normal((12, 4)))).astype(np.float32))
        w = (0.002 * rng.standard_normal((steps, B, 12))).astype(np.float32)
    # the oracle's loop
    fma = O.Oracle(prob, np.float32, settings, arith="fma")
    step = O.Oracle(dict(prob, Adyn=plant[0], Bdyn=plant[1]) if sim else prob, np.float32).plant_step
    st = O.new_state(B, 12, 4, N)
    x, u0s, xs = x0.copy(), [], []
    for k in range(steps):
        st["x"][:, 0] = x; st["y"][:] = 0; st["g"][:] = 0
        fma.solve(st, *bnds, ref_at(ref, k, 1, N, B), nthreads=8)
        u0s.append(st["u"][:, 0].copy())
        x = step(x, u0s[-1])
        if sim:
            x = (x + w[k]).astype(np.float32)
        xs.append(x.copy())
    st["x"][:, 0] = x
    its = st["iter"]
    assert (its == 30).any() and (its < 30).any(), "the case needs instances that run out of iterations and instances that converge"
    # the device's
    sol = _handle(T, prob, B, settings, 3, family, bnds, ref, name)
    sol.set_x0(x0)
    assert sol.kernel_name() == name, sol.kernel_name()
    if sim:
        sol.set_plant(*plant)
        assert sol.closed_loop_kernel_name() == "rowlane<12,4,10,fast>", sol.closed_loop_kernel_name()
        u, xt = sol.mpc_run_sim(steps, 1, w)
        assert same_bits(xt, np.array(xs)), f"{name}: the state trajectory differs"
    else:
        assert sol.closed_loop_kernel_name() == name, sol.closed_loop_kernel_name()
        u = sol.mpc_run_traj(steps, 1)
    assert same_bits(u, np.array(u0s)), f"{name} sim={sim}: u.col(0) differs from step {int(np.argmax([not same_bits(a, b) for a, b in zip(u, u0s)]))} on"
    assert same_bits(sol.get_x0(), x), f"{name} sim={sim}: the final x0 differs"
    assert_bitwise(sol.get_state(), st, f"{name} sim={sim}: final workspace")
    sol.close()


# ---- inputs on which nothing rounds: the device's fma mode against the EXACT oracle ---------------------------------------------------------------

@pytest.mark.parametrize("max_iter", [1, 2])
@pytest.mark.parametrize("dims,family,name", [((12, 4, 10), 1, "rowlane<12,4,10,fast"), ((8, 3, 7), 1, "rowlane<8,3,7,fast"), ((12, 4, 10), 5, "tile16<12,4,10,fast")])
def test_fma_kernels_equal_the_exact_oracle_where_nothing_rounds(tinympc, oracle_mod, dims, family, name, max_iter):
    """helpers.rounding_free_case on the device: a fused multiply-add and a multiply followed by an add coincide there, so the fma kernels must equal
    the EXACT oracle in value (signs of zeros excepted: the negated gains flip them).  Ties the two arithmetic modes together on the device,
    independent of the fma-order C code.  The premise — the fp32 exact oracle equals the fp64 one — is asserted here too."""
    T, O = tinympc, oracle_mod
    nx, nu, N = dims
    B = 37
    prob, settings, x0, xref, bnds, _ = rounding_free_case(nx, nu, N, B, seed=0)
    settings = dict(settings, max_iter=max_iter)
    if family == 5:   # the shared-table instantiation: one reference for the batch
        xref = xref[0]
    ref, ref64 = O.new_state(B, nx, nu, N), O.new_state(B, nx, nu, N, np.float64)
    ref["x"][:, 0] = x0; ref64["x"][:, 0] = x0
    rc_ref = O.Oracle(prob, np.float32, settings).solve(ref, *bnds, xref)
    O.Oracle(prob, np.float64, settings, allow_unpinned_dims=True).solve(ref64, *[b.astype(np.float64) for b in bnds], xref.astype(np.float64))
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(ref[k], ref64[k]), f"{dims}: the premise fails, {k} rounds in fp32"
    sol = _handle(T, prob, B, settings, 3, family, bnds, xref, name)
    sol.set_x0(x0)
    _named(sol, name)
    rc = sol.solve()
    got = sol.get_state()
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(got[k], ref[k]), f"{sol.kernel_name()} max_iter={max_iter}: {k} differs from the exact oracle in value"
    assert rc == (1 if rc_ref else 0)
    sol.close()
