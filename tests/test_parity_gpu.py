"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C-ABI,
against (a) the golden vectors produced by the compiled reference, (b) the CPU oracle on seeded
inputs, and (c) size-independent properties at BASELINE.json's full batch sizes.

Two arithmetic modes exist and each has its own bar, written here because the work is floating point:

EXACT arithmetic (rowlane kernel, `exact` variants): every product and sum is rounded separately and
  summed in the order the reference's SSE2 Eigen build uses => results must be BITWISE EQUAL to the
  reference: all twelve work arrays, the four residuals, status and iter.

FAST arithmetic (fma chains: v_mfma_f32_16x16x4_f32 in the streaming kernel, v_fmac_f32_dpp in the
  rowlane kernel): one rounding per multiply-add instead of two, so bit equality is impossible.  ADMM
  with the examples' early exit (residual < 1e-3) is rounding sensitive: the reference's OWN fp64 and fp32
  builds disagree on the iteration count of ~47 % of the tracking instances and on u by up to 6e-5
  (tests/fuzz/parity_yardstick.py).  BASELINE.json's "u* within 1e-5" therefore cannot be met even by the
  reference against itself; the bar used instead is the reference's own precision spread, measured on the
  same inputs with the fp64 oracle (bit-exact with the reference's fp64 build, tests/test_oracle.py):
    * per array, over instances whose iteration count agrees, relative inf-norm error (normalised by
      max(|ref|_inf, natural scale)) <= 4 x the fp64-vs-fp32 spread of the same array, with an absolute
      floor of 2e-5 (u, z, znew) / 5e-5 (everything else) for tiny batches;
    * fraction of instances whose iteration count differs from the fp32 reference <= max(1.5 x the
      fp64-vs-fp32 fraction, 2 %), and never by more than the fp64 spread + 2 termination checks;
    * hard cap regardless of the yardstick: u within 3e-4 of the reference relative to the input bound.
  The fma kernels of the row family (rowlane, rowloop, rowstream, the step functions) and tile16 now ALSO have a bitwise bar: the
  fma-order mode of the oracle, tests/test_fma_oracle_gpu.py.  The yardstick tests here stay as they are; they alone guard the fma
  kernels that sum in an order of their own (quadlane, the wave kernels, tile48, stream).
"""
import numpy as np
import pytest

from helpers import STATE_ORDER, bounds_of, load_fixture, rel_inf

pytestmark = pytest.mark.gpu

PRIMAL_X = ("x", "v", "vnew")
PRIMAL_U = ("u", "z", "znew")
SCALARS = ("iter", "status", "residuals")

# kernel variants under test: (select_kernel id, exact?, set_row_kernel family: 0 auto = rowlane where instantiated)
VARIANTS = {"row_exact": (2, True, 0), "row_fast": (3, False, 0), "stream": (1, False, 0),
            "loop_exact": (2, True, 2), "loop_fast": (3, False, 2), "rowstream_exact": (2, True, 3),
            "lane_exact": (2, True, 1),  # auto prefers quadlane for nx=4, nu=1: keep the 16-lane kernel covered there too
            # 16 instances per wave, products on the matrix cores (admm_tile16.hip; quadrotor N=30 only): exact = K=1 MFMA products
            # + reference-order sums, bitwise like the row kernels; fma = MFMA chains, bitwise equal to the row kernels' fma mode
            "tile_exact": (2, True, 5), "tile_fast": (3, False, 5)}


def _floor(name, prob, ref):
    if name in PRIMAL_U:
        return max(abs(prob["u_max"]), abs(prob["u_min"]), 1e-3)
    if name in PRIMAL_X:
        return 1.0
    return max(float(np.max(np.abs(ref))), 1.0)


def yardstick(O, prob, settings, pre, xref, bnds, uref=None):
    """fp64 oracle (== the reference's fp64 build) on the same live-in: the intrinsic rounding spread."""
    st = {k: (v.astype(np.float64) if v.dtype == np.float32 else v.copy()) for k, v in pre.items()}
    # a yardstick, not a parity claim: the fp64 restatement is accepted for every dimension
    orc = O.Oracle(prob, np.float64, settings, allow_unpinned_dims=True)
    orc.set_uref(uref)
    orc.solve(st, *[np.asarray(b, np.float64) for b in bnds], np.asarray(xref, np.float64), nthreads=8)
    return st


def assert_bitwise(got, ref, what):
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} is not bitwise equal (max diff {np.max(np.abs(got[k].astype(np.float64) - ref[k]))})"
        if got[k].dtype.kind == "f":  # array_equal treats -0.0 == +0.0: the sign of a zero is part of "bitwise"
            assert np.array_equal(np.signbit(got[k]), np.signbit(ref[k])), f"{what}: {k} differs in the sign of a zero"
    return 0


def compare_states(got, ref, prob, what, ref64=None, exact=False, fixed=False, ct=1):
    if exact:
        return assert_bitwise(got, ref, what)
    same = (got["iter"] == ref["iter"]) & (got["status"] == ref["status"])
    nflip = int((~same).sum())
    if fixed or ref64 is None:  # fixed-iteration solves: the iteration count cannot legitimately change
        assert nflip == 0, f"{what}: iter/status differ for {nflip} instances"
        same64 = np.ones_like(same)
    else:
        same64 = (ref64["iter"] == ref["iter"]) & (ref64["status"] == ref["status"])
        f64 = float((~same64).mean())
        assert nflip / same.size <= max(1.5 * f64, 0.02) + 1.0 / same.size, \
            f"{what}: {nflip}/{same.size} iteration-count changes vs fp32 reference; the reference's own fp64 build changes {f64:.3f}"
        if nflip:
            spread = int(np.abs(ref64["iter"] - ref["iter"]).max())
            assert int(np.abs(got["iter"][~same] - ref["iter"][~same]).max()) <= spread + 2 * ct, what  # exits only happen every ct iterations
    if same.any():
        for k in STATE_ORDER:
            fl = _floor(k, prob, ref[k])
            e = rel_inf(got[k][same], ref[k][same], fl)
            bar = 2e-5 if k in PRIMAL_U else 5e-5  # g, q, p inherit the x-type error through x - vnew
            if ref64 is not None and same64.any():
                bar = max(bar, 4.0 * float(rel_inf(ref64[k][same64], ref[k][same64], fl).max()))
            assert e.max() <= bar, f"{what}: array {k} rel-inf error {e.max():.3e} > {bar:.3e} (instance {int(e.argmax())})"
        eu = rel_inf(got["u"][same], ref["u"][same], _floor("u", prob, ref["u"]))
        assert eu.max() <= 3e-4, f"{what}: u off by {eu.max():.3e}"
    return nflip


class DevBuf:
    """A device copy of a numpy array through the HIP runtime the library itself links (no torch in these tests)."""

    def __init__(self, a):
        import ctypes
        self._hip = ctypes.CDLL("libamdhip64.so")
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        assert self._hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(a.nbytes)) == 0
        assert self._hip.hipMemcpy(p, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes), 1) == 0
        self.ptr = p.value

    def free(self):
        import ctypes
        self._hip.hipFree(ctypes.c_void_p(self.ptr))


def make_solver(T, prob, B, settings, xref, variant="stream", bnds=None):
    """Create a solver forced onto one kernel variant; skips the test if that variant has no instantiation."""
    s = T.TinyBatchSolver(prob, B, settings=settings)
    try:
        s.select_kernel(VARIANTS[variant][0])
        s.set_row_kernel(VARIANTS[variant][2])
    except T.TinyBatchError as e:
        s.close()
        pytest.skip(f"variant {variant} unavailable for nx={prob['nx']} nu={prob['nu']} N={prob['N']}: {e}")
    s.set_bounds(*(bnds if bnds is not None else bounds_of(prob, np.float32)))
    if xref is not None:
        s.set_xref(xref)
    return s


@pytest.fixture(params=list(VARIANTS))
def variant(request):
    return request.param


F32_FIXTURES = ["quad_hover_f32_N30", "quad_track_f32_N30", "quad_batch_f32_N30", "quad_trackbatch_f32_N30",
                "cartpole_f32_N10", "random_f32_32_16_50", "dims_f32_8_3_7"]


@pytest.mark.parametrize("name", F32_FIXTURES)
def test_golden_vectors(tinympc, oracle_mod, variant, name):
    """live-in of every golden solve -> HIP tiny_batch_solve -> live-out, vs the compiled reference."""
    exact = VARIANTS[variant][1]
    meta, prob, solves, _ = load_fixture(name)
    bnds = bounds_of(prob, np.float32)
    for s in solves:
        B = s["pre"]["x"].shape[0]
        sol = make_solver(tinympc, prob, B, s["settings"], s["xref"], variant)
        sol.set_state(s["pre"])
        rc = sol.solve()
        got = sol.get_state()
        fixed = s["settings"]["abs_pri_tol"] == 0
        r64 = None if exact else yardstick(oracle_mod, prob, s["settings"], s["pre"], s["xref"], bnds)
        nf = compare_states(got, s["post"], prob, f"{name}[k={s['k']}] {variant}", ref64=r64, exact=exact, fixed=fixed)
        if nf == 0:
            assert rc == (1 if s["rc"] > 0 else 0)
        sol.close()


def plant_of(prob):
    """x1 = Adyn*x0 + Bdyn*u0 in the order of the examples' Eigen expression (quadrotor_hovering.cpp:110-111): the oracle's
    restatement, pinned against the compiled expression in tests/test_oracle.py."""
    from oracle import oracle as O
    orc = O.Oracle(prob, np.float32)
    return lambda x0, u0: orc.plant_step(np.atleast_2d(x0), np.atleast_2d(u0)).reshape(np.shape(x0))


def test_golden_warm_start_chain(tinympc, variant):
    """Closed loop driven by the HIP solver itself from the k=0 live-in: state persists on the device between
    solves (warm start), reset_dual_variables() between them — quadrotor_hovering.cpp:90-114."""
    exact = VARIANTS[variant][1]
    meta, prob, solves, z = load_fixture("quad_hover_f32_N30")
    sol = make_solver(tinympc, prob, 1, solves[0]["settings"], solves[0]["xref"], variant)
    sol.set_state(solves[0]["pre"])
    plant = plant_of(prob)
    x0 = solves[0]["pre"]["x"][:, 0].copy()
    iters, u0s = [], []
    for k in range(70):
        sol.set_x0(x0)
        sol.reset_dual_variables()
        sol.solve()
        u0 = sol.get_u()[:, 0]
        iters.append(int(sol.get_status()[0][0])); u0s.append(u0[0].copy())
        x0 = plant(x0, u0)  # the examples' plant step, as in tests/golden/make_golden.py
    ref_it = z["trace_iter"]
    if exact:  # the whole 70-step closed loop is reproduced bit for bit
        assert np.array_equal(np.array(iters), ref_it) and np.array_equal(np.array(u0s), z["trace_u0"])
    else:
        np.testing.assert_allclose(np.array(u0s[:3]), z["trace_u0"][:3], rtol=0, atol=1e-5)
        assert iters[0] == ref_it[0] == 100 and iters[69] == ref_it[69] == 2
        assert abs(sum(iters) - int(ref_it.sum())) <= 0.03 * ref_it.sum(), (sum(iters), int(ref_it.sum()))
    sol.close()


@pytest.mark.parametrize("B", [1, 3, 4, 5, 15, 16, 17, 100, 1000])
def test_ragged_batches_vs_oracle(tinympc, oracle_mod, variant, B):
    """Batch sizes around the 4- and 16-instance wave granules; cold start + one warm start; early exit and fixed."""
    O, pr = oracle_mod, tinympc.problems
    exact = VARIANTS[variant][1]
    prob = pr.quadrotor(20, 30)
    x0, xref = pr.hover_batch(B, 30, seed=100 + B)
    bnds = pr.bounds_arrays(prob)
    for settings, fixed in ((dict(O.DEFAULT_SETTINGS), False),
                            (dict(O.DEFAULT_SETTINGS, abs_pri_tol=0.0, abs_dua_tol=0.0, max_iter=10), True)):
        orc = O.Oracle(prob, np.float32, settings)
        sol = make_solver(tinympc, prob, B, settings, xref, variant, bnds)
        st = O.new_state(B, 12, 4, 30)
        st["x"][:, 0] = x0
        sol.set_x0(x0)
        for k in range(2):
            st["y"][:] = 0; st["g"][:] = 0
            sol.reset_dual_variables()
            pre = O.copy_state(st)
            orc.solve(st, *bnds, xref, nthreads=8)
            sol.solve()
            got = sol.get_state()
            r64 = None if exact else yardstick(O, prob, settings, pre, xref, bnds)
            compare_states(got, st, prob, f"B={B} k={k} fixed={fixed} {variant}", ref64=r64, exact=exact, fixed=fixed)
            if not exact:
                sol.set_state(st)  # re-synchronise so the next warm start compares like with like
        sol.close()


def test_settings_variants_vs_oracle(tinympc, oracle_mod, variant):
    """check_termination > 1 (stale residuals), bounds disabled, max_iter=1, infeasible bounds (min > max,
    as in examples/codegen_random.cpp:28-31), per-step bounds, per-instance bounds and per-instance Xref."""
    O, pr = oracle_mod, tinympc.problems
    exact = VARIANTS[variant][1]
    prob = pr.quadrotor(20, 30)
    B = 48
    rng = np.random.default_rng(5)
    x0, _ = pr.hover_batch(B, 30, seed=5, spread=0.5)
    xref = (rng.standard_normal((B, 30, 12)) * 0.3).astype(np.float32)
    xmn, xmx, umn, umx = pr.bounds_arrays(prob)
    step_scale_x = rng.uniform(0.5, 1.0, size=(30, 1)).astype(np.float32)
    step_scale_u = rng.uniform(0.5, 1.0, size=(29, 1)).astype(np.float32)
    variants = [
        (dict(check_termination=3, max_iter=50), (xmn, xmx, umn, umx)),
        (dict(check_termination=7, max_iter=20), (xmn, xmx, umn, umx)),
        (dict(en_state_bound=0, en_input_bound=0, max_iter=30), (xmn, xmx, umn, umx)),
        (dict(en_state_bound=0, max_iter=30), (xmn, xmx, umn, umx)),
        (dict(en_input_bound=0, max_iter=30), (xmn, xmx, umn, umx)),
        (dict(max_iter=1), (xmn, xmx, umn, umx)),
        (dict(max_iter=15, abs_pri_tol=0.0, abs_dua_tol=0.0), (xmx * 0.1, xmn * 0.1, umx, umn)),  # min > max
        (dict(max_iter=15, abs_pri_tol=0.0, abs_dua_tol=0.0),
         (xmn * step_scale_x, xmx * step_scale_x, umn * step_scale_u, umx * step_scale_u)),     # per-step, shared
        (dict(max_iter=15, abs_pri_tol=0.0, abs_dua_tol=0.0),
         tuple((a[None] * rng.uniform(0.5, 1.0, size=(B, 1, 1))).astype(np.float32) for a in (xmn, xmx, umn, umx))),
    ]
    for over, bnds in variants:
        settings = dict(O.DEFAULT_SETTINGS, **over)
        orc = O.Oracle(prob, np.float32, settings)
        sol = make_solver(tinympc, prob, B, settings, xref, variant, bnds)
        if bnds[0].ndim == 3 and variant != "stream":
            # per-instance bounds: the unrolled and the rolled-loop register-resident kernels read them per lane-step from the
            # [B][N][16] table; a handle forced onto another family runs on the streaming row kernel (same arithmetic: still
            # bitwise when exact)
            # (round 4: the sixteen-instances-per-wave kernel serves them itself, rows fetched by LDS-DMA: the `pi` instantiations)
            fam = VARIANTS[variant][2]
            want = "rowlane" if fam in (0, 1) else "rowloop" if fam == 2 else "tile16" if fam == 5 else "rowstream"
            assert sol.kernel_name().startswith(want), (variant, sol.kernel_name())
            assert fam != 5 or sol.kernel_name().endswith(",pi>"), sol.kernel_name()
        st = O.new_state(B, 12, 4, 30)
        st["x"][:, 0] = x0
        st["residuals"][:] = rng.uniform(0, 1, size=(B, 4)).astype(np.float32)  # residual fields are live-in
        for k in ("d", "v", "z", "y", "g"):
            st[k][:] = (rng.standard_normal(st[k].shape) * 0.05).astype(np.float32)
        sol.set_state(st)
        pre = O.copy_state(st)
        orc.solve(st, *bnds, xref, nthreads=8)
        sol.solve()
        fixed = settings["abs_pri_tol"] == 0 or settings["max_iter"] == 1
        r64 = None if exact else yardstick(O, prob, settings, pre, xref, bnds)
        compare_states(sol.get_state(), st, prob, f"variant {over} {variant}", ref64=r64, exact=exact, fixed=fixed,
                       ct=settings["check_termination"])
        sol.close()


def test_max_iter_zero(tinympc, variant):
    """admm.cpp:114-117,151: status=11, iter=1, rc=1 and nothing else is touched."""
    meta, prob, solves, _ = load_fixture("quad_hover_f32_N30")
    s = solves[2]
    sol = make_solver(tinympc, prob, 1, dict(s["settings"], max_iter=0), s["xref"], variant)
    sol.set_state(s["pre"])
    sol.reset_dual_variables()  # pre already has y = g = 0
    assert sol.solve() == 1
    got = sol.get_state()
    assert got["status"][0] == 11 and got["iter"][0] == 1
    for k in STATE_ORDER + ("residuals",):
        assert np.array_equal(got[k], s["pre"][k]), k
    sol.close()


def test_reset_dual_variables_is_observable(tinympc, variant):
    """reset_dual_variables() is folded into the next solve, but a read in between must already see zeros."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    sol = make_solver(tinympc, prob, 20, None, None, variant)
    rng = np.random.default_rng(0)
    y = rng.standard_normal((20, 29, 4)).astype(np.float32)
    g = rng.standard_normal((20, 30, 12)).astype(np.float32)
    sol.set_array("y", y); sol.set_array("g", g)
    assert np.array_equal(sol.get_array("y"), y) and np.array_equal(sol.get_array("g"), g)
    sol.reset_dual_variables()
    assert not sol.get_array("y").any() and not sol.get_array("g").any()
    sol.reset_workspace()
    for name in tinympc.ARRAY_IDS:
        assert not sol.get_array(name).any(), name
    sol.close()


def test_layout_round_trip_all_arrays(tinympc, variant):
    """set_array/get_array round-trip every work array bit-exactly (host (B,N,nx) <-> device layout)."""
    pr = tinympc.problems
    for prob, B in ((pr.quadrotor(20, 30), 37), (pr.cartpole(10), 5), (pr.random_system(8, 3, 7, seed=1), 33)):
        sol = tinympc.TinyBatchSolver(prob, B)
        try:
            sol.select_kernel(VARIANTS[variant][0])
        except tinympc.TinyBatchError:
            sol.close()
            continue
        rng = np.random.default_rng(B)
        arrs = {}
        for name in tinympc.ARRAY_IDS:
            arrs[name] = rng.standard_normal(sol._xshape(name)).astype(np.float32)
            sol.set_array(name, arrs[name])
        for name in tinympc.ARRAY_IDS:
            assert np.array_equal(sol.get_array(name), arrs[name]), name
        sol.close()


def test_kernel_variants_agree_after_switch(tinympc):
    """Switching the kernel variant on a live handle converts the device layout and keeps every array."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    sol = tinympc.TinyBatchSolver(prob, 21)
    rng = np.random.default_rng(1)
    arrs = {n: rng.standard_normal(sol._xshape(n)).astype(np.float32) for n in tinympc.ARRAY_IDS}
    for n, a in arrs.items():
        sol.set_array(n, a)
    for vid in [v[0] for v in VARIANTS.values()] + [0]:
        try:
            sol.select_kernel(vid)
        except tinympc.TinyBatchError:
            continue
        for n, a in arrs.items():
            assert np.array_equal(sol.get_array(n), a), (vid, n)
    sol.close()


def test_window_reference_equals_expanded_reference(tinympc, variant):
    """set_xref_window (device-side gather from the trajectory table, quadrotor_tracking.cpp:84-85,101) gives
    bit-identical results to uploading the expanded per-instance windows."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 500
    x0, table, start = pr.tracking_batch(B, 30, seed=3)
    outs = []
    for mode in ("window", "expanded"):
        sol = make_solver(tinympc, prob, B, None, None, variant, pr.bounds_arrays(prob))
        if mode == "window":
            sol.set_xref_window(table, start)
        else:
            sol.set_xref(pr.expand_windows(table, start, 30))
        sol.set_x0(x0)
        sol.solve()
        outs.append(sol.get_state())
        sol.close()
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(outs[0][k], outs[1][k]), k


def test_device_closed_loop_matches_host_loop(tinympc, variant):
    """tiny_batch_mpc_step_async (x0 update + dual reset + solve + plant step on the device, window sliding)
    against the same loop driven from the host through set_x0/reset/solve/get_u."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 64
    x0, table, start = pr.tracking_batch(B, 30, seed=9)
    bnds = pr.bounds_arrays(prob)
    plant = plant_of(prob)
    dev = make_solver(tinympc, prob, B, None, None, variant, bnds)
    host = make_solver(tinympc, prob, B, None, None, variant, bnds)
    for s in (dev, host):
        s.set_xref_window(table, start)
        s.set_x0(x0)
    xh = x0.copy()
    for k in range(5):
        dev.mpc_step_async(1)
        host.set_xref_window(table, start + k)
        host.set_x0(xh)
        host.reset_dual_variables()
        host.solve()
        assert np.array_equal(host.get_status()[0], dev.get_status()[0])
        assert np.array_equal(host.get_u(), dev.get_u())
        xd = dev.get_x0()
        uh = host.get_u()[:, 0]
        # the plant step's order is the reference's in both arithmetic modes: bitwise the oracle's, signs of zeros included
        xw = plant(xh, uh)
        assert np.array_equal(xd, xw) and np.array_equal(np.signbit(xd), np.signbit(xw)), k
        xh = xd  # follow the device trajectory so that later steps compare like with like
    dev.close(); host.close()


def test_errors_are_reported_not_swallowed(tinympc):
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    with pytest.raises(tinympc.TinyBatchError):
        tinympc.TinyBatchSolver(dict(prob, nx=72, Kinf=np.zeros((4, 72)), Pinf=np.zeros((72, 72)), AmBKt=np.zeros((72, 72)),
                                     Adyn=np.zeros((72, 72)), Bdyn=np.zeros((72, 4)), Q=np.zeros(72)), 4)  # nx > 64: no kernel
    sol = tinympc.TinyBatchSolver(prob, 4)
    with pytest.raises(tinympc.TinyBatchError):
        sol.set_xref_window(np.zeros((20, 12), np.float32), np.zeros(4, np.int32))  # table shorter than N
    with pytest.raises(tinympc.TinyBatchError):
        sol.set_settings(1e-3, 1e-3, 10, 0, 1, 1)  # check_termination = 0 would divide by zero in the reference
    sol.set_xmin(np.zeros((4, 30, 12), np.float32))  # per-instance min with shared max
    with pytest.raises(tinympc.TinyBatchError):
        sol.solve()
    sol.close()


# ---------------------------------------------------------------------------------------------------
# BASELINE.json full sizes: size-independent properties + sampled oracle comparison
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,B", [("hover", 4096), ("tracking", 65536)])
def test_full_size_properties(tinympc, oracle_mod, variant, config, B):
    O, pr = oracle_mod, tinympc.problems
    exact = VARIANTS[variant][1]
    prob = pr.quadrotor(20, 30)
    bnds = pr.bounds_arrays(prob)
    sol = make_solver(tinympc, prob, B, None, None, variant, bnds)
    half = B // 2
    if config == "hover":
        x0, xref = pr.hover_batch(B, 30)
        x0[half:] = x0[:half]
        sol.set_xref(xref)
        xref_of = lambda idx: xref
    else:
        x0, table, start = pr.tracking_batch(B, 30)
        x0[half:] = x0[:half]
        start[half:] = start[:half]
        sol.set_xref_window(table, start)
        xref_of = lambda idx: pr.expand_windows(table, start[idx], 30)
    sol.set_x0(x0)
    rc = sol.solve()
    a = sol.get_state()
    # (1) duplicates (second half of the batch repeats the first) agree bit for bit, wherever they sit
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(a[k][:half], a[k][half:]), k
    # (2) determinism: cold restart gives the identical answer
    sol.reset_workspace(); sol.set_x0(x0); sol.solve()
    b = sol.get_state()
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(a[k], b[k]), k
    # (2b) the dispatch order is invisible in the results: longest first by the predicted iteration count (a no-op below
    # 4096 groups and for the kernels that stream their state), then the caller's own order, here the reverse
    sol.set_dispatch(1)
    sol.reset_workspace(); sol.set_x0(x0); sol.solve()
    b = sol.get_state()
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(a[k], b[k]), ("dispatch 1", k)
    order = DevBuf(np.arange((B + 3) // 4, dtype=np.int32)[::-1].copy())
    sol.set_dispatch_order_device(order.ptr)
    sol.reset_workspace(); sol.set_x0(x0); sol.solve()
    b = sol.get_state()
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(a[k], b[k]), ("reverse order", k)
    sol.set_dispatch_order_device(None); sol.set_dispatch(0)
    sol.synchronize(); order.free()
    # (3) invariants of the algorithm
    s = sol.settings
    assert set(np.unique(a["status"])) <= {1, 11} and a["iter"].min() >= 1 and a["iter"].max() <= s["max_iter"]
    solved = a["status"] == 1
    assert rc == (0 if solved.all() else 1)
    assert np.all(a["residuals"][solved][:, :2] < s["abs_pri_tol"]) and np.all(a["residuals"][solved][:, 2:] < s["abs_dua_tol"])
    assert np.all(a["iter"][~solved] == s["max_iter"])
    assert a["znew"].max() <= prob["u_max"] and a["znew"].min() >= prob["u_min"]
    assert a["vnew"].max() <= prob["x_max"] and a["vnew"].min() >= prob["x_min"]
    assert np.array_equal(a["x"][:, 0], x0)
    # unsolved instances ran the v/z copy on their last iteration (admm.cpp:141-142)
    assert np.array_equal(a["v"][~solved], a["vnew"][~solved]) and np.array_equal(a["z"][~solved], a["znew"][~solved])
    # dynamics consistency of the rollout: x_{i+1} = A x_i + B u_i
    A, Bm = prob["Adyn"], prob["Bdyn"]
    idx = np.arange(0, B, max(1, B // 512))
    xs, us = a["x"][idx].astype(np.float64), a["u"][idx].astype(np.float64)
    assert np.max(np.abs(xs[:, :-1] @ A.T + us @ Bm.T - xs[:, 1:])) < 5e-5
    # (4) sampled comparison with the oracle
    st = O.new_state(idx.size, 12, 4, 30)
    st["x"][:, 0] = x0[idx]
    pre = O.copy_state(st)
    O.Oracle(prob, np.float32, s).solve(st, *bnds, xref_of(idx), nthreads=8)
    got = {k: a[k][idx] for k in STATE_ORDER + SCALARS}
    r64 = None if exact else yardstick(O, prob, s, pre, xref_of(idx), bnds)
    compare_states(got, st, prob, f"{config} B={B} sample {variant}", ref64=r64, exact=exact)
    sol.close()


# ---------------------------------------------------------------------------------------------------
# the six step functions of admm.hpp:12-18 as separate batched calls
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["quad30", "quad_window", "cartpole", "odd_8_3_7", "quad_N17"])
@pytest.mark.parametrize("exact", [True, False])
def test_step_functions_individually(tinympc, oracle_mod, case, exact):
    """Each exported step function, applied to a random workspace, against the oracle's restatement of the same
    reference function: bitwise in exact arithmetic, rounding-level in fast arithmetic.  Then one ADMM iteration
    composed from the six calls in tiny_solve's order (admm.cpp:117-144)."""
    O, pr = oracle_mod, tinympc.problems
    prob = {"quad30": lambda: pr.quadrotor(20, 30), "quad_window": lambda: pr.quadrotor(20, 30),
            "cartpole": lambda: pr.cartpole(10), "odd_8_3_7": lambda: pr.random_system(8, 3, 7, seed=99),
            "quad_N17": lambda: pr.quadrotor(20, 17)}[case]()   # N=17 has no fused rowlane instantiation
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    B = 23
    rng = np.random.default_rng(7)
    bnds = tuple(a * s for a, s in zip(pr.bounds_arrays(prob), (0.2, 0.2, 1.0, 1.0)))  # tight enough to clip
    st = O.new_state(B, nx, nu, N)
    for k in STATE_ORDER:
        st[k][:] = (rng.standard_normal(st[k].shape) * 0.3).astype(np.float32)
    st["iter"][:] = rng.integers(1, 9, size=B)
    st["status"][:] = 11
    st["residuals"][:] = rng.uniform(0, 1, size=(B, 4)).astype(np.float32)
    settings = dict(O.DEFAULT_SETTINGS, check_termination=2, abs_pri_tol=0.5, abs_dua_tol=5.0)
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.select_kernel(0 if exact else (3 if (nx, nu, N) != (12, 4, 17) else 0))
    if not exact and (nx, nu, N) == (12, 4, 17):
        sol.close(); pytest.skip("fast arithmetic is selected through the rowlane-fast variant, which N=17 lacks")
    sol.set_bounds(*bnds)
    if case == "quad_window":
        _, table, start = pr.tracking_batch(B, N, seed=2)
        sol.set_xref_window(table, start)
        xref = pr.expand_windows(table, start, N)
    else:
        xref = (rng.standard_normal((B, N, nx)) * 0.3).astype(np.float32)
        sol.set_xref(xref)
    orc = O.Oracle(prob, np.float32, settings)

    def check(what):
        got = sol.get_state()
        for k in STATE_ORDER + ("residuals",):
            if exact:
                assert np.array_equal(got[k], st[k]), f"{case} {what}: {k} not bitwise equal"
            else:
                scale = max(1.0, float(np.abs(st[k]).max()))
                assert np.max(np.abs(got[k].astype(np.float64) - st[k])) <= 2e-5 * scale, f"{case} {what}: {k}"

    for fn in O.Oracle.STEP_FUNCTIONS:
        sol.set_state(st)
        ref_rv = orc.step(fn, st, *bnds, xref)
        rv = getattr(sol, fn)()
        if fn == "termination_condition":
            assert np.array_equal(rv, ref_rv) or not exact
        check(fn)
    # one iteration assembled from the six calls
    sol.set_state(st)
    for fn in ("forward_pass", "update_slack", "update_dual", "update_linear_cost"):
        orc.step(fn, st, *bnds, xref); getattr(sol, fn)()
    orc.step("termination_condition", st, *bnds, xref); sol.termination_condition()
    st["v"][:] = st["vnew"]; st["z"][:] = st["znew"]
    sol.set_array("v", sol.get_array("vnew")); sol.set_array("z", sol.get_array("znew"))
    orc.step("backward_pass_grad", st, *bnds, xref); sol.backward_pass_grad()
    check("composed iteration")
    sol.close()


@pytest.mark.parametrize("case", [("quad", 5), ("quad", 17), ("quad", 20), ("quad", 25), ("quad", 32), ("quad", 33), ("quad", 45), ("quad", 40), ("quad", 50), ("quad", 64), ("quad", 65),
                                  ("cartpole", 25), ("cartpole", 40), ("odd", 12), ("odd", 2),
                                  ("r8_4", 9), ("r8_4", 40), ("r12_2", 11), ("r4_2", 8), ("r4_4", 6)])  # classes pinned in test_oracle.py
@pytest.mark.parametrize("variant_name", ["row_exact", "row_fast"])
def test_any_horizon_row_kernel(tinympc, oracle_mod, case, variant_name):
    """Horizons other than the examples' 10 and 30: a few have an unrolled instantiation (rowlane), otherwise N <= 64 runs on
    the rolled-loop register-resident kernels (rowloop) and longer horizons on the any-N row kernel with the state in HBM
    (rowstream); all stay bitwise in exact arithmetic.
    Cold start, then a warm start with reset duals; early exit."""
    O, pr = oracle_mod, tinympc.problems
    exact = VARIANTS[variant_name][1]
    kind, N = case
    if kind.startswith("r") and "_" in kind:
        nxk, nuk = (int(v) for v in kind[1:].split("_"))
        prob = pr.random_system(nxk, nuk, N, seed=nxk * 100 + nuk)
    else:
        prob = {"quad": lambda: pr.quadrotor(20, N), "cartpole": lambda: pr.cartpole(N),
                "odd": lambda: pr.random_system(8, 3, N, seed=99)}[kind]()
    nx, nu = prob["nx"], prob["nu"]
    B = 700 if N in (40, 50) else 70   # the fma bar is a rate (iteration-count changes against the fp64-vs-fp32 rate): long horizons need the sample
    rng = np.random.default_rng(N)
    x0 = (rng.uniform(-0.3, 0.3, size=(B, nx))).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.1).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=60)
    sol = make_solver(tinympc, prob, B, settings, xref, variant_name, bnds)
    unrolled = (kind, N) in (("quad", 20), ("quad", 25), ("quad", 40), ("quad", 50))  # TINY_FOR_EACH_ROWLANE
    assert sol.kernel_name().startswith("rowlane" if unrolled else "rowloop" if N <= 64 else "rowstream"), sol.kernel_name()
    orc = O.Oracle(prob, np.float32, settings)
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = x0
    sol.set_x0(x0)
    for k in range(2):
        st["y"][:] = 0; st["g"][:] = 0
        sol.reset_dual_variables()
        pre = O.copy_state(st)
        orc.solve(st, *bnds, xref, nthreads=8)
        sol.solve()
        r64 = None if exact else yardstick(O, prob, settings, pre, xref, bnds)
        compare_states(sol.get_state(), st, prob, f"{case} k={k} {variant_name}", ref64=r64, exact=exact)
        if not exact:
            sol.set_state(st)
    sol.close()


def test_mixed_problem_classes_on_two_streams(tinympc, oracle_mod):
    """BASELINE.json config 5's mixed-size batch: a cartpole class and a quadrotor class are two handles; enqueued on
    two HIP streams they run concurrently and each stays bitwise equal to the oracle."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")  # the runtime the library itself links (already loaded)
    O, pr = oracle_mod, tinympc.problems
    cases = []
    for prob, B in ((pr.cartpole(10), 3000), (pr.quadrotor(20, 30), 2000)):
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        rng = np.random.default_rng(B)
        x0 = rng.uniform(-0.2, 0.2, size=(B, nx)).astype(np.float32)
        xref = np.zeros((N, nx), np.float32)
        bnds = pr.bounds_arrays(prob)
        sol = tinympc.TinyBatchSolver(prob, B, settings=dict(max_iter=150))
        stream = ctypes.c_void_p()
        assert hip.hipStreamCreate(ctypes.byref(stream)) == 0
        sol.set_stream(stream.value)
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
        O.Oracle(prob, np.float32, dict(O.DEFAULT_SETTINGS, max_iter=150)).solve(st, *bnds, xref, nthreads=8)
        cases.append((sol, st, stream))
    for sol, _, _ in cases:
        sol.solve_async()          # both launches are in flight before either is waited for
    for sol, st, _ in cases:
        sol.wait()
        assert_bitwise(sol.get_state(), st, sol.kernel_name())
        sol.close()
    for _, _, stream in cases:
        hip.hipStreamDestroy(stream)


def test_reference_wrapper_names_drive_the_hovering_loop():
    """An FFI script written for the reference's generated wrapper library (set_x0 / reset_dual_variables /
    call_tiny_solve / get_u, tiny_wrapper.hpp:14-23) runs unchanged against libtinympc_wrapper.so: the 70-step hovering
    loop of examples/quadrotor_hovering.cpp reproduces the compiled reference's controls and iteration counts bit for bit."""
    import ctypes as C
    from pathlib import Path
    meta, prob, solves, z = load_fixture("quad_hover_f32_N30")
    lib = C.CDLL(str(Path(__file__).resolve().parents[1] / "accelerated-tinympc_amd" / "lib" / "libtinympc_wrapper.so"))
    F = C.POINTER(C.c_float)
    cm = lambda m: np.ascontiguousarray(np.asarray(m, np.float32).T).ravel()
    fp = lambda a: a.ctypes.data_as(F)
    mats = [cm(prob[k]) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")] + [np.asarray(prob["Q"], np.float32)]
    lib.tiny_wrapper_setup.argtypes = [C.c_int] * 3 + [C.c_float] + [F] * 7 + [C.c_float] * 2 + [C.c_int] * 5
    assert lib.tiny_wrapper_setup(12, 4, 30, prob["rho"], *[fp(m) for m in mats], 1e-3, 1e-3, 100, 1, 1, 1, 0) == 0
    for fn in ("set_x0", "set_xref", "set_umin", "set_umax", "set_xmin", "set_xmax", "get_x", "get_u"):
        getattr(lib, fn).argtypes, getattr(lib, fn).restype = [F, C.c_int], None
    xmn, xmx, umn, umx = bounds_of(prob, np.float32)
    lib.set_xmin(fp(xmn), 0); lib.set_xmax(fp(xmx), 0); lib.set_umin(fp(umn), 0); lib.set_umax(fp(umx), 0)
    xref = np.ascontiguousarray(solves[0]["xref"], np.float32)
    lib.set_xref(fp(xref), 0)
    plant = plant_of(prob)
    x0 = solves[0]["pre"]["x"][0, 0].copy()
    u = np.zeros((29, 4), np.float32)
    it, stt = C.c_int(), C.c_int()
    iters, u0s = [], []
    for k in range(70):
        lib.set_x0(fp(x0), 0)
        lib.reset_dual_variables(0)
        lib.call_tiny_solve(0)
        lib.get_u(fp(u), 0)
        assert lib.tiny_wrapper_last_status(C.byref(it), C.byref(stt)) == 0
        iters.append(it.value); u0s.append(u[0].copy())
        x0 = plant(x0, u[0])
    assert np.array_equal(np.array(iters), z["trace_iter"]) and np.array_equal(np.array(u0s), z["trace_u0"])
    lib.tiny_wrapper_teardown()


@pytest.mark.parametrize("double", [False, True])
def test_cpp_hovering_example_runs_against_the_native_names(tinympc, tmp_path, double):
    """examples/quadrotor_hovering_native.cpp — the reference's hovering example written against include/tinympc_admm.h — built
    with g++ for float (libtinympc_wrapper.so, N = 30) and, as the reference is checked in, for double (libtinympc_wrapper64.so,
    N = 10): 70 closed-loop steps through tiny_solve(&solver), the tracking error shrinks to the hover point and the last solve
    converges in the iteration count of the compiled reference's own run."""
    import shutil
    import subprocess
    from pathlib import Path
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    root = Path(__file__).resolve().parents[1]
    lib_dir = root / "accelerated-tinympc_amd" / "lib"
    exe = tmp_path / ("hover64" if double else "hover32")
    cmd = ["g++", "-std=c++17", "-O1", f"-I{root / 'include'}", str(root / "examples" / "quadrotor_hovering_native.cpp"), f"-L{lib_dir}",
           "-ltinympc_wrapper64" if double else "-ltinympc_wrapper", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)]
    if double:
        cmd.insert(1, "-DTINYMPC_TINYTYPE_DOUBLE")
    subprocess.run(cmd, check=True)
    r = subprocess.run([str(exe), str(root / "accelerated-tinympc_amd" / "data" / "quadrotor_20hz.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    errs = [float(l.split(":")[1]) for l in lines if l.startswith("tracking error")]
    assert len(errs) == 70 and errs[0] > 2.0 and errs[-1] < 0.02 and errs[-1] < errs[35] < errs[0]
    _, _, _, z = load_fixture("quad_hover_f64_N10" if double else "quad_hover_f32_N30")
    assert lines[-1] == f"final: iter={int(z['trace_iter'][69])} status=1", lines[-1]


def test_cpp_batched_tracking_example_runs(tinympc, tmp_path):
    """examples/quadrotor_tracking_batched.cpp (nothing but include/tinympc_batch.h) built with g++ and run: 512 quadrotors track
    the trajectory in closed loop on the exact register-resident kernel, the tracking error falls."""
    import re
    import shutil
    import subprocess
    from pathlib import Path
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    root = Path(__file__).resolve().parents[1]
    lib_dir = root / "accelerated-tinympc_amd" / "lib"
    exe = tmp_path / "track"
    subprocess.run(["g++", "-std=c++17", "-O1", f"-I{root / 'include'}", str(root / "examples" / "quadrotor_tracking_batched.cpp"), f"-L{lib_dir}",
                    "-ltinympc_hip", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(root / "accelerated-tinympc_amd" / "data" / "quadrotor_20hz.bin"), "512", "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "kernel: rowlane<12,4,30,exact>, 512 instances" in r.stdout, r.stdout[:300]
    errs = [float(m) for m in re.findall(r"mean tracking error ([0-9.eE+-]+)", r.stdout)]
    assert len(errs) >= 5 and all(np.isfinite(errs)) and errs[-1] <= errs[0]


def test_native_names_tiny_solve_hovering_loop(tinympc):
    """examples/quadrotor_hovering.cpp:90-114 written against include/tinympc_admm.h (TinySolver{settings,cache,work},
    tiny_solve): the caller owns the workspace arrays, warm start travels through them like in the reference.  Controls,
    iteration counts and the full workspace of the recorded solves equal the compiled reference's bit for bit."""
    from accelerated_tinympc_amd import native
    meta, prob, solves, z = load_fixture("quad_hover_f32_N30")
    ns = native.NativeSolver(prob, solves[0]["settings"])
    for k, arr in zip(("x_min", "x_max", "u_min", "u_max"), bounds_of(prob, np.float32)):
        ns.a[k][:] = arr
    ns.a["Xref"][:] = solves[0]["xref"]
    plant = plant_of(prob)
    x0 = solves[0]["pre"]["x"][0, 0].copy()
    recorded = {s["k"]: s for s in solves}
    iters, u0s = [], []
    for k in range(70):
        ns.a["x"][0] = x0                       # hovering.cpp:95
        ns.a["y"][:] = 0; ns.a["g"][:] = 0      # :100-101
        rc = ns.tiny_solve()                    # :104
        iters.append(ns.work.iter); u0s.append(ns.a["u"][0].copy())
        if k in recorded:
            post = recorded[k]["post"]
            assert rc == recorded[k]["rc"]
            for name in STATE_ORDER:
                assert np.array_equal(ns.a[name], post[name][0]), f"step {k}: {name}"
            assert np.array_equal(ns.residuals, post["residuals"][0]) and ns.work.status == post["status"][0]
        x0 = plant(x0, ns.a["u"][0])  # :110-111
    assert np.array_equal(np.array(iters), z["trace_iter"]) and np.array_equal(np.array(u0s), z["trace_u0"])


@pytest.mark.parametrize("case", ["quad30", "cartpole"])
def test_native_names_step_functions(tinympc, oracle_mod, case):
    """forward_pass ... termination_condition under the reference's own names over a caller-owned TinySolver: each call
    leaves the structs exactly as the oracle's restatement of the same reference function does."""
    from accelerated_tinympc_amd import native
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 30) if case == "quad30" else pr.cartpole(10)
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    rng = np.random.default_rng(11)
    bnds = tuple(a * s for a, s in zip(pr.bounds_arrays(prob), (0.2, 0.2, 1.0, 1.0)))
    settings = dict(O.DEFAULT_SETTINGS, check_termination=2, abs_pri_tol=0.5, abs_dua_tol=5.0)
    st = O.new_state(1, nx, nu, N)
    for k in STATE_ORDER:
        st[k][:] = (rng.standard_normal(st[k].shape) * 0.3).astype(np.float32)
    st["iter"][:] = 4; st["status"][:] = 11
    st["residuals"][:] = rng.uniform(0, 1, size=(1, 4)).astype(np.float32)
    xref = (rng.standard_normal((1, N, nx)) * 0.3).astype(np.float32)
    orc = O.Oracle(prob, np.float32, settings)
    ns = native.NativeSolver(prob, settings)
    for k, arr in zip(("x_min", "x_max", "u_min", "u_max"), bnds):
        ns.a[k][:] = arr
    ns.a["Xref"][:] = xref[0]

    def load(state):
        for k in STATE_ORDER:
            ns.a[k][:] = state[k][0]
        w = ns.work
        (w.primal_residual_state, w.primal_residual_input, w.dual_residual_state, w.dual_residual_input) = map(float, state["residuals"][0])
        w.iter, w.status = int(state["iter"][0]), int(state["status"][0])

    for fn in O.Oracle.STEP_FUNCTIONS:
        load(st)
        ref_rv = orc.step(fn, st, *bnds, xref)
        rv = ns.call(fn)
        if fn == "termination_condition":
            assert bool(rv) == bool(ref_rv[0])
        for k in STATE_ORDER:
            assert np.array_equal(ns.a[k], st[k][0]), f"{fn}: {k}"
        assert np.array_equal(ns.residuals, st["residuals"][0]), fn
        assert ns.work.iter == st["iter"][0] and ns.work.status == st["status"][0], fn
    # tiny_solve from the same random warm state, with max_iter small enough to exhaust and large enough to converge
    for max_iter in (3, 200):
        settings2 = dict(settings, max_iter=max_iter, check_termination=1, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
        ns.settings.max_iter, ns.settings.check_termination = max_iter, 1
        ns.settings.abs_pri_tol = ns.settings.abs_dua_tol = 1e-3
        st2 = O.copy_state(st)
        load(st2)
        rcs = O.Oracle(prob, np.float32, settings2).solve(st2, *bnds, xref)
        rc = ns.tiny_solve()
        assert rc == (1 if st2["status"][0] == 11 else 0)
        for k in STATE_ORDER:
            assert np.array_equal(ns.a[k], st2[k][0]), f"tiny_solve max_iter={max_iter}: {k}"
        assert ns.work.iter == st2["iter"][0] and ns.work.status == st2["status"][0]


# ---------------------------------------------------------------------------------------------------------------------
# fp16 storage with fp32 arithmetic (BASELINE.json configs[4]; tiny_batch_set_storage(16)).
# Semantics: every per-instance horizon array is IEEE binary16 in HBM; each assignment to a work array rounds to nearest
# even; products, sums and the four residual reductions are fp32.  The oracle's _h16 instantiation restates exactly that
# (oracle/tinympc_oracle_impl.h: ST()), so the bar for EXACT arithmetic is unchanged: BITWISE equality with the oracle.
# FAST arithmetic (fma) may differ from it in the last fp16 bit of a stored value, which 29 rounded roll-out steps and the
# early exit amplify.  Its yardstick is the storage mode's own quantisation error, measured in the test: the fp32 oracle
# run from the same (binary16-representable) live-in, used with the multipliers of the fp32 fast bar above.  Bar: the
# fraction of instances whose iteration count differs from the _h16 oracle's <= max(1.5 x the fraction that differs
# between fp16 storage and fp32, 2 %); the others agree with it within max(4 binary16 ulps of the array's magnitude
# (2^-10 = 9.8e-4 each, the "~1e-3" SURVEY.md expects), 4 x the fp16-storage-vs-fp32 spread of the same array).
# The iteration-count drift against fp32 storage is reported by tools/bench_configs.py, not bounded here.
# ---------------------------------------------------------------------------------------------------------------------
H16_CASES = {"quad30": ("quad", 30), "quad17": ("quad", 17), "quad40": ("quad", 70), "cartpole10": ("cartpole", 10),
             "cartpole25": ("cartpole", 25)}  # rowlane, rowloop, rowstream, rowlane, rowloop


@pytest.mark.parametrize("variant_name", ["row_exact", "row_fast"])
@pytest.mark.parametrize("case", list(H16_CASES))
def test_fp16_storage_vs_oracle(tinympc, oracle_mod, case, variant_name):
    O, pr = oracle_mod, tinympc.problems
    exact = VARIANTS[variant_name][1]
    kind, N = H16_CASES[case]
    prob = pr.quadrotor(20, N) if kind == "quad" else pr.cartpole(N)
    nx, nu = prob["nx"], prob["nu"]
    B = 203
    rng = np.random.default_rng(N + nx)
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.1).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=80)
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.select_kernel(VARIANTS[variant_name][0])
    sol.set_storage(16, 16)
    assert sol.kernel_name().endswith(",h16>"), sol.kernel_name()
    sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
    orc = O.Oracle(prob, "h16", settings)
    bnds_h, xref_h = tuple(O.round_h16(b) for b in bnds), O.round_h16(xref)
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = O.round_h16(x0)
    for k in range(3):  # cold start, then two warm starts with reset duals
        st["y"][:] = 0; st["g"][:] = 0
        sol.reset_dual_variables()
        st32 = O.copy_state(st)
        orc.solve(st, *bnds_h, xref_h, nthreads=8)
        sol.solve()
        got = sol.get_state()
        for name in STATE_ORDER:
            assert np.array_equal(got[name], O.round_h16(got[name])), f"{name} is not binary16-representable"
        if exact:
            assert_bitwise(got, st, f"h16 {case} k={k}")
        else:
            O.Oracle(prob, np.float32, settings).solve(st32, *bnds_h, xref_h, nthreads=8)  # the quantisation yardstick
            same32 = st32["iter"] == st["iter"]
            same = (got["iter"] == st["iter"]) & (got["status"] == st["status"])
            f32flips = float((~same32).mean())
            assert (~same).mean() <= max(1.5 * f32flips, 0.02) + 1.0 / B, \
                f"h16 fast {case} k={k}: {(~same).mean():.2f} change the iteration count; fp16 storage itself changes {f32flips:.2f} vs fp32"
            for name in STATE_ORDER:
                scale = max(float(np.abs(st[name]).max()), 1e-2)
                err = np.abs(got[name][same].astype(np.float64) - st[name][same]).max() / scale
                sel = same32 if same32.any() else slice(None)
                spread = np.abs(st32[name][sel].astype(np.float64) - st[name][sel]).max() / scale
                assert err <= max(4 * 2.0 ** -10, 4 * spread), \
                    f"h16 fast {case} k={k}: {name} off by {err:.2e} of its magnitude (storage spread {spread:.2e})"
            sol.set_state(st)
    # what the caller stores is rounded on the way in, and a state written back reads back identically
    sol.set_array("d", st["d"] + np.float32(1e-4))
    assert np.array_equal(sol.get_array("d"), O.round_h16(st["d"] + np.float32(1e-4)))
    with pytest.raises(tinympc.TinyBatchError):
        sol.select_kernel(1)  # the streaming kernel has no fp16 storage
    sol.set_storage(32)       # back to fp32: workspace restarts from zero
    assert not np.any(sol.get_array("d")) and not sol.kernel_name().endswith("h16>")
    sol.close()


@pytest.mark.parametrize("variant_name", ["row_exact", "row_fast"])
@pytest.mark.parametrize("case", ["quad30", "cartpole10"])
def test_fp16_storage_with_fp32_duals_vs_oracle(tinympc, oracle_mod, case, variant_name):
    """tiny_batch_set_storage_ex(16, 32): ten work arrays, Xref and bounds in binary16, the duals y, g in fp32.  The
    oracle's _h16d instantiation restates it (STD() = identity on the two assignments of admm.cpp:69-70); exact arithmetic
    equals it bit for bit, fast arithmetic is held to the bar of the all-fp16 mode above (duals scaled by their primal array)."""
    O, pr = oracle_mod, tinympc.problems
    exact = VARIANTS[variant_name][1]
    kind, N = H16_CASES[case]
    prob = pr.quadrotor(20, N) if kind == "quad" else pr.cartpole(N)
    nx, nu = prob["nx"], prob["nu"]
    B = 203
    rng = np.random.default_rng(N + nx + 1)
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.1).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=80)
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.select_kernel(VARIANTS[variant_name][0])
    sol.set_storage(16, 32)
    assert sol.kernel_name().endswith(",h16d>"), sol.kernel_name()
    sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
    orc = O.Oracle(prob, "h16d", settings)
    bnds_h, xref_h = tuple(O.round_h16(b) for b in bnds), O.round_h16(xref)
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = O.round_h16(x0)
    for k in range(3):  # cold start, then two WARM starts that keep the fp32 duals
        if k == 1:
            st["y"][:] = 0; st["g"][:] = 0
            sol.reset_dual_variables()
        st32 = O.copy_state(st)
        orc.solve(st, *bnds_h, xref_h, nthreads=8)
        sol.solve()
        got = sol.get_state()
        for name in STATE_ORDER:
            if name not in ("g", "y"):
                assert np.array_equal(got[name], O.round_h16(got[name])), f"{name} is not binary16-representable"
        if exact:
            assert_bitwise(got, st, f"h16d {case} k={k}")
        else:
            O.Oracle(prob, np.float32, settings).solve(st32, *bnds_h, xref_h, nthreads=8)  # the quantisation yardstick
            same32 = st32["iter"] == st["iter"]
            same = (got["iter"] == st["iter"]) & (got["status"] == st["status"])
            f32flips = float((~same32).mean())
            assert (~same).mean() <= max(1.5 * f32flips, 0.02) + 1.0 / B, \
                f"h16d fast {case} k={k}: {(~same).mean():.2f} change the iteration count; fp16 storage itself changes {f32flips:.2f} vs fp32"
            for name in STATE_ORDER:
                # a dual is a sum of differences of binary16 values: flipped fp16 bits of x (u) move g (y) by ulps of x (u)
                ref = {"g": "x", "y": "u"}.get(name, name)
                scale = max(float(np.abs(st[ref]).max()), 1e-2)
                err = np.abs(got[name][same].astype(np.float64) - st[name][same]).max() / scale
                sel = same32 if same32.any() else slice(None)
                spread = np.abs(st32[name][sel].astype(np.float64) - st[name][sel]).max() / scale
                assert err <= max(4 * 2.0 ** -10, 4 * spread), \
                    f"h16d fast {case} k={k}: {name} off by {err:.2e} of the magnitude of {ref} (storage spread {spread:.2e})"
            sol.set_state(st)
    # the duals round-trip through the accessors as fp32, the primal arrays as binary16
    gnew = (st["g"] + np.float32(1e-5)).astype(np.float32)
    sol.set_array("g", gnew)
    assert np.array_equal(sol.get_array("g"), gnew)
    sol.set_array("d", st["d"] + np.float32(1e-4))
    assert np.array_equal(sol.get_array("d"), O.round_h16(st["d"] + np.float32(1e-4)))
    # outside the register-resident kernels the mode is refused, loudly
    sol.set_bounds(*[np.broadcast_to(b, (B,) + b.shape).copy() for b in bnds])  # per-instance bounds -> streaming row kernel
    with pytest.raises(tinympc.TinyBatchError):
        sol.solve()
    sol.close()
    s2 = tinympc.TinyBatchSolver(pr.quadrotor(20, 17), 8, settings=settings)  # no rowlane instantiation for N = 17
    with pytest.raises(tinympc.TinyBatchError):
        s2.set_storage(16, 32)
    s2.close()


def test_fp16_storage_step_functions(tinympc, oracle_mod):
    """The six step functions under fp16 storage: each equals the oracle's _h16 restatement bit for bit."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 17)
    nx, nu, N, B = 12, 4, 17, 19
    rng = np.random.default_rng(5)
    bnds = tuple(O.round_h16(a * s) for a, s in zip(pr.bounds_arrays(prob), (0.2, 0.2, 1.0, 1.0)))
    st = O.new_state(B, nx, nu, N)
    for k in STATE_ORDER:
        st[k][:] = O.round_h16(rng.standard_normal(st[k].shape) * 0.3)
    st["iter"][:] = 2; st["status"][:] = 11
    xref = O.round_h16(rng.standard_normal((B, N, nx)) * 0.3)
    settings = dict(O.DEFAULT_SETTINGS, check_termination=2, abs_pri_tol=0.5, abs_dua_tol=5.0)
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.set_storage(16, 16)
    sol.set_bounds(*bnds); sol.set_xref(xref)
    orc = O.Oracle(prob, "h16", settings)
    for fn in O.Oracle.STEP_FUNCTIONS:
        sol.set_state(st)
        ref_rv = orc.step(fn, st, *bnds, xref)
        rv = getattr(sol, fn)()
        if fn == "termination_condition":
            assert np.array_equal(rv, ref_rv)
        got = sol.get_state()
        for k in STATE_ORDER + ("residuals",):
            assert np.array_equal(got[k], st[k]), f"h16 {fn}: {k}"
    sol.close()


def test_mixed_size_group_solve_fp16(tinympc, oracle_mod):
    """BASELINE.json configs[4] as one call: a cartpole class and a quadrotor class, both with fp16 storage, solved by
    tiny_batch_group_solve; each class stays bitwise equal to its oracle, and the group result equals separate solves."""
    O, pr = oracle_mod, tinympc.problems
    sols, refs = [], []
    for prob, B in ((pr.cartpole(10), 3001), (pr.quadrotor(20, 30), 2002)):
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        rng = np.random.default_rng(B)
        x0 = rng.uniform(-0.2, 0.2, size=(B, nx)).astype(np.float32)
        xref = np.zeros((N, nx), np.float32)
        bnds = pr.bounds_arrays(prob)
        settings = dict(O.DEFAULT_SETTINGS, max_iter=150)
        sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
        sol.set_storage(16, 16)
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = O.round_h16(x0)
        O.Oracle(prob, "h16", settings).solve(st, *[O.round_h16(b) for b in bnds], xref, nthreads=8)
        sols.append(sol); refs.append(st)
    n_unsolved = tinympc.solve_group(sols)
    assert n_unsolved == sum(int((st["status"] != 1).sum()) for st in refs)
    for sol, st in zip(sols, refs):
        assert_bitwise(sol.get_state(), st, "group " + sol.kernel_name())
        sol.close()


def test_device_pointer_io_equals_host_io(tinympc):
    """set_xref_device / set_array_device / get_array_device (device-resident fp32 arrays in the ABI layout, no host round
    trip) give bit-identical results to the host-pointer calls."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B, N, nx, nu = 517, 30, 12, 4
    x0, table, start = pr.tracking_batch(B, N, seed=4)
    xref = pr.expand_windows(table, start, N)
    xfull = np.zeros((B, N, nx), np.float32); xfull[:, 0] = x0

    def dev(a):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0  # H2D
        return p

    ref = tinympc.TinyBatchSolver(prob, B)
    ref.set_bounds(*pr.bounds_arrays(prob)); ref.set_xref(xref); ref.set_x0(x0); ref.solve()
    sol = tinympc.TinyBatchSolver(prob, B)
    sol.set_bounds(*pr.bounds_arrays(prob))
    d_xref, d_x = dev(xref), dev(xfull)
    sol._check(sol.lib.tiny_batch_set_xref_device(sol._h, d_xref, 0))
    sol._check(sol.lib.tiny_batch_set_array_device(sol._h, tinympc.ARRAY_IDS["x"], d_x))
    sol.solve()
    u = np.empty((B, N - 1, nu), np.float32)
    d_u = dev(u)
    sol._check(sol.lib.tiny_batch_get_array_device(sol._h, tinympc.ARRAY_IDS["u"], d_u))
    sol.synchronize()
    assert hip.hipMemcpy(u.ctypes.data_as(ctypes.c_void_p), d_u, ctypes.c_size_t(u.nbytes), 2) == 0  # D2H
    assert np.array_equal(u, ref.get_u()) and np.array_equal(sol.get_x(), ref.get_x())
    assert np.array_equal(sol.get_status()[0], ref.get_status()[0])
    for p in (d_xref, d_x, d_u):
        hip.hipFree(p)
    sol.close(); ref.close()


@pytest.mark.parametrize("wave_kernel", ["wavestream", "waveres", "tile48"])
@pytest.mark.parametrize("B", [1, 3, 66])
def test_wave_kernel_vs_oracle(tinympc, oracle_mod, B, wave_kernel):
    """nx = 32, nu = 16, N = 50 (BASELINE.json configs[3]) on the two wave-per-instance exact kernels (state streamed through
    HBM / state in registers and LDS, the default for N <= 50 below 4 096 instances) and on the sixteen-instances-per-workgroup
    matrix-core kernel (the default wherever its rounds of 4 096 instances beat the wave kernel's of 2 048): bitwise equal to the
    oracle (== the compiled reference for this class, tests/test_oracle.py) over a warm-started chain, with early exit,
    sparse termination checks, one iteration, bounds disabled and a random time-varying reference."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.random_system(32, 16, 50)
    nx, nu, N = 32, 16, 50
    rng = np.random.default_rng(B)
    x0 = rng.uniform(-1, 1, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.2).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    for settings in (dict(max_iter=40), dict(max_iter=25, check_termination=4), dict(max_iter=1),
                     dict(max_iter=12, en_state_bound=0, en_input_bound=0), dict(max_iter=0)):
        settings = dict(O.DEFAULT_SETTINGS, **settings)
        sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
        assert sol.kernel_name() == "waveres<32,16,exact>", sol.kernel_name()   # the automatic choice
        sol.set_row_kernel({"wavestream": 6, "waveres": 7, "tile48": 8}[wave_kernel])
        assert sol.kernel_name() == (f"{wave_kernel}<32,16,exact>" if wave_kernel != "tile48" else "tile48<32,16,50,exact>"), sol.kernel_name()
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
        orc = O.Oracle(prob, np.float32, settings)
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
        for k in range(3):
            st["y"][:] = 0; st["g"][:] = 0
            sol.reset_dual_variables()
            rc_ref = orc.solve(st, *bnds, xref, nthreads=8)
            rc = sol.solve()
            assert rc == (1 if rc_ref else 0)
            assert_bitwise(sol.get_state(), st, f"wave B={B} {settings} k={k}")
        if wave_kernel == "wavestream":
            with pytest.raises(tinympc.TinyBatchError):
                sol.select_kernel(3)  # fma arithmetic for this class: the state-on-chip wave kernel or the streaming kernel
        else:
            sol.select_kernel(3)
            assert sol.kernel_name() == ("waveres<32,16,fast>" if wave_kernel == "waveres" else "tile48<32,16,50,fast>"), sol.kernel_name()
        sol.select_kernel(1)          # the streaming MFMA kernel takes over the same workspace
        assert sol.kernel_name() == "stream<8,4>"
        got = sol.get_state()
        for name in STATE_ORDER:
            assert np.array_equal(got[name], st[name]), f"layout switch lost {name}"
        sol.close()


@pytest.mark.parametrize("N", [50, 37, 2])
def test_tile48_kernel_equals_wave_kernel_bitwise(tinympc, N):
    """admm_tile48.hip (sixteen instances per workgroup, products on the matrix cores, duals in LDS, slack streamed through its own
    array) against the one-wave-per-instance kernel it replaces for large batches: every work array, residuals, iteration counts
    and status bit for bit — ragged batches (columns past the batch), per-instance bounds, window of a trajectory table as the
    reference, warm-started chains in which the columns of a tile converge at different iterations, sparse termination checks,
    horizons below the capacity of 50; and the automatic choice (by rounds of the launch)."""
    pr = tinympc.problems
    nx, nu = 32, 16
    prob = pr.random_system(nx, nu, N)
    shared = pr.bounds_arrays(prob)
    if N == 50:   # the automatic choice goes by rounds of the launch (256 CUs: 2 048 instances per round of the wave kernel, 4 096 of the tile kernel)
        for B, name in ((2048, "waveres"), (2049, "tile48"), (4096, "tile48"), (4352, "waveres"), (6144, "waveres"), (6145, "tile48"), (16384, "tile48")):
            sol = tinympc.TinyBatchSolver(prob, B)
            assert sol.kernel_name().startswith(name), (B, sol.kernel_name())
            sol.select_kernel(3)
            assert sol.kernel_name().startswith(name) and sol.kernel_name().endswith("fast>"), (B, sol.kernel_name())
            sol.close()
    for B, settings, per_inst, window in ((4096, dict(max_iter=30), False, False), (1000, dict(max_iter=100, abs_pri_tol=3e-2, abs_dua_tol=3e-2), True, False),
                                         (37, dict(max_iter=60, check_termination=7, abs_pri_tol=3e-2, abs_dua_tol=3e-2), False, True), (16, dict(max_iter=1), True, True)):
        s = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1); s.update(settings)
        rng = np.random.default_rng(B + N)
        x0 = rng.uniform(-1, 1, size=(B, nx)).astype(np.float32)
        bnds = tuple((a[None] * rng.uniform(0.2, 1.0, size=(B,) + a.shape)).astype(np.float32) for a in shared) if per_inst else shared
        sols = []
        for fam in (7, 8):
            sol = tinympc.TinyBatchSolver(prob, B, settings=s)
            if B >= 4096 and N == 50:
                assert sol.kernel_name() == "tile48<32,16,50,exact>", sol.kernel_name()   # the automatic choice
            sol.set_row_kernel(fam)
            assert sol.kernel_name() == (f"waveres<32,16,exact>" if fam == 7 else f"tile48<32,16,{N},exact>"), sol.kernel_name()
            sol.set_bounds(*bnds)
            if window:
                table = (rng.standard_normal((N + 40, nx)) * 0.2).astype(np.float32) if fam == 7 else table
                start = rng.integers(0, 41, size=B).astype(np.int32) if fam == 7 else start
                sol.set_xref_window(table, start)
            else:
                xref = (rng.standard_normal((B, N, nx)) * 0.2).astype(np.float32) if fam == 7 else xref
                sol.set_xref(xref)
            sol.set_x0(x0)
            sols.append(sol)
        for k in range(3):
            sts = []
            for sol in sols:
                if k == 1:
                    sol.reset_dual_variables()
                rc = sol.solve(); st = sol.get_state(); st["rc"] = np.array([rc]); sts.append(st)
            for name in sts[0]:
                assert np.asarray(sts[0][name]).tobytes() == np.asarray(sts[1][name]).tobytes(), f"tile48 vs waveres: {name}, B={B} N={N} {settings} k={k}"
            if B == 1000 and N == 50 and k == 0:
                assert len(np.unique(sts[1]["iter"])) > 3, "the columns of a tile should stop at different iterations in this case"
        for sol in sols:
            sol.close()


@pytest.mark.parametrize("dims", [(32, 16, 50), (16, 8, 49), (16, 4, 33), (20, 8, 21), (32, 16, 50, "tile48"), (32, 16, 31, "tile48")])
def test_wave_kernel_fma_arithmetic(tinympc, oracle_mod, dims):
    """fma arithmetic of the state-on-chip wave kernel (waveres<...,fast>) and of the matrix-core tile kernel of the nx = 32 class
    (tile48<...,fast>: every stage one fma chain on the matrix cores): held to the bar of every other fma variant —
    iteration counts and arrays within the reference's own fp64-vs-fp32 spread (compare_states) — over a warm-started
    chain, with the early exit and with a fixed iteration count."""
    O, pr = oracle_mod, tinympc.problems
    tile = len(dims) == 4
    nx, nu, N = dims[:3]
    prob = pr.random_system(nx, nu, N)
    B = 96
    rng = np.random.default_rng(nx + N)
    x0 = rng.uniform(-1, 1, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.2).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    for extra, fixed in ((dict(max_iter=60), False), (dict(max_iter=9, abs_pri_tol=0.0, abs_dua_tol=0.0), True)):
        settings = dict(O.DEFAULT_SETTINGS, **extra)
        sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
        sol.select_kernel(3)
        assert sol.kernel_name() == f"waveres<{nx},{nu},fast>", sol.kernel_name()
        if tile:
            sol.set_row_kernel(8)
            assert sol.kernel_name() == f"tile48<{nx},{nu},{N},fast>", sol.kernel_name()
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
        orc = O.Oracle(prob, np.float32, settings, allow_unpinned_dims=True)
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
        for k in range(3):
            st["y"][:] = 0; st["g"][:] = 0
            sol.reset_dual_variables()
            pre = O.copy_state(st)
            orc.solve(st, *bnds, xref, nthreads=8)
            sol.solve()
            ref64 = None if fixed else yardstick(O, prob, settings, pre, xref, bnds)
            compare_states(sol.get_state(), st, prob, f"waveres fast {dims} {extra} k={k}", ref64=ref64, fixed=fixed)
            sol.set_state(st)
        sol.close()


@pytest.mark.parametrize("dims", [(20, 12, 12), (6, 2, 9), (30, 10, 7), (5, 5, 8), (3, 2, 6), (10, 3, 11), (40, 12, 6), (64, 32, 4), (33, 17, 5)])
def test_classes_without_an_instantiation_run_on_the_padded_mfma_kernel(tinympc, oracle_mod, dims):
    """The reference takes any NSTATES / NINPUTS / NHORIZON (glob_opts.hpp:5-7).  A class with no compiled exact kernel is
    served, in fma arithmetic, by the smallest MFMA streaming instantiation that contains it (any nx <= 64, nu <= 32, any N).
    Round 3: the yardstick is the COMPILED REFERENCE of exactly that class (oracle/Makefile FALLBACK_CONFIGS, fp32 and fp64
    builds), not an unpinned restatement: at a fixed iteration count every array stays within 4x the reference's own
    fp64-vs-fp32 spread (floor 2e-5 of the array's scale); with early exit the same instances converge, iteration counts
    within the spread of the two reference builds + 2."""
    O, pr = oracle_mod, tinympc.problems
    nx, nu, N = dims
    if not (O.have_ref(np.float32, nx, nu, N) and O.have_ref(np.float64, nx, nu, N)):
        pytest.skip("oracle/_ref has no build of this class (needs /root/reference at build time)")
    prob = pr.random_system(nx, nu, N, seed=nx * 31 + nu)
    B = 53
    rng = np.random.default_rng(N)
    x0 = rng.uniform(-0.5, 0.5, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.1).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    bnds64 = [np.asarray(b, np.float64) for b in bnds]
    for extra in (dict(max_iter=8, abs_pri_tol=0.0, abs_dua_tol=0.0), dict(max_iter=60)):
        settings = dict(O.DEFAULT_SETTINGS, **extra)
        sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
        # round 4: the arithmetic mode is a contract — the automatic choice is exact arithmetic or nothing, fma arithmetic is an opt-in
        if all(d <= 4 or d % 4 == 0 for d in (nx, nu)) and nx <= 36:   # the reference's orders are defined: the run-time-dimension exact kernel
            assert sol.kernel_name() == f"generic<{nx},{nu},exact>" and sol.arithmetic() == "exact", sol.kernel_name()
        else:
            assert sol.kernel_name() == "unsupported"
            with pytest.raises(tinympc.TinyBatchError, match="opts into fma"):
                sol.arithmetic()
            with pytest.raises(tinympc.TinyBatchError, match="opts into fma"):
                sol.solve()
        sol.select_kernel(1)
        assert sol.kernel_name().startswith("stream<") and sol.arithmetic() == "fma", sol.kernel_name()
        sol.solve()
        got = sol.get_state()
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
        O.Reference(prob, np.float32, settings).solve(st, *bnds, xref)                       # the reference's fp32 build
        s64 = O.new_state(B, nx, nu, N, np.float64); s64["x"][:, 0] = x0
        O.Reference(prob, np.float64, settings).solve(s64, *bnds64, xref.astype(np.float64))  # ... and its fp64 build
        if extra["max_iter"] == 8:
            assert np.array_equal(got["iter"], st["iter"]) and np.array_equal(got["status"], st["status"])
            for k in ("x", "u", "d", "p", "y", "g", "v", "z"):
                scale = max(float(np.abs(st[k]).max()), 1e-2)
                err = float(np.abs(got[k].astype(np.float64) - st[k]).max()) / scale
                spread = float(np.abs(s64[k] - st[k]).max()) / scale
                assert err <= max(4.0 * spread, 2e-5), f"{dims} {k}: GPU-vs-reference {err:.2e}, reference fp64-vs-fp32 {spread:.2e}"
        else:
            same = got["status"] == st["status"]
            same_ref = s64["status"] == st["status"]
            assert same.mean() >= min(0.9, same_ref.mean()), (dims, same.mean(), same_ref.mean())
            ref_iter_spread = int(np.abs(s64["iter"][same_ref].astype(int) - st["iter"][same_ref]).max()) if same_ref.any() else 0
            assert np.abs(got["iter"][same].astype(int) - st["iter"][same]).max() <= ref_iter_spread + 2
        sol.close()
    with pytest.raises(tinympc.TinyBatchError):
        tinympc.TinyBatchSolver(pr.random_system(68, 4, 5, seed=1), 4)   # nx > 64: no kernel at all, refused at create


@pytest.mark.parametrize("variant_name", ["row_exact", "row_fast", "loop_exact", "stream", "generic"])
def test_mpc_run_equals_step_by_step(tinympc, variant_name):
    """tiny_batch_mpc_run_async(steps) leaves exactly the state that `steps` calls of tiny_batch_mpc_step_async leave, in both
    implementations: the on-chip closed loop of the unrolled row kernel (row_* variants: one launch, the state stays in
    registers/LDS between solves) and the (solve + plant step) x steps sequence captured once into a hipGraph (the other
    kernels).  A second run continues the trajectory; a change of settings rebuilds the graph."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 48
    x0, table, start = pr.tracking_batch(B, 30, seed=11)
    bnds = pr.bounds_arrays(prob)

    def mk():
        if variant_name != "generic":
            return make_solver(tinympc, prob, B, None, None, variant_name, bnds)
        # variant 4, the run-time-dimension kernel (not in VARIANTS: every test driven by the `variant` fixture iterates over that dict)
        s = tinympc.TinyBatchSolver(prob, B)
        s.select_kernel(4)
        s.set_bounds(*bnds)
        assert s.kernel_name() == "generic<12,4,exact>", s.kernel_name()
        return s

    a, b = mk(), mk()
    for s in (a, b):
        s.set_xref_window(table, start)
        s.set_x0(x0)
    for rounds in range(2):
        a.mpc_run_async(6, 1)
        for _ in range(6):
            b.mpc_step_async(1)
        sa, sb = a.get_state(), b.get_state()
        for k in STATE_ORDER + SCALARS:
            assert np.array_equal(sa[k], sb[k]), f"round {rounds}: {k}"
        assert np.array_equal(a.get_x0(), b.get_x0())
    for s in (a, b):
        s.set_settings(**dict(s.settings, max_iter=7))   # baked into the captured kernel arguments: the graph must be rebuilt
    a.mpc_run_async(3, 0)
    for _ in range(3):
        b.mpc_step_async(0)
    assert np.array_equal(a.get_u(), b.get_u()) and np.array_equal(a.get_status()[0], b.get_status()[0])
    assert a.get_status()[0].max() <= 7
    a.close(); b.close()


@pytest.mark.parametrize("B", [1, 15, 16, 17, 333])
def test_quadlane_kernel_vs_oracle(tinympc, oracle_mod, B):
    """The four-lanes-per-instance kernel (cartpole class) against the oracle: ragged batches around its 16-instance
    wave, warm-started chain, sparse termination checks, one iteration, exhausted iterations, bounds disabled, per-step
    bounds, time-varying per-instance reference, window reference; exact arithmetic bitwise, fma arithmetic to the
    yardstick."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.cartpole(10)
    nx, nu, N = 4, 1, 10
    rng = np.random.default_rng(B)
    x0 = (np.array([0, 0, 0.1, 0], np.float32) + rng.uniform(-0.05, 0.05, size=(B, nx))).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.05).astype(np.float32)
    xmn, xmx, umn, umx = pr.bounds_arrays(prob)
    umn = umn * np.linspace(0.2, 1.0, N - 1, dtype=np.float32)[:, None]   # per-step input bounds, some of them active
    bnds = (xmn, xmx, umn, umx)
    for settings in (dict(max_iter=150), dict(max_iter=40, check_termination=3), dict(max_iter=1), dict(max_iter=4),
                     dict(max_iter=30, en_state_bound=0, en_input_bound=0), dict(max_iter=0)):
        settings = dict(O.DEFAULT_SETTINGS, **settings)
        for exact in (True, False):
            sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
            sol.select_kernel(2 if exact else 3)
            assert sol.kernel_name().startswith("quadlane<4,1,10"), sol.kernel_name()
            sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
            orc = O.Oracle(prob, np.float32, settings)
            st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
            for k in range(3):
                st["y"][:] = 0; st["g"][:] = 0
                sol.reset_dual_variables()
                pre = O.copy_state(st)
                orc.solve(st, *bnds, xref, nthreads=4)
                sol.solve()
                r64 = None if exact else yardstick(O, prob, settings, pre, xref, bnds)
                compare_states(sol.get_state(), st, prob, f"quadlane B={B} {settings} exact={exact} k={k}", ref64=r64, exact=exact,
                               ct=settings["check_termination"])
                if not exact:
                    sol.set_state(st)
            sol.close()


@pytest.mark.parametrize("variant_name", ["row_exact", "loop_exact"])
def test_mpc_run_records_the_input_trajectory(tinympc, variant_name):
    """tiny_batch_mpc_run_traj_async writes u.col(0) of every MPC step to a device buffer [steps][B][nu]: equal to what a
    host loop reads with get_u after every step (on-chip loop and graph replay alike); windows that run off the end of
    the trajectory table clamp like the reference's would."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B, K = 37, 9
    x0, table, start = pr.tracking_batch(B, 30, seed=21)
    start = np.minimum(start + 40, 301 - 30).astype(np.int32)  # some windows reach the end of the table within K steps
    bnds = pr.bounds_arrays(prob)
    a = make_solver(tinympc, prob, B, None, None, variant_name, bnds)
    b = make_solver(tinympc, prob, B, None, None, variant_name, bnds)
    for s in (a, b):
        s.set_xref_window(table, start)
        s.set_x0(x0)
    traj = np.zeros((K, B, 4), np.float32)
    d_traj = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_traj), ctypes.c_size_t(traj.nbytes)) == 0
    a._check(a.lib.tiny_batch_mpc_run_traj_async(a._h, K, 1, d_traj))
    a.synchronize()
    assert hip.hipMemcpy(traj.ctypes.data_as(ctypes.c_void_p), d_traj, ctypes.c_size_t(traj.nbytes), 2) == 0
    for k in range(K):
        b.reset_dual_variables(); b.solve()
        assert np.array_equal(traj[k], b.get_u()[:, 0]), f"step {k}"
        # advance b by hand: x_1 of the solve IS the plant step (the plant is the model, hovering.cpp:110); a window that
        # runs off the table keeps repeating its last row
        x_next = b.get_x()[:, 1]
        padded = np.vstack([table, np.repeat(table[-1:], K + 1, 0)])
        b.set_xref(pr.expand_windows(padded, start + k + 1, 30))
        b.set_x0(x_next)
    hip.hipFree(d_traj)
    a.close(); b.close()


@pytest.mark.parametrize("exact", [True, False])
def test_mpc_run_on_chip_cartpole(tinympc, exact):
    """The on-chip closed loop of the four-lanes-per-instance kernel (cartpole): K MPC steps in one launch leave the state
    of K step-by-step calls, with a per-instance time-varying reference held fixed and with a sliding window."""
    pr = tinympc.problems
    prob = pr.cartpole(10)
    B, K = 53, 12
    rng = np.random.default_rng(3)
    x0 = (np.array([0, 0, 0.1, 0], np.float32) + rng.uniform(-0.05, 0.05, size=(B, 4))).astype(np.float32)
    table = (rng.standard_normal((60, 4)) * 0.02).astype(np.float32)
    start = rng.integers(0, 30, size=B).astype(np.int32)
    for windowed in (False, True):
        sols = []
        for _ in range(2):
            s = tinympc.TinyBatchSolver(prob, B, settings=dict(max_iter=60))
            s.select_kernel(2 if exact else 3)
            assert s.kernel_name().startswith("quadlane"), s.kernel_name()
            s.set_bounds(*pr.bounds_arrays(prob))
            if windowed:
                s.set_xref_window(table, start)
            else:
                s.set_xref(pr.expand_windows(table, start, 10))
            s.set_x0(x0)
            sols.append(s)
        a, b = sols
        a.mpc_run_async(K, 1 if windowed else 0)
        for _ in range(K):
            b.mpc_step_async(1 if windowed else 0)
        sa, sb = a.get_state(), b.get_state()
        for k in STATE_ORDER + SCALARS:
            assert np.array_equal(sa[k], sb[k]), f"windowed={windowed}: {k}"
        assert np.array_equal(a.get_x0(), b.get_x0())
        a.close(); b.close()


def test_kernel_selection_and_option_errors(tinympc):
    """Every option that cannot be honoured is refused with a TinyBatchError and leaves the handle usable."""
    pr = tinympc.problems
    q17 = tinympc.TinyBatchSolver(pr.quadrotor(20, 17), 8)         # no unrolled instantiation for N = 17
    assert q17.kernel_name().startswith("rowloop")
    for bad in (1, 4, 5, -1):
        with pytest.raises(tinympc.TinyBatchError):
            q17.set_row_kernel(bad)
    q17.set_row_kernel(3); assert q17.kernel_name().startswith("rowstream")
    q17.set_row_kernel(0); assert q17.kernel_name().startswith("rowloop")
    with pytest.raises(tinympc.TinyBatchError):
        q17.set_storage(8)
    with pytest.raises(tinympc.TinyBatchError):
        q17.mpc_run_async(0, 0)
    with pytest.raises(tinympc.TinyBatchError):
        q17.set_dispatch(3)
    q17.set_dispatch(1); q17.set_dispatch(2)                                            # accepted everywhere, acts on large rowlane launches only
    q17.close()
    q40 = tinympc.TinyBatchSolver(pr.quadrotor(20, 70), 8)         # N > 64: only the streaming row kernel
    assert q40.kernel_name().startswith("rowstream")
    with pytest.raises(tinympc.TinyBatchError):
        q40.set_row_kernel(2)
    q40.close()
    r = tinympc.TinyBatchSolver(pr.random_system(32, 16, 50), 4)    # wave-per-instance class
    assert r.kernel_name().startswith("waveres")
    with pytest.raises(tinympc.TinyBatchError):
        r.set_storage(16, 16)                                          # fp16 storage: row kernels only
    with pytest.raises(tinympc.TinyBatchError):
        r.set_row_kernel(1)
    with pytest.raises(tinympc.TinyBatchError):
        r.forward_pass()                                           # single-function kernels: nx + nu <= 16
    r.select_kernel(1); assert r.kernel_name() == "stream<8,4>"
    r.close()
    a = tinympc.TinyBatchSolver(pr.cartpole(10), 4)
    with pytest.raises(tinympc.TinyBatchError):
        tinympc.solve_group([a, a])                                # the same handle twice
    assert tinympc.solve_group([a]) >= 0                           # a group of one is an ordinary solve
    a.close()


def test_per_instance_bounds_exact(tinympc, oracle_mod):
    """Per-instance (and per-step) box bounds — every reference workspace owns its u_min .. x_max (types.hpp:88-91) — in exact
    arithmetic: the quadrotor class stays on the register-resident row kernels (bounds read per lane-step from the [B][N][16]
    table: unrolled for N = 30 in fp32 storage, rolled-loop for fp16 storage and for horizons without an unrolled instantiation
    up to 64), longer horizons run on the streaming row kernel, the nx = 32 class on the wave kernel, and update_slack works as
    a separate call — all bitwise equal to the oracle."""
    O, pr = oracle_mod, tinympc.problems
    for prob, B, name in ((pr.quadrotor(20, 30), 37, "rowlane"), (pr.quadrotor(20, 17), 21, "rowloop"), (pr.quadrotor(20, 47), 9, "rowloop"),
                          (pr.quadrotor(20, 66), 6, "rowstream"), (pr.random_system(32, 16, 50), 5, "waveres")):
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        rng = np.random.default_rng(B)
        x0 = rng.uniform(-0.4, 0.4, size=(B, nx)).astype(np.float32)
        xref = (rng.standard_normal((N, nx)) * 0.1).astype(np.float32)
        bnds = tuple((a[None] * rng.uniform(0.05, 1.0, size=(B,) + a.shape)).astype(np.float32) for a in pr.bounds_arrays(prob))
        settings = dict(O.DEFAULT_SETTINGS, max_iter=25, check_termination=2)
        for storage in ((32, 16) if name != "waveres" else (32,)):
            sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
            sol.set_storage(storage, storage)
            sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
            want = "rowloop" if (storage == 16 and name == "rowlane") else name
            assert sol.kernel_name().startswith(want), sol.kernel_name()
            R = O.round_h16 if storage == 16 else (lambda a: a)
            orc = O.Oracle(prob, "h16" if storage == 16 else np.float32, settings)
            st = O.new_state(B, nx, nu, N); st["x"][:, 0] = R(x0)
            bn = tuple(R(b) for b in bnds)
            for k in range(2):
                st["y"][:] = 0; st["g"][:] = 0
                sol.reset_dual_variables()
                orc.solve(st, *bn, R(xref), nthreads=8)
                sol.solve()
                assert_bitwise(sol.get_state(), st, f"per-instance bounds {sol.kernel_name()} k={k}")
            if name != "waveres":
                orc.step("update_slack", st, *bn, R(xref))
                sol.update_slack()
                assert_bitwise(sol.get_state(), st, "update_slack with per-instance bounds")
            sol.close()


@pytest.mark.parametrize("variant_name", ["row_exact", "loop_exact", "rowstream_exact", "lane_exact", "stream"])
def test_cold_start_that_converges_immediately(tinympc, oracle_mod, variant_name):
    """reset_workspace() then a solve from x0 = 0 with a zero reference converges in its first iteration, before any backward
    sweep: p, d, v, z must read back as the zeros reset_workspace() promised (not whatever an earlier solve left in memory),
    and x, u follow from d = 0.  Found by tests/fuzz/fuzz_api.py on the kernels that stream their state."""
    O, pr = oracle_mod, tinympc.problems
    for prob in (pr.quadrotor(20, 30), pr.cartpole(10), pr.random_system(32, 16, 50)):
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        B = 9
        rng = np.random.default_rng(1)
        bnds = pr.bounds_arrays(prob)
        try:
            sol = make_solver(tinympc, prob, B, dict(O.DEFAULT_SETTINGS, max_iter=30), None, variant_name, bnds)
        except pytest.skip.Exception:
            continue
        # dirty the workspace with an ordinary solve first
        sol.set_xref((rng.standard_normal((N, nx)) * 0.2).astype(np.float32))
        sol.set_x0(rng.uniform(-0.3, 0.3, size=(B, nx)).astype(np.float32))
        sol.solve()
        sol.set_xref(np.zeros((N, nx), np.float32))
        sol.reset_workspace()                      # x0 stays 0
        sol.solve()
        got = sol.get_state()
        assert np.all(got["iter"] == 1) and np.all(got["status"] == 1)
        for name in STATE_ORDER:
            assert not np.any(got[name]), f"{sol.kernel_name()}: {name} is not zero after a trivially converged cold start"
        sol.close()


@pytest.mark.parametrize("tool", ["fuzz_parity.py", "fuzz_mpc.py", "fuzz_api.py", "fuzz_native.py", "fuzz_fast_families.py",
                                  "fuzz_stream_consistency.py"])
def test_randomised_differential_tools_short_run(tool):
    """A few seconds of each randomised differential tool (tests/fuzz/fuzz_*.py; the minutes-long runs are recorded in DESIGN.md),
    with a fixed seed so that the test is reproducible: keeps the tools working and replays a few thousand drawn cases."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / "tests" / "fuzz" / tool), "6", "1"], capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0 and "fuzz ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("dims", [(16, 8, 10), (16, 4, 12), (16, 4, 33), (16, 8, 49), (16, 4, 60), (20, 8, 10), (20, 8, 37), (24, 4, 10), (24, 4, 55)])
def test_wave_kernel_other_classes(tinympc, oracle_mod, dims):
    """Four more classes of the wave-per-instance kernel, each pinned against its own reference build in test_oracle.py:
    (16,8) and (20,8) take Eigen's GEMV path like (32,16), (16,4) and (24,4) do not.  Horizons on both sides of the register vectors' 32- and
    48-step seams of the state-on-chip kernel, and one beyond its 50 steps (streaming kernel)."""
    O, pr = oracle_mod, tinympc.problems
    nx, nu, N = dims
    prob = pr.random_system(nx, nu, N, seed=nx * 100 + nu)
    B = 21
    rng = np.random.default_rng(nx + nu)
    x0 = rng.uniform(-0.5, 0.5, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.2).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=40, check_termination=2)
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    assert sol.kernel_name() == f"{'waveres' if N <= 50 else 'wavestream'}<{nx},{nu},exact>", sol.kernel_name()
    sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
    orc = O.Oracle(prob, np.float32, settings)
    st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
    for k in range(3):
        st["y"][:] = 0; st["g"][:] = 0
        sol.reset_dual_variables()
        orc.solve(st, *bnds, xref, nthreads=8)
        sol.solve()
        assert_bitwise(sol.get_state(), st, f"wave {dims} k={k}")
    sol.close()


OPT_CASES = {"quad30": lambda pr: pr.quadrotor(20, 30), "quad45": lambda pr: pr.quadrotor(20, 45), "cartpole": lambda pr: pr.cartpole(10),
             "dims_8_4_9": lambda pr: pr.random_system(8, 4, 9, seed=5), "dims_12_2_11": lambda pr: pr.random_system(12, 2, 11, seed=6)}


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("case", list(OPT_CASES))
def test_optional_terms_vs_oracle(tinympc, oracle_mod, case, exact):
    """The two terms the reference ships commented out (admm.cpp:20 "+ coeff_d2p * d", admm.cpp:79 Uref), switched on:
    fused solve chain and the two step functions they live in, against the oracle (itself pinned against Eigen in
    tests/test_oracle.py) — bitwise in exact arithmetic, fp64-yardstick in fma arithmetic; per-instance and shared Uref;
    fp16 storage; switching them off again restores the default kernels and the reference's results."""
    O, pr = oracle_mod, tinympc.problems
    prob = dict(OPT_CASES[case](pr))
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    rng = np.random.default_rng(nx * 7 + nu)
    prob["coeff_d2p"] = (rng.standard_normal((nx, nu)) * 0.02).astype(np.float32)
    prob["R"] = rng.uniform(0.5, 2.0, nu).astype(np.float32)
    B = 41
    bnds = pr.bounds_arrays(prob)
    x0 = (rng.uniform(-0.3, 0.3, (B, nx)) * (0.2 if case == "cartpole" else 1.0)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.05).astype(np.float32)
    umax = float(np.max(bnds[3]))
    settings = dict(O.DEFAULT_SETTINGS, max_iter=30, check_termination=2, en_uref=1, en_coeff_d2p=1)
    base = {k: v for k, v in settings.items() if not k.startswith("en_u") and not k.startswith("en_c")}
    for storage, shared in ((32, False), (32, True), (16, False)):
        R16 = O.round_h16 if storage == 16 else (lambda a: a)
        uref = (rng.uniform(-0.3, 0.3, ((N - 1, nu) if shared else (B, N - 1, nu))) * umax).astype(np.float32)
        uref[..., 0, :] = 0.0
        sol = tinympc.TinyBatchSolver(prob, B, settings=base)
        sol.select_kernel(2 if exact else 3)
        sol.set_storage(storage, storage)
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
        default_kernel = sol.kernel_name()
        sol.set_optional_terms(True, True)
        with pytest.raises(tinympc.TinyBatchError):  # enabled but R / Uref / coeff_d2p not given yet
            sol.solve()
        sol.set_input_cost(prob["R"]); sol.set_coeff_d2p(prob["coeff_d2p"]); sol.set_uref(uref)
        # round 4: with fp32 storage (and batch-shared bounds) the terms live in the register-resident kernel where the class has one —
        # no reroute to the kernel that streams its state; fp16 storage still takes that one
        if storage == 32 and default_kernel.startswith(("rowlane", "quadlane")):
            assert sol.kernel_name().startswith("rowlane"), (default_kernel, sol.kernel_name())
        else:
            assert sol.kernel_name().startswith("rowstream"), sol.kernel_name()
        dt = "h16" if storage == 16 else np.float32
        orc = O.Oracle(prob, dt, settings)
        orc.set_uref(R16(uref))
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = R16(x0)
        bn = tuple(R16(b) for b in bnds)
        for k in range(3):
            pre = O.copy_state(st)
            orc.solve(st, *bn, R16(xref), nthreads=8)
            sol.solve()
            got = sol.get_state()
            what = f"optional terms {case} {sol.kernel_name()} shared={shared} k={k}"
            if exact:
                assert_bitwise(got, st, what)
            else:
                ref64 = yardstick(O, prob, settings, pre, R16(xref), bn, uref=R16(uref)) if storage == 32 else None
                if storage == 32:
                    compare_states(got, st, prob, what, ref64=ref64, ct=2)
                sol.set_state(st)  # continue the chain from the oracle's state
        assert np.abs(st["u"]).max() > 0 and st["iter"].max() > 1
        # the two step functions the terms live in, on a random workspace
        for k in STATE_ORDER:
            st[k][:] = R16((rng.standard_normal(st[k].shape) * 0.3).astype(np.float32))
        for fn in ("update_linear_cost", "backward_pass_grad"):
            sol.set_state(st)
            orc.step(fn, st, *bn, R16(xref))
            getattr(sol, fn)()
            got = sol.get_state()
            for k in STATE_ORDER:
                if exact:
                    assert np.array_equal(got[k], st[k]) and np.array_equal(np.signbit(got[k]), np.signbit(st[k])), (case, fn, k, storage)
                elif storage == 32:
                    assert np.max(np.abs(got[k].astype(np.float64) - st[k])) <= 2e-5 * max(1.0, float(np.abs(st[k]).max())), (case, fn, k)
        # the terms are live: the same solve without them gives different inputs
        st2 = O.new_state(B, nx, nu, N); st2["x"][:, 0] = R16(x0)
        ref_on, ref_off = O.copy_state(st2), O.copy_state(st2)
        orc.solve(ref_on, *bn, R16(xref), nthreads=8)
        O.Oracle(prob, dt, base).solve(ref_off, *bn, R16(xref), nthreads=8)
        assert not np.array_equal(ref_on["u"], ref_off["u"])
        # switched off again: default kernel, the reference's results
        sol.set_optional_terms(False, False)
        assert sol.kernel_name() == default_kernel
        sol.reset_workspace(); sol.set_x0(x0)
        sol.solve()
        if exact:
            assert_bitwise(sol.get_state(), ref_off, f"{case} terms switched off again")
        sol.close()


def test_optional_terms_closed_loop_native_and_errors(tinympc, oracle_mod):
    """Optional terms in the closed loop (graph replay == step by step), through the reference's own names (TinySolver
    members R, Uref, coeff_d2p become live), and the refusals: classes without a row kernel and the MFMA variant."""
    O, pr = oracle_mod, tinympc.problems
    prob = dict(pr.quadrotor(20, 30))
    nx, nu, N = 12, 4, 30
    rng = np.random.default_rng(3)
    prob["coeff_d2p"] = (rng.standard_normal((nx, nu)) * 0.02).astype(np.float32)
    B = 19
    uref = rng.uniform(-0.1, 0.1, (B, N - 1, nu)).astype(np.float32)
    x0, table, start = pr.tracking_batch(B, N, seed=4)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=20)

    def make():
        s = tinympc.TinyBatchSolver(prob, B, settings=settings)
        s.set_bounds(*pr.bounds_arrays(prob)); s.set_xref_window(table, start); s.set_x0(x0)
        s.set_input_cost(prob["R"]); s.set_coeff_d2p(prob["coeff_d2p"]); s.set_uref(uref); s.set_optional_terms(True, True)
        return s
    a, b = make(), make()
    a.mpc_run_async(4, 1); a.synchronize()
    for _ in range(4):
        b.mpc_step_async(1)
    b.synchronize()
    assert_bitwise(a.get_state(), b.get_state(), "optional terms: graph replay vs step by step")
    assert np.array_equal(a.get_x0(), b.get_x0())
    # ... and the first of those solves is the oracle's
    c = make(); c.solve()
    orc = O.Oracle(prob, np.float32, dict(settings, en_uref=1, en_coeff_d2p=1)); orc.set_uref(uref)
    st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
    orc.solve(st, *pr.bounds_arrays(prob), pr.expand_windows(table, start, N), nthreads=8)
    assert_bitwise(c.get_state(), st, "optional terms with a window reference")
    # MFMA variant and classes beyond 16 lanes refuse
    with pytest.raises(tinympc.TinyBatchError, match="optional"):
        c.select_kernel(1); c.solve()
    for s in (a, b, c):
        s.close()
    big = pr.random_system(32, 16, 50)
    s = tinympc.TinyBatchSolver(big, 3, settings=settings)
    s.set_bounds(*pr.bounds_arrays(big)); s.set_xref(np.zeros((50, 32), np.float32)); s.set_x0(np.zeros((3, 32), np.float32))
    s.set_input_cost(big["R"]); s.set_coeff_d2p(np.zeros((32, 16), np.float32)); s.set_uref(np.zeros((49, 16), np.float32))
    s.set_optional_terms(True, False)
    with pytest.raises(tinympc.TinyBatchError, match="optional"):
        s.solve()
    s.set_optional_terms(False, False)
    s.solve()
    s.close()
    # the reference's own names: TinySolver members R, Uref, coeff_d2p
    from accelerated_tinympc_amd import native
    ns = native.NativeSolver(prob, settings)
    try:
        ns.set_optional_terms(True, True)
        ns.a["x"][0] = x0[0]; ns.a["Xref"][:] = table[:N]; ns.a["Uref"][:] = uref[0]
        for k, v in zip(("x_min", "x_max", "u_min", "u_max"), pr.bounds_arrays(prob)):
            ns.a[k][:] = v
        orc.set_uref(uref[0])
        st = O.new_state(1, nx, nu, N); st["x"][0, 0] = x0[0]
        for k in range(2):
            rc = ns.tiny_solve()
            ref_rc = orc.solve(st, *pr.bounds_arrays(prob), table[:N])
            assert rc == ref_rc
            for name in STATE_ORDER:
                assert np.array_equal(ns.a[name], st[name][0]), (k, name)
    finally:
        ns.set_optional_terms(False, False)


@pytest.mark.parametrize("family", [0, 2])   # set_row_kernel: the unrolled and the rolled-loop register-resident kernels
@pytest.mark.parametrize("exact", [True, False])
def test_predicted_longest_first_dispatch(tinympc, oracle_mod, exact, family):
    """tiny_batch_set_dispatch(1): the predictor sweep and the bucket sort run ahead of the register-resident kernel for
    launches of >= 4096 groups (warm and cold workspaces, fp16 storage, a ragged last group) — results bitwise those of the
    index-order launch, and the exact ones those of the oracle on a sample."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 4 * 4096 + 3
    x0, table, start = pr.tracking_batch(B, 30, seed=9)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=40)
    for storage in (32, 16):
        res = []
        for mode in (0, 1):
            sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
            sol.select_kernel(2 if exact else 3)
            sol.set_storage(storage, storage)
            sol.set_row_kernel(family)
            sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.set_x0(x0)
            assert sol.kernel_name().startswith("rowloop" if family == 2 else "rowlane")
            sol.set_dispatch(mode)
            chain = []
            for k in range(3):      # cold, then two warm-started solves (the predictor reads d, y, g of the workspace)
                sol.solve()
                chain.append(sol.get_state())
                if k == 1:
                    sol.reset_dual_variables()
            res.append(chain)
            sol.close()
        for k in range(3):
            for name in STATE_ORDER + SCALARS:
                assert np.array_equal(res[0][k][name], res[1][k][name]), (storage, k, name)
        if storage == 16:
            # closed loop with the predicted order inside a replayed hipGraph (fp16 storage runs the unrolled kernel from a
            # graph; fp32 keeps the state on chip and never re-dispatches) against step-by-step launches in index order
            pair = []
            for mode in (1, 0):
                sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
                sol.select_kernel(2 if exact else 3)
                sol.set_storage(16, 16)
                sol.set_row_kernel(family)
                sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.set_x0(x0)
                sol.set_dispatch(mode)
                if mode:
                    sol.mpc_run_async(3, 1)
                else:
                    for _ in range(3):
                        sol.mpc_step_async(1)
                sol.synchronize()
                pair.append((sol.get_state(), sol.get_x0()))
                sol.close()
            for name in STATE_ORDER + SCALARS:
                assert np.array_equal(pair[0][0][name], pair[1][0][name]), ("closed loop", name)
            assert np.array_equal(pair[0][1], pair[1][1])
        if exact and storage == 32:
            idx = np.r_[np.arange(0, B, 97), B - 3, B - 2, B - 1]
            st = O.new_state(idx.size, 12, 4, 30); st["x"][:, 0] = x0[idx]
            O.Oracle(prob, np.float32, settings).solve(st, *pr.bounds_arrays(prob), pr.expand_windows(table, start[idx], 30), nthreads=8)
            assert_bitwise({k: res[1][0][k][idx] for k in STATE_ORDER + SCALARS}, st, "dispatch 1 vs oracle")


CLOSED_LOOP_CASES = [("hover", "row_exact"), ("hover", "loop_exact"), ("hover", "rowstream_exact"), ("hover", "tile_exact"),
                     ("track", "row_exact"), ("track", "loop_exact"), ("track", "rowstream_exact"), ("track", "tile_exact"),
                     ("cartpole", "row_exact"), ("cartpole", "lane_exact"), ("cartpole", "loop_exact"),
                     ("dims837", "row_exact"), ("dims837", "loop_exact")]


@pytest.mark.parametrize("name,variant_name", CLOSED_LOOP_CASES)
def test_device_closed_loop_equals_reference_trace(tinympc, oracle_mod, name, variant_name):
    """the device closed loop against the COMPILED REFERENCE's closed loop (tiny_solve + the examples' own
    Eigen plant step x1 = work.Adyn*x0 + work.Bdyn*work.u.col(0), quadrotor_hovering.cpp:90-114, quadrotor_tracking.cpp:93-118),
    recorded in tests/golden/closed_loop_traces.npz: 70 hovering steps, 110 tracking steps with sliding per-instance
    windows, 100 cartpole steps, 25 steps of the (8,3,7) class, 64 (20) instances each.  Exact arithmetic: u.col(0) of EVERY
    step, the iteration counts and statuses and the final plant state must be equal bit for bit — through
    tiny_batch_mpc_run_traj_async (on-chip loop for the unrolled row kernel and the quad kernel, hipGraph replay for the
    others) and through the step-by-step tiny_batch_mpc_step_async loop."""
    from helpers import GOLDEN, closed_loop_case
    O, pr = oracle_mod, tinympc.problems
    z = np.load(GOLDEN / "closed_loop_traces.npz")
    prob, x0, xref_fn, steps, settings, table, start = closed_loop_case(pr, O, z, name)
    B = x0.shape[0]
    adv = 1 if table is not None else 0

    def fresh():
        s = make_solver(tinympc, prob, B, settings, None, variant_name, pr.bounds_arrays(prob))
        if table is not None:
            s.set_xref_window(table, start)
        else:
            s.set_xref(xref_fn(0))
        s.set_x0(x0)
        return s
    a = fresh()
    kn = a.kernel_name()
    if name == "cartpole" and variant_name == "row_exact":
        assert kn.startswith("quadlane"), kn
    # (1) all steps in one call, split in two runs so that the continuation across calls is covered too
    k1 = steps // 3
    traj = np.concatenate([a.mpc_run_traj(k1, adv), a.mpc_run_traj(steps - k1, adv)])
    assert np.array_equal(traj, z[f"{name}_u0"]), f"{kn}: u.col(0) differs from the reference's closed loop at step " \
        f"{int(np.argmax(np.any(traj != z[name + '_u0'], axis=(1, 2))))}"
    assert np.array_equal(np.signbit(traj), np.signbit(z[f"{name}_u0"]))
    it, stt, _ = a.get_status()
    assert np.array_equal(it, z[f"{name}_iter"][-1]) and np.array_equal(stt, z[f"{name}_status"][-1])
    xf = a.get_x0()
    assert np.array_equal(xf, z[f"{name}_x_final"]) and np.array_equal(np.signbit(xf), np.signbit(z[f"{name}_x_final"])), kn
    a.close()
    # (2) step by step: iteration counts and statuses of every step
    b = fresh()
    for k in range(steps):
        b.mpc_step_async(adv)
        it, stt, _ = b.get_status()
        assert np.array_equal(it, z[f"{name}_iter"][k]) and np.array_equal(stt, z[f"{name}_status"][k]), (kn, k)
        assert np.array_equal(b.get_u()[:, 0], z[f"{name}_u0"][k]), (kn, k)
    assert np.array_equal(b.get_x0(), z[f"{name}_x_final"])
    b.close()


def test_mpc_run_replays_one_graph_while_only_buffer_contents_change(tinympc):
    """`set_xref; mpc_run(k)` in a loop must replay ONE captured hipGraph: the derived reference / bounds buffers keep their address while their
    size does not change (round-3 advisor: they used to be freed and re-allocated on every refill, so the replay depended on the allocator
    handing the same address back).  tiny_batch_debug_graph_captures counts the captures."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 17)   # a class whose closed loop runs from a graph (rolled-loop kernel)
    B = 33
    x0, table, start = pr.tracking_batch(B, 17, seed=2)
    rng = np.random.default_rng(0)
    sol = tinympc.TinyBatchSolver(prob, B)
    sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_x0(x0)
    caps = lambda: sol.lib.tiny_batch_debug_graph_captures(sol._h)
    for k in range(6):
        sol.set_xref((rng.standard_normal((B, 17, 12)) * 0.1).astype(np.float32))   # new CONTENTS, same shape
        if k == 3:
            sol.set_bounds(*[b * np.float32(0.9) for b in pr.bounds_arrays(prob)])   # same for the bounds table
        sol.mpc_run_async(3, 0); sol.synchronize()
        assert caps() == 1, (k, caps())
    sol.set_xref((rng.standard_normal((17, 12)) * 0.1).astype(np.float32))           # per-instance -> shared: another stride, another graph
    sol.mpc_run_async(3, 0); sol.synchronize()
    assert caps() == 2
    sol.close()


@pytest.mark.parametrize("variant_name", ["loop_exact", "rowstream_exact", "stream"])
def test_mpc_run_graph_is_rebuilt_when_its_arguments_change(tinympc, variant_name):
    """The hipGraph that tiny_batch_mpc_run_async replays carries rho, the bound flags and the reference strides as kernel
    ARGUMENTS: after set_cache (another rho), set_settings (bound flags) or a switch between a shared and a per-instance
    reference a replay of the old graph would silently use stale values.  Each change must give what a fresh handle,
    configured the same way and advanced step by step, gives."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B, K = 40, 4
    x0, table, start = pr.tracking_batch(B, 30, seed=13)
    bnds = pr.bounds_arrays(prob)
    xr_shared = np.tile(pr.HOVER_XREF, (30, 1)).astype(np.float32)
    xr_inst = pr.expand_windows(table, start, 30)
    # a cache for another rho: same gains, the solver only reads rho from it in the iteration (a self-consistent cache is
    # not needed for this test: both handles use the same numbers)
    prob2 = dict(prob, rho=prob["rho"] * 0.5)

    def configure(s, stage):
        s.set_xref(xr_shared if stage < 2 else xr_inst)          # stage 2: shared -> per-instance reference (strides)
        if stage >= 1:
            s.set_cache(prob2)                                    # stage 1: rho
        if stage >= 3:
            s.set_settings(**dict(s.settings, en_state_bound=0))  # stage 3: bound flag
    a = make_solver(tinympc, prob, B, None, xr_shared, variant_name, bnds)
    a.set_x0(x0)
    for stage in range(4):
        configure(a, stage)
        a.mpc_run_async(K, 0)
        b = make_solver(tinympc, prob, B, None, xr_shared, variant_name, bnds)
        configure(b, stage)
        b.set_x0(x0)
        # bring b to a's state before this stage's run, then advance it step by step
        if stage:
            b.set_state(prev_state); b.set_x0(prev_x0)
        for _ in range(K):
            b.mpc_step_async(0)
        sa, sb = a.get_state(), b.get_state()
        for k in STATE_ORDER + SCALARS:
            assert np.array_equal(sa[k], sb[k]), f"{a.kernel_name()} stage {stage}: {k}"
        assert np.array_equal(a.get_x0(), b.get_x0())
        prev_state, prev_x0 = sa, a.get_x0()
        b.close()
    a.close()


def test_negative_window_advance_is_refused(tinympc):
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    x0, table, start = pr.tracking_batch(8, 30, seed=1)
    s = tinympc.TinyBatchSolver(prob, 8)
    s.set_bounds(*pr.bounds_arrays(prob)); s.set_xref_window(table, start); s.set_x0(x0)
    with pytest.raises(tinympc.TinyBatchError):
        s.mpc_step_async(-1)
    with pytest.raises(tinympc.TinyBatchError):
        s.mpc_run_async(3, -2)
    s.mpc_step_async(1)   # the handle stays usable
    assert s.get_status()[0].min() >= 1
    s.close()


@pytest.mark.parametrize("B", [2048, 16384])
def test_config4_full_size_properties(tinympc, oracle_mod, B):
    """BASELINE.json configs[3] at its stated sizes — nx=32, nu=16, N=50, 16 384 instances on one GPU and the 2 048 one of
    eight GPUs receives (the bench.py --config random32 workload) — on the exact kernel that
    serves the class; the two sizes run the kernel's two instantiations (look-ahead 4 at <= 2 048 instances, look-ahead 1
    above).  Size-independent properties (duplicates, determinism, invariants, rollout consistency) plus a bitwise
    comparison with the oracle on a sample spread over the whole batch."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.random_system(32, 16, 50, seed=1234)
    nx, nu, N = 32, 16, 50
    bnds = pr.bounds_arrays(prob)
    x0, xref = pr.random_batch(B, nx, N)
    half = B // 2
    x0[half:] = x0[:half]
    sol = tinympc.TinyBatchSolver(prob, B)
    assert sol.kernel_name().endswith("exact>") and "32,16" in sol.kernel_name(), sol.kernel_name()
    sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
    rc = sol.solve()
    a = sol.get_state()
    for k in STATE_ORDER + SCALARS:                       # (1) duplicates agree wherever they sit
        assert np.array_equal(a[k][:half], a[k][half:]), k
    sol.reset_workspace(); sol.set_x0(x0); sol.solve()    # (2) determinism
    b = sol.get_state()
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(a[k], b[k]), k
    s = sol.settings                                      # (3) invariants
    solved = a["status"] == 1
    assert set(np.unique(a["status"])) <= {1, 11} and a["iter"].min() >= 1 and a["iter"].max() <= s["max_iter"]
    assert rc == (0 if solved.all() else 1) and 0.05 < solved.mean() < 1.0   # the workload has both kinds of instance
    assert np.all(a["residuals"][solved][:, :2] < s["abs_pri_tol"]) and np.all(a["residuals"][solved][:, 2:] < s["abs_dua_tol"])
    assert np.all(a["iter"][~solved] == s["max_iter"])
    assert a["znew"].max() <= prob["u_max"] and a["znew"].min() >= prob["u_min"]
    assert a["vnew"].max() <= prob["x_max"] and a["vnew"].min() >= prob["x_min"]
    assert np.array_equal(a["x"][:, 0], x0)
    assert np.array_equal(a["v"][~solved], a["vnew"][~solved]) and np.array_equal(a["z"][~solved], a["znew"][~solved])
    idx = np.arange(0, B, max(1, B // 256))
    xs, us = a["x"][idx].astype(np.float64), a["u"][idx].astype(np.float64)
    assert np.max(np.abs(xs[:, :-1] @ prob["Adyn"].T + us @ prob["Bdyn"].T - xs[:, 1:])) < 2e-4
    st = O.new_state(idx.size, nx, nu, N)                 # (4) sampled bitwise comparison with the oracle
    st["x"][:, 0] = x0[idx]
    O.Oracle(prob, np.float32, s).solve(st, *bnds, xref, nthreads=8)
    assert_bitwise({k: a[k][idx] for k in STATE_ORDER + SCALARS}, st, f"config 4, B={B}, {sol.kernel_name()}")
    sol.close()


def test_tile16_two_ended_tile_queue_solves_every_tile_exactly_once(tinympc, oracle_mod):
    """tiny_batch_set_tile_queue: every k-th wave of admm_tile16.hip claims its tiles from the short end of the dispatch order (one atomic word, head
    count in the low and tail count in the high half).  Whatever the stride — 1: every wave at the tail, 3: strides that do not divide the wave
    count, 255: a single tail wave — and whatever the launch (fewer tiles than waves, ragged last tile, predicted order and index order,
    shared tables and the per-instance-table instantiation) every instance must be solved exactly once: all work arrays, residuals, status and
    iteration counts bit for bit those of the single counter, and of the oracle on a sample.  The automatic choice must switch it on for the
    headline launch only (cold start, predicted order, >= 3 tiles per wave slot), which shows in nothing but the time."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 30)
    bnds = pr.bounds_arrays(prob)
    for B, per_instance in ((1, False), (17, False), (1000, True), (5000, False), (20000, False), (49152 + 5, False), (49152 + 5, True)):
        x0, table, start = pr.tracking_batch(B, 30, seed=B % 1000)
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.select_kernel(2); sol.set_row_kernel(5); sol.set_dispatch(1)
        if per_instance:   # every instance its own limits, constant along the horizon: the pi instantiation with resident rows
            rng = np.random.default_rng(B)
            scale = (1.0 + 0.2 * rng.random((B, 1, 1))).astype(np.float32)
            sol.set_bounds(*[(b[None] * scale).astype(np.float32) for b in bnds])
        else:
            sol.set_bounds(*bnds)
        sol.set_xref_window(table, start)
        assert sol.kernel_name() == ("tile16<12,4,30,exact,pi>" if per_instance else "tile16<12,4,30,exact>"), sol.kernel_name()
        ref = None
        for stride in (0, 1, 3, 8, 255, -1):
            sol.set_tile_queue(stride)
            sol.reset_workspace(); sol.set_x0(x0)
            rc = sol.solve()
            got = sol.get_state()
            assert (got["iter"] >= 1).all() and (got["status"] >= 0).all()
            if ref is None:
                ref, rc0 = got, rc
                continue
            assert rc == rc0
            assert_bitwise(got, ref, f"tile queue stride {stride} vs one counter, B={B}, per-instance bounds {per_instance}")
        if not per_instance:
            idx = np.unique(np.concatenate([np.arange(min(B, 40)), np.arange(max(B - 40, 0), B)]))
            st = O.new_state(len(idx), 12, 4, 30); st["x"][:, 0] = x0[idx]
            O.Oracle(prob, np.float32, O.DEFAULT_SETTINGS).solve(st, *bnds, pr.expand_windows(table, start, 30)[idx], nthreads=8)
            assert_bitwise({k: ref[k][idx] for k in STATE_ORDER + SCALARS}, st, f"tile queue, B={B} vs oracle")
        sol.close()
    with pytest.raises(Exception):
        sol = tinympc.TinyBatchSolver(prob, 16); sol.set_tile_queue(256)


@pytest.mark.parametrize("exact", [True, False])
def test_tile16_kernel_equals_row_kernel_bitwise(tinympc, oracle_mod, exact):
    """admm_tile16.hip (16 instances per wavefront as MFMA columns, set_row_kernel(5)) against the 16-lane row kernel on the
    same inputs: ragged batches around its 16-instance tile and 4-tile workgroup, cold and warm starts, sparse termination
    checks, one and zero iterations, bounds off, shared reference and window reference with clamping at the end of the
    table.  Both arithmetic modes must agree BIT FOR BIT with the row kernel (exact: K=1 MFMA products are separately
    rounded products; fma: v_mfma_f32_16x16x4_f32 is the same k-ascending fma chain as the row kernel's v_fmac_f32_dpp),
    and the exact mode with the oracle."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 30)
    bnds = pr.bounds_arrays(prob)
    for B, settings, warm, ref in ((1, {}, 1, "window"), (15, {}, 0, "shared"), (16, dict(max_iter=7), 0, "window"), (17, {}, 2, "window"),
                                   (63, dict(max_iter=40, check_termination=3), 1, "window"), (65, dict(max_iter=1), 0, "window"),
                                   (130, dict(max_iter=0), 0, "window"), (333, dict(max_iter=30, en_state_bound=0, en_input_bound=0), 1, "endclamp"),
                                   (3000, {}, 0, "window")):
        settings = dict(O.DEFAULT_SETTINGS, **settings)
        x0, table, start = pr.tracking_batch(B, 30, seed=B)
        if ref == "endclamp":
            start = np.minimum(start + 200, 301 - 30).astype(np.int32)
        outs = []
        for fam in (1, 5):
            sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
            sol.select_kernel(2 if exact else 3); sol.set_row_kernel(fam)
            sol.set_bounds(*bnds)
            if ref == "shared":
                sol.set_xref(np.tile(pr.HOVER_XREF, (30, 1)).astype(np.float32))
            else:
                sol.set_xref_window(table, start)
            assert sol.kernel_name().startswith("tile16<12,4,30" if fam == 5 else "rowlane<12,4,30"), sol.kernel_name()
            sol.set_x0(x0)
            rcs = [sol.solve()]
            for _ in range(warm):
                if ref != "shared":
                    sol.mpc_step_async(1)           # plant step + window slide + dual reset + solve (graph-free path)
                else:
                    sol.reset_dual_variables(); rcs.append(sol.solve())
            outs.append((rcs, sol.get_state(), sol.get_x0()))
            sol.close()
        (r1, a, xa), (r5, b, xb) = outs
        assert r1 == r5 and np.array_equal(xa, xb)
        assert_bitwise(b, a, f"tile16 vs rowlane, exact={exact}, B={B}, {settings}, warm={warm}, {ref}")
        if exact and warm == 0 and B <= 400:
            st = O.new_state(B, 12, 4, 30); st["x"][:, 0] = x0
            xr = np.tile(pr.HOVER_XREF, (30, 1)).astype(np.float32) if ref == "shared" else pr.expand_windows(table, start, 30)
            O.Oracle(prob, np.float32, settings).solve(st, *bnds, xr, nthreads=8)
            if settings["max_iter"] > 0:
                assert_bitwise(b, st, f"tile16 exact vs oracle, B={B}, {settings}")
    # a per-instance reference array is served by the `pi` instantiations since round 4 (test_tile16_per_instance_tables_bitwise)
    sol = tinympc.TinyBatchSolver(prob, 20)
    sol.set_row_kernel(5); sol.set_bounds(*bnds)
    x0, table, start = pr.tracking_batch(20, 30, seed=2)
    sol.set_xref(pr.expand_windows(table, start, 30))
    assert sol.kernel_name() == "tile16<12,4,30,exact,pi>", sol.kernel_name()
    sol.close()
    with pytest.raises(tinympc.TinyBatchError):
        s2 = tinympc.TinyBatchSolver(pr.cartpole(10), 4)
        try:
            s2.set_row_kernel(5)
        finally:
            s2.close()


@pytest.mark.parametrize("exact", [True, False])
def test_tile16_per_instance_tables_bitwise(tinympc, oracle_mod, exact):
    """The `pi` instantiations of admm_tile16.hip: box bounds and / or the reference PER INSTANCE (types.hpp:88-92 — every reference
    workspace owns its u_min .. x_max and its Xref), fetched by LDS-DMA into per-wave slots: ONE resident row per instance when the table
    does not change along the horizon ("const"), a ring of step slots fed from the table's tile image when it does ("steps").  Every
    combination — bounds const / steps with a shared / windowed / per-instance const / per-instance steps reference, shared bounds with a
    per-instance reference — on ragged batches around the tile of sixteen and the workgroup of four tiles, every compiled horizon, cold and
    warm starts, sparse checks, max_iter 1 / 2 (the deferred sweep of the epilogue) and bounds that bind hard: bit for bit the 16-lane
    row kernel in both arithmetic modes, and the oracle in exact arithmetic.  (Per-step bounds together with a trajectory table too long for
    the LDS share beside their ring keep the 16-lane kernel: checked by name.)"""
    O, pr = oracle_mod, tinympc.problems
    rng = np.random.default_rng(77)
    #        N   B     settings                               bounds    reference  warm
    cases = [(30, 1, {}, "steps", "steps", 0), (30, 17, dict(max_iter=9), "steps", "shared", 1), (30, 65, dict(max_iter=1), "const", "window", 0),
             (30, 130, dict(max_iter=2), "shared", "steps", 1), (30, 333, dict(max_iter=40, check_termination=3), "steps", "steps", 1),
             (30, 1000, dict(max_iter=30), "const", "endclamp", 2), (25, 70, dict(max_iter=25), "const", "steps", 1), (20, 47, dict(max_iter=30), "steps", "window", 2),
             (10, 260, dict(max_iter=60), "steps", "const", 1), (10, 16, dict(max_iter=3, en_state_bound=0), "const", "const", 0),
             (30, 200, dict(max_iter=25), "shared", "const", 1), (30, 77, dict(max_iter=12), "steps", "window", 0), (30, 4133, {}, "steps", "steps", 0)]
    for N, B, over, bmode, rmode, warm in cases:
        prob = pr.quadrotor(20, N)
        settings = dict(O.DEFAULT_SETTINGS, **over)
        shared = pr.bounds_arrays(prob)
        # per-instance bounds that bind: each instance scales the box by its own factor; "steps": some steps tighter still
        scale = rng.uniform(0.02, 1.0, size=(B, 1, 1)) * (rng.uniform(0.6, 1.0, size=(1, N, 1)) if bmode == "steps" else 1.0)
        scale = np.broadcast_to(scale, (B, N, 1))
        bnds = shared if bmode == "shared" else tuple((a[None] * scale[:, :a.shape[0]]).astype(np.float32) for a in shared)
        x0, table, start = pr.tracking_batch(B, N, seed=B)
        if rmode == "endclamp":
            start = np.minimum(start + 200, table.shape[0] - N).astype(np.int32)   # the window slides past the table's end in the warm steps: rows clamp
        xr_inst = (pr.expand_windows(table, start, N) + rng.standard_normal((B, N, 12)).astype(np.float32) * 0.05).astype(np.float32)
        if rmode == "const":
            xr_inst = np.repeat(xr_inst[:, :1], N, axis=1).copy()                  # every instance regulates to its own set point
        outs = []
        for fam in (1, 5):
            sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
            sol.select_kernel(2 if exact else 3); sol.set_row_kernel(fam)
            sol.set_bounds(*bnds)
            if rmode in ("steps", "const"):
                sol.set_xref(xr_inst)
            elif rmode == "shared":
                sol.set_xref(np.tile(pr.HOVER_XREF, (N, 1)).astype(np.float32))
            else:
                sol.set_xref_window(table, start)
            # at N = 30 the ring of per-step bounds (8 KB per step slot and CU, four slots) leaves 8 KB of LDS for a staged table: 128 rows — the 301-row
            # trajectory table does not fit (it does beside the 80 KB of slack of N = 20)
            too_long = bmode == "steps" and rmode in ("window", "endclamp") and N == 30
            want = f"rowlane<12,4,{N}" if fam == 1 or too_long else f"tile16<12,4,{N},{'exact' if exact else 'fast'},pi>"
            assert sol.kernel_name().startswith(want), (sol.kernel_name(), want, bmode, rmode)
            sol.set_x0(x0)
            rcs = [sol.solve()]
            for _ in range(warm):
                if rmode in ("window", "endclamp"):
                    sol.mpc_step_async(1)            # plant step + window slide + dual reset + solve, one launch per step
                else:
                    rcs.append(sol.solve())          # warm start from the live-in state, duals included
            outs.append((rcs, sol.get_state(), sol.get_x0()))
            sol.close()
        (r1, a, xa), (r5, b, xb) = outs
        what = f"tile16 pi vs rowlane, exact={exact}, N={N}, B={B}, {over}, bounds {bmode}, reference {rmode}, warm={warm}"
        assert r1 == r5 and np.array_equal(xa, xb), what
        assert_bitwise(b, a, what)
        if exact and warm == 0 and B <= 400:
            st = O.new_state(B, 12, 4, N); st["x"][:, 0] = x0
            xr = xr_inst if rmode in ("steps", "const") else np.tile(pr.HOVER_XREF, (N, 1)).astype(np.float32) if rmode == "shared" else pr.expand_windows(table, start, N)
            O.Oracle(prob, np.float32, settings).solve(st, *bnds, xr, nthreads=8)
            assert_bitwise(b, st, what + " (oracle)")
    # a closed-loop run on chip is instantiated for shared tables only: with per-instance bounds it keeps the 16-lane kernel, same bits (fuzz_mpc)
    prob = pr.quadrotor(20, 30)
    sol = tinympc.TinyBatchSolver(prob, 64)
    sol.set_row_kernel(5)
    sol.set_bounds(*[np.broadcast_to(b, (64,) + b.shape).copy() for b in pr.bounds_arrays(prob)])
    x0, table, start = pr.tracking_batch(64, 30, seed=3)
    sol.set_xref_window(table, start); sol.set_x0(x0)
    assert sol.kernel_name() == "tile16<12,4,30,exact,pi>", sol.kernel_name()
    sol.mpc_run_async(3, 1); sol.wait()
    assert sol.closed_loop_kernel_name().startswith("rowlane<12,4,30"), sol.closed_loop_kernel_name()
    sol.close()


@pytest.mark.parametrize("dual_bits", [16, 32])
def test_config5_fp16_storage_against_the_fp32_reference(tinympc, oracle_mod, dual_bits):
    """BASELINE.json configs[4] as stated: a mixed batch (cartpole + quadrotor tracking) in one tiny_batch_group_solve call
    with fp16 storage and fp32 arithmetic / residual accumulation, held against the PINNED fp32 oracle (== the compiled
    reference) — not against the _h16 restatement, which the reference has no counterpart for.  SURVEY.md §8(d) asks for a
    stated looser tolerance and the iteration-count drift; the bars below are the measured figures of DESIGN.md §6 with a
    margin, in the units a user cares about:
      * u.col(0) of instances that reach the tolerance in both precisions, relative to the input bound:
        quadrotor <= 2e-2 (measured 9.4e-3), cartpole <= 5e-3 (8.3e-4): binary16 resolves 2^-11 of a value and the roll-out
        passes 29 rounded steps;
      * converged fraction: quadrotor >= 0.88 (measured 0.916; fp32 1.00), cartpole >= 0.65 (0.726; fp32 0.974) — binary16's
        resolution near |x| ~ 1-2 (1e-3 .. 2e-3) is coarser than the 1e-3 residual tolerance, so some instances stall above it;
      * iteration-count drift of the instances that converge in both precisions: the count changes for 99.8 % of the
        quadrotor and 25 % of the cartpole instances; mean drift -8.7 / -1.7 iterations (the coarser slack reaches the
        tolerance earlier); bars |mean drift| <= 12 / <= 4.
    dual_bits = 32 (tiny_batch_set_storage_ex(16, 32), the duals kept in fp32): the stall caused by dual increments lost
    below an fp16 ulp goes away — cartpole converges 0.982 (above fp32's 0.974), bar >= 0.95; the quadrotor's remaining
    stall is the PRIMAL quantisation (rho x one fp16 ulp of v > abs_dua_tol): 0.934, bar >= 0.90.  Same u0 bars."""
    O, pr = oracle_mod, tinympc.problems
    B = 8192
    cases = []
    cp = pr.cartpole(10)
    rng = np.random.default_rng(1)
    x0c = (np.array([[0, 0, 0.1, 0]], np.float32) + rng.uniform(-0.05, 0.05, size=(B, 4))).astype(np.float32)
    cases.append(("cartpole", cp, x0c, np.zeros((10, 4), np.float32), dict(O.DEFAULT_SETTINGS, max_iter=150), None, 5e-3,
                  0.65 if dual_bits == 16 else 0.95, 4.0))
    qd = pr.quadrotor(20, 30)
    x0q, table, start = pr.tracking_batch(B, 30)
    cases.append(("quadrotor", qd, x0q, pr.expand_windows(table, start, 30), dict(O.DEFAULT_SETTINGS), (table, start), 2e-2, 0.88 if dual_bits == 16 else 0.90, 12.0))
    sols = []
    for name, prob, x0, xref, settings, window, _, _, _ in cases:
        sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
        sol.set_storage(16, dual_bits)
        sol.set_bounds(*pr.bounds_arrays(prob))
        if window is not None:
            sol.set_xref_window(*window)
        else:
            sol.set_xref(xref)
        sol.set_x0(x0)
        sols.append(sol)
    tinympc.solve_group(sols)
    report = {}
    for (name, prob, x0, xref, settings, window, u_bar, conv_bar, _), sol in zip(cases, sols):
        nx, nu, N = prob["nx"], prob["nu"], prob["N"]
        got = sol.get_state()
        assert sol.kernel_name().endswith(",h16>" if dual_bits == 16 else ",h16d>"), sol.kernel_name()
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
        O.Oracle(prob, np.float32, settings).solve(st, *pr.bounds_arrays(prob), xref, nthreads=8)   # the pinned fp32 reference
        both = (got["status"] == 1) & (st["status"] == 1)
        ub = max(abs(prob["u_max"]), abs(prob["u_min"]))
        err = np.abs(got["u"][both, 0].astype(np.float64) - st["u"][both, 0]).max(axis=1) / ub
        drift = (got["iter"][both].astype(np.int64) - st["iter"][both])
        # instances the fp16 run does NOT bring to the tolerance (they stop at max_iter): what a caller gets if it applies their
        # u.col(0) anyway, against the fp32 reference's converged control (round 3: reported and bounded, not only the rest)
        stalled = (got["status"] != 1) & (st["status"] == 1)
        err_st = (np.abs(got["u"][stalled, 0].astype(np.float64) - st["u"][stalled, 0]).max(axis=1) / ub) if stalled.any() else np.zeros(1)
        report[name] = dict(conv_h16=float((got["status"] == 1).mean()), conv_f32=float((st["status"] == 1).mean()),
                            u0_err_unconverged_max=float(err_st.max()), u0_err_unconverged_p99=float(np.percentile(err_st, 99)),
                            frac_unconverged=float(stalled.mean()),
                            u0_err_max=float(err.max()), u0_err_p99=float(np.percentile(err, 99)), changed=float((drift != 0).mean()),
                            mean_drift=float(drift.mean()), mean_iter_h16=float(got["iter"].mean()), mean_iter_f32=float(st["iter"].mean()))
        sol.close()
    print(f"config 5 (fp16 storage, {dual_bits}-bit duals, vs fp32 reference):", report)
    for (name, _, _, _, _, _, u_bar, conv_bar, drift_bar) in cases:
        r = report[name]
        assert r["conv_h16"] >= conv_bar, (name, r)
        assert r["u0_err_max"] <= u_bar, (name, r)
        assert abs(r["mean_drift"]) <= drift_bar, (name, r)
        # unconverged fp16 instances carry a u.col(0) that can be far off (measured r02: up to 0.67 of the input bound for the
        # cartpole with 16-bit duals): the status flag, not the control, is what a caller must look at.  With fp32 duals the
        # stalled quadrotor instances sit within an fp16 ulp of the answer (measured 1.4e-2 of the input bound; bounded here at 5 %);
        # a stalled cartpole instance (1.7 % of the batch) can still be 0.7 of the bound off: reported, not bounded.
        if dual_bits == 32 and name == "quadrotor":
            assert r["u0_err_unconverged_max"] <= 5e-2, (name, r)


def test_default_16_bit_storage_keeps_the_duals_in_fp32_where_a_register_resident_kernel_exists(tinympc):
    """tiny_batch_set_storage(tb, 16) (no dual precision given): fp32 duals on the classes with an unrolled / quad kernel, 16-bit
    duals where only the kernels that stream or roll their state exist; _ex(16, 16) forces binary16 everywhere."""
    pr = tinympc.problems
    for prob, want in ((pr.quadrotor(20, 30), ",h16d>"), (pr.cartpole(10), ",h16d>"), (pr.quadrotor(20, 17), ",h16>")):
        sol = tinympc.TinyBatchSolver(prob, 64)
        sol.set_storage(16)
        sol.set_bounds(*pr.bounds_arrays(prob))
        assert sol.kernel_name().endswith(want), sol.kernel_name()
        sol.set_storage(16, 16)
        assert sol.kernel_name().endswith(",h16>"), sol.kernel_name()
        sol.close()


def test_debug_guard_zones_stay_intact(tinympc):
    """SURVEY.md section 5 asks for a debug bounds-checked variant (there is no GPU address sanitizer on this platform).  Under
    tiny_batch_debug_guards(1) every device allocation of the library carries NaN guard zones; this sweep drives EVERY kernel family
    (unrolled / rolled / streaming row kernels, quad, tile16 incl. its on-chip closed loop, wave kernels, tile48, MFMA streaming, the
    run-time-dimension kernel, the six step functions, fp16 storage, per-instance bounds, optional terms, pack / unpack / plant / predictor
    helpers) over ragged batch sizes and then asks the library how many guard words were overwritten: none, and no result is NaN (an
    out-of-bounds read would return the guard pattern).  The checker itself is tested with a deliberate out-of-bounds write."""
    pr = tinympc.problems
    tinympc.debug_guards(True)
    try:
        assert tinympc.debug_check() == 0
        rng = np.random.default_rng(11)
        runs = []   # (problem, batch, variant, family, extra)
        q30, q17, q77, cp, r32, odd, gen = pr.quadrotor(20, 30), pr.quadrotor(20, 17), pr.quadrotor(20, 77), pr.cartpole(10), \
            pr.random_system(32, 16, 50, seed=1234), pr.random_system(8, 3, 7, seed=99), pr.random_system(20, 12, 12, seed=2012)
        for B in (1, 17, 203):
            runs += [(q30, B, 2, 1, {}), (q30, B, 3, 1, {}), (q30, B, 2, 2, {}), (q30, B, 2, 3, {}), (q30, B, 2, 5, {}), (q30, B, 3, 5, {}), (q30, B, 1, 0, {}),
                     (q30, B, 2, 1, dict(per_instance_bounds=True)), (q30, B, 2, 0, dict(storage=16)), (q30, B, 2, 1, dict(optional=True)),
                     # the pi instantiations of tile16 (LDS-DMA slots and rings, tile images): resident bounds row + reference ring; both rings, cold and warm
                     (q30, B, 2, 5, dict(per_instance_bounds=True)), (q30, B, 3, 5, dict(per_instance_bounds=True, per_step=True)),
                     (q17, B, 2, 0, {}), (q77, B, 2, 0, {}), (cp, B, 2, 0, {}), (cp, B, 2, 1, {}), (odd, B, 2, 0, {}),
                     (r32, B, 2, 6, {}), (r32, B, 2, 7, {}), (r32, B, 2, 8, {}), (r32, B, 3, 8, {}), (r32, B, 1, 0, {}), (gen, B, 0, 0, {}), (q30, B, 4, 0, {})]
        names = set()
        for prob, B, variant, family, extra in runs:
            nx, nu, N = prob["nx"], prob["nu"], prob["N"]
            sol = tinympc.TinyBatchSolver(prob, B, settings=dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=7, check_termination=2, en_state_bound=1, en_input_bound=1))
            if extra.get("storage"):
                sol.set_storage(extra["storage"])
            sol.select_kernel(variant)
            if family:
                sol.set_row_kernel(family)
            bnds = pr.bounds_arrays(prob)
            if extra.get("per_instance_bounds"):
                bnds = tuple(np.broadcast_to(a, (B,) + a.shape).copy() for a in bnds)
                if extra.get("per_step"):
                    bnds[1][:, N // 2] *= 0.9
            sol.set_bounds(*bnds)
            table = (rng.standard_normal((N + 9, nx)) * 0.1).astype(np.float32)
            start = rng.integers(0, 9, size=B).astype(np.int32)
            if nx <= 16 and not extra.get("per_instance_bounds"):
                sol.set_xref_window(table, start)
            else:
                sol.set_xref(pr.expand_windows(table, start, N))
            if extra.get("optional"):
                sol.set_input_cost(prob["R"]); sol.set_coeff_d2p(np.zeros((nx, nu), np.float32) + 0.01); sol.set_uref(np.zeros((N - 1, nu), np.float32) + 0.02)
                sol.set_optional_terms(True, True)
            sol.set_x0(rng.uniform(-0.2, 0.2, size=(B, nx)).astype(np.float32))
            sol.set_dispatch(1)
            sol.solve(); sol.reset_dual_variables(); sol.solve(); sol.reset_workspace(); sol.set_x0(np.zeros((B, nx), np.float32) + 0.05); sol.solve()
            names.add(sol.kernel_name())
            if nx + nu <= 16 and variant in (2, 3) and not extra.get("optional"):
                sol.mpc_run_async(3, 1 if nx <= 16 else 0); sol.synchronize()
                if not extra.get("storage"):
                    for fn in ("forward_pass", "update_slack", "update_dual", "update_linear_cost", "backward_pass_grad"):
                        getattr(sol, fn)()
            st = sol.get_state()
            assert all(np.all(np.isfinite(st[k])) for k in STATE_ORDER), (sol.kernel_name(), B, "a NaN: an out-of-bounds read?")
            assert tinympc.debug_check() == 0, (sol.kernel_name(), B, extra)
            sol.close()
        families = {n.split("<")[0] for n in names}
        assert {"rowlane", "rowloop", "rowstream", "quadlane", "tile16", "wavestream", "waveres", "tile48", "stream", "generic"} <= families, families
        assert {"tile16<12,4,30,exact,pi>", "tile16<12,4,30,fast,pi>"} <= names, names
        # the checker itself: one word written just outside a work array must be counted
        sol = tinympc.TinyBatchSolver(q30, 5)
        for which in (0, 1):
            sol._check(sol.lib.tiny_batch_debug_poke(sol._h, which))
            assert tinympc.debug_check() == which + 1
        sol.close()
        assert tinympc.debug_check() == 0   # the damaged allocation is gone with its handle
    finally:
        tinympc.debug_guards(False)


GENERIC_DIMS = [(20, 12, 12), (3, 2, 6), (8, 8, 6), (4, 3, 9), (36, 4, 5), (28, 16, 6)]


@pytest.mark.parametrize("dims", GENERIC_DIMS)
def test_generic_exact_kernel_bitwise_vs_compiled_reference(tinympc, oracle_mod, dims):
    """Round 4 (review: "bitwise arithmetic outside the compiled class lists"): a class with no compiled exact kernel but with dimensions the
    reference's orders are defined for (nx, nu each <= 4 or a multiple of 4, nx <= 36) is solved in EXACT arithmetic by the
    run-time-dimension kernel (admm_generic.hip) — the automatic choice, no rebuild — bit for bit what the reference COMPILED FOR THAT CLASS
    computes (oracle/_ref, built by oracle/Makefile; the oracle where the GPU box has no such build): warm states with signed zeros,
    four settings, shared and per-instance bounds, shared / per-instance / windowed references, cold starts, chains of solves."""
    O, pr = oracle_mod, tinympc.problems
    nx, nu, N = dims
    prob = pr.random_system(nx, nu, N, seed=nx * 100 + nu)
    Ref = O.Reference if O.have_ref(np.float32, nx, nu, N) else O.Oracle
    rng = np.random.default_rng(nx + nu + N)
    B = 37
    st0 = O.new_state(B, nx, nu, N)
    for k in STATE_ORDER:
        st0[k][:] = (rng.standard_normal(st0[k].shape) * 0.3).astype(np.float32)
    for k in ("x", "d", "v", "z", "g", "y"):
        st0[k][rng.random(st0[k].shape) < 0.1] = 0.0
        st0[k][rng.random(st0[k].shape) < 0.1] = -0.0
    st0["x"][0, 0] = -0.0; st0["g"][0] = 0.0; st0["y"][0] = 0.0; st0["d"][0] = 0.0
    shared = pr.bounds_arrays(prob)
    per_inst = tuple((a[None] * rng.uniform(0.3, 1.0, size=(B,) + a.shape)).astype(np.float32) for a in shared)
    table = (rng.standard_normal((N + 20, nx)) * 0.2).astype(np.float32)
    start = rng.integers(0, 20, size=B).astype(np.int32)
    refs = {"shared": (rng.standard_normal((N, nx)) * 0.2).astype(np.float32), "per_instance": (rng.standard_normal((B, N, nx)) * 0.2).astype(np.float32),
            "window": None}
    cases = [(dict(max_iter=1, abs_pri_tol=0, abs_dua_tol=0), shared, "per_instance"), (dict(max_iter=12, abs_pri_tol=0, abs_dua_tol=0), per_inst, "shared"),
             (dict(max_iter=60, check_termination=3), shared, "window"), (dict(max_iter=5, en_state_bound=0, en_input_bound=0), per_inst, "per_instance")]
    for extra, bnds, refmode in cases:
        settings = dict(O.DEFAULT_SETTINGS, **extra)
        sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
        assert sol.kernel_name() == f"generic<{nx},{nu},exact>" and sol.arithmetic() == "exact", sol.kernel_name()
        sol.set_bounds(*bnds)
        if refmode == "window":
            sol.set_xref_window(table, start); xref = pr.expand_windows(table, start, N)
        else:
            xref = refs[refmode]; sol.set_xref(xref)
        st = O.copy_state(st0)
        sol.set_state(st)
        ref = Ref(prob, np.float32, settings)
        for k in range(3):   # a warm solve, then two with the duals reset
            if k:
                st["y"][:] = 0; st["g"][:] = 0; sol.reset_dual_variables()
            rc_ref = ref.solve(st, *bnds, xref)
            rc = sol.solve()
            assert (rc != 0) == (rc_ref != 0)
            assert_bitwise(sol.get_state(), st, f"generic {dims} {extra} k={k}")
        # a cold start (reset_workspace folded into the launch)
        x0 = rng.uniform(-0.5, 0.5, size=(B, nx)).astype(np.float32)
        sol.reset_workspace(); sol.set_x0(x0)
        st = O.new_state(B, nx, nu, N); st["x"][:, 0] = x0
        ref.solve(st, *bnds, xref); sol.solve()
        assert_bitwise(sol.get_state(), st, f"generic {dims} {extra} cold")
        sol.close()
    # the same kernel on a COMPILED class, on request (variant 4), equals that class's own exact kernel
    if dims == GENERIC_DIMS[0]:
        q = pr.quadrotor(20, 10)
        x0, tb_, s_ = pr.tracking_batch(64, 10, seed=3)
        outs = []
        for variant in (0, 4):
            sol = tinympc.TinyBatchSolver(q, 64)
            sol.select_kernel(variant)
            sol.set_bounds(*pr.bounds_arrays(q)); sol.set_xref_window(tb_, s_); sol.set_x0(x0)
            sol.solve(); sol.reset_dual_variables(); sol.solve()
            outs.append((sol.kernel_name(), sol.get_state())); sol.close()
        assert outs[1][0] == "generic<12,4,exact>" and outs[0][0].startswith("rowlane<12,4,10,exact")
        assert_bitwise(outs[1][1], outs[0][1], "generic vs rowlane on the quadrotor class")


def test_arithmetic_mode_is_reported_by_the_library(tinympc):
    """tiny_batch_arithmetic(): "exact" for every automatic choice (each BASELINE class), "fma" only after the caller selected an fma variant."""
    pr = tinympc.problems
    for prob, B in ((pr.quadrotor(20, 30), 64), (pr.quadrotor(20, 30), 40000), (pr.cartpole(10), 64), (pr.random_system(32, 16, 50, seed=1234), 64),
                    (pr.random_system(32, 16, 50, seed=1234), 4096), (pr.quadrotor(20, 77), 8)):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.set_bounds(*pr.bounds_arrays(prob))
        assert sol.arithmetic() == "exact" and sol.kernel_name().split(",")[-1].startswith("exact"), sol.kernel_name()
        sol.select_kernel(3)
        assert sol.arithmetic() == "fma", sol.kernel_name()
        sol.select_kernel(0)
        assert sol.arithmetic() == "exact"
        sol.close()


def test_default_16_bit_storage_is_a_preference_not_a_refusal(tinympc, oracle_mod):
    """tiny_batch_set_storage(tb, 16) asks for fp32 duals where the kernel keeps them and must not make anything fail that the 16-bit
    mode could do (round-3 advisor finding): per-instance bounds, the Uref term, a forced rolled kernel and the single-function calls
    resolve to kernels with binary16 duals — the duals pair is converted and the result is the `_h16` oracle's, bit for bit; a later
    call that resolves to the register-resident kernel gets fp32 duals back (`_h16d` oracle); an explicit (16, 32) stays a requirement."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 30)
    nx, nu, N, B = 12, 4, 30, 37
    rng = np.random.default_rng(5)
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.1).astype(np.float32)
    shared = pr.bounds_arrays(prob)
    per_inst = tuple(np.broadcast_to(a, (B,) + a.shape).copy() for a in shared)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=40)
    xref_h, x0_h = O.round_h16(xref), O.round_h16(x0)

    def oracle_solve(kind, bnds, n=2):
        st = O.new_state(B, nx, nu, N)
        st["x"][:, 0] = x0_h
        orc = O.Oracle(prob, kind, settings)
        for _ in range(n):
            st["y"][:] = 0; st["g"][:] = 0
            orc.solve(st, *tuple(O.round_h16(b) for b in bnds), xref_h, nthreads=8)
        return st

    # (a) per-instance bounds under fp16 storage: the streaming row kernel, binary16 duals
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.set_storage(16)
    sol.set_bounds(*shared); sol.set_xref(xref); sol.set_x0(x0)
    assert sol.kernel_name() == "rowlane<12,4,30,exact,h16d>", sol.kernel_name()
    sol.set_bounds(*per_inst)
    assert sol.kernel_name().endswith(",h16>") and not sol.kernel_name().startswith("rowlane"), sol.kernel_name()
    for _ in range(2):
        sol.reset_dual_variables(); sol.solve()
    assert_bitwise(sol.get_state(), oracle_solve("h16", shared), "set_storage(16) + per-instance bounds")
    # (b) back to shared bounds: the register-resident kernel, fp32 duals again (the state carries over, converted)
    sol.set_bounds(*shared)
    assert sol.kernel_name() == "rowlane<12,4,30,exact,h16d>", sol.kernel_name()
    sol.reset_workspace(); sol.set_x0(x0)
    for _ in range(2):
        sol.reset_dual_variables(); sol.solve()
    assert_bitwise(sol.get_state(), oracle_solve("h16d", shared), "set_storage(16), shared bounds again")
    # (c) a forced rolled kernel and (d) a single-function call
    sol.set_row_kernel(2)
    assert sol.kernel_name() == "rowloop<12,4,exact,h16>", sol.kernel_name()
    sol.reset_workspace(); sol.set_x0(x0)
    for _ in range(2):
        sol.reset_dual_variables(); sol.solve()
    want = oracle_solve("h16", shared)
    assert_bitwise(sol.get_state(), want, "set_storage(16) + forced rowloop")
    sol.set_row_kernel(0)
    sol.forward_pass()  # the single-function kernels store binary16 duals: converted, not refused
    orc = O.Oracle(prob, "h16", settings)
    orc.step("forward_pass", want, *tuple(O.round_h16(b) for b in shared), xref_h)
    got = sol.get_state()
    for name in ("x", "u", "y", "g"):
        assert got[name].tobytes() == want[name].tobytes(), name
    sol.close()
    # (e) the Uref term
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.set_storage(16)
    sol.set_bounds(*shared); sol.set_xref(xref); sol.set_x0(x0)
    uref = (rng.standard_normal((B, N - 1, nu)) * 0.05).astype(np.float32)
    sol.set_input_cost(prob["R"]); sol.set_uref(uref); sol.set_optional_terms(True, False)
    assert sol.kernel_name() == "rowstream<12,4,exact,h16>", sol.kernel_name()
    sol.reset_dual_variables(); assert sol.solve() in (0, 1)
    sol.close()
    # (f) an explicit (16, 32) is still a requirement
    sol = tinympc.TinyBatchSolver(prob, B, settings=settings)
    sol.set_storage(16, 32)
    sol.set_bounds(*per_inst); sol.set_xref(xref); sol.set_x0(x0)
    with pytest.raises(tinympc.TinyBatchError):
        sol.solve()
    sol.close()


def test_per_instance_bounds_stay_on_the_register_resident_kernel_and_cost_little(tinympc):
    """The headline workload with every instance owning its bounds (the same values, so the iterates are identical).  Round 4: the
    automatic choice stays on the sixteen-instances-per-wave kernel (`tile16<…,pi>`: the rows arrive by LDS-DMA); the
    16-lane kernel (`rowlane<…>` with its BPI instantiation, set_row_kernel(1)) stays within 25 % of its own shared-bounds run.  All four
    runs return the same bits, and the automatic choice must be the faster of the two per-instance kernels."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 65536
    x0, table, start = pr.tracking_batch(B, 30)
    shared = pr.bounds_arrays(prob)
    res = {}
    for mode, fam, want in (("shared", 0, "tile16<12,4,30,exact>"), ("shared", 1, "rowlane<12,4,30,exact>"),
                            ("per_instance", 0, "tile16<12,4,30,exact,pi>"), ("per_instance", 1, "rowlane<12,4,30,exact>")):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.set_bounds(*(shared if mode == "shared" else tuple(np.broadcast_to(a, (B,) + a.shape).copy() for a in shared)))
        sol.set_xref_window(table, start)
        sol.set_row_kernel(fam)
        assert sol.kernel_name() == want, (mode, fam, sol.kernel_name())
        sol.enable_timing(True)
        ms = []
        for r in range(6):
            sol.reset_workspace(); sol.set_x0(x0); sol.solve_async(); sol.synchronize()
            if r >= 2:
                ms.append(sol.last_solve_ms())
        res[(mode, fam)] = (float(np.median(ms)), sol.get_u(), sol.get_status()[0])
        sol.close()
    print("kernel ms (shared tile16, shared rowlane, per-instance tile16 pi, per-instance rowlane):", [round(res[k][0], 3) for k in res])
    ref = res[("shared", 1)]
    for k, v in res.items():
        assert np.array_equal(ref[1], v[1]) and np.array_equal(ref[2], v[2]), k
    assert res[("per_instance", 1)][0] <= 1.25 * res[("shared", 1)][0], res
    assert res[("per_instance", 0)][0] <= 1.02 * res[("per_instance", 1)][0], res   # why the automatic choice is what it is


# ---------------------------------------------------------------------------------------------------------------------
# tinytype = double (the reference as shipped, glob_opts.hpp:3): include/tinympc_batch64.h
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2])
def test_fp64_as_shipped_hovering_loop_and_golden_vectors(tinympc, oracle_mod, kernel):
    """The reference exactly as checked in — typedef double tinytype, NSTATES 12, NINPUTS 4, NHORIZON 10 (glob_opts.hpp:3-7),
    examples/quadrotor_hovering.cpp — through the fp64 library: the recorded solves (k = 0 and k = 69) reproduce all twelve
    work arrays, residuals, status and iter of the compiled reference bit for bit, and the whole 70-step closed loop reproduces
    its controls and iteration counts (SURVEY.md §4 KATs: 1269 iterations, u0 = 0.488778532 ...).  Both kernels: one thread
    per instance with the state in HBM (1), sixteen lanes per instance with the state in registers (2, the default here)."""
    O = oracle_mod
    meta, prob, solves, z = load_fixture("quad_hover_f64_N10")
    assert meta["dtype"] == "float64" and prob["N"] == 10
    bnds = bounds_of(prob, np.float64)
    for s in solves:
        sol = tinympc.TinyBatchSolver64(prob, 1, settings=s["settings"])
        assert sol.kernel_name() == "rows64<12,4,10>", sol.kernel_name()   # the automatic choice
        sol.select_kernel(kernel)
        assert sol.kernel_name() == ("thread64<12,4>" if kernel == 1 else "rows64<12,4,10>")
        sol.set_bounds(*bnds); sol.set_xref(s["xref"])
        sol.set_state(s["pre"])
        rc = sol.solve()
        assert rc == (1 if s["rc"] else 0)
        assert_bitwise(sol.get_state(), s["post"], f"fp64 golden solve k={s['k']}")
        sol.close()
    sol = tinympc.TinyBatchSolver64(prob, 1, settings=solves[0]["settings"])
    sol.select_kernel(kernel)
    sol.set_bounds(*bnds); sol.set_xref(solves[0]["xref"])
    sol.set_state(solves[0]["pre"])
    orc = O.Oracle(prob, np.float64)
    x0 = solves[0]["pre"]["x"][:, 0].copy()
    iters, u0s = [], []
    for k in range(70):
        sol.set_x0(x0)                       # hovering.cpp:95
        sol.reset_dual_variables()           # :100-101
        sol.solve()                          # :104
        u0 = sol.get_u()[:, 0]
        iters.append(int(sol.get_status()[0][0])); u0s.append(u0[0].copy())
        x0 = orc.plant_step(x0, u0)          # :110-111 in the examples' own order (pinned in tests/test_oracle.py)
    assert np.array_equal(np.array(iters), z["trace_iter"]) and np.array_equal(np.array(u0s), z["trace_u0"])
    assert sum(iters) == 1269 and iters[0] == 100 and iters[69] == 2
    np.testing.assert_allclose(u0s[0], [0.488778532, 0.478938215, 0.542743696, 0.551056731], rtol=0, atol=5e-10)
    # the same loop with the plant update on the device (tiny_batch64_mpc_step): identical trace, identical next x0
    sol.set_state(solves[0]["pre"])
    it2, u2 = [], []
    for k in range(70):
        sol.mpc_step()
        xk, uk = sol.first_columns()
        it2.append(int(sol.get_status()[0][0])); u2.append(uk[0].copy())
    assert np.array_equal(np.array(it2), z["trace_iter"]) and np.array_equal(np.array(u2), z["trace_u0"])
    assert np.array_equal(xk, np.reshape(x0, xk.shape)) and np.array_equal(np.signbit(xk), np.signbit(np.reshape(x0, xk.shape)))
    sol.close()


@pytest.mark.parametrize("case", ["quad10", "cartpole", "r8_4"])
def test_fp64_step_functions_batched_and_native(tinympc, oracle_mod, case):
    """The six step functions in double: over a batch (tiny_batch64_forward_pass ...) and under the reference's own names over a
    caller-owned TinySolver with double members (libtinympc_wrapper64.so: the reference as checked in).  Each call leaves the
    workspace exactly as the fp64 oracle's restatement of the same reference function; tiny_solve from a random warm state too."""
    from accelerated_tinympc_amd import native
    O, pr = oracle_mod, tinympc.problems
    prob = {"quad10": lambda: pr.quadrotor(20, 10), "cartpole": lambda: pr.cartpole(10, riccati=O.riccati),
            "r8_4": lambda: pr.random_system(8, 4, 9, seed=804, riccati=O.riccati)}[case]()
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    B = 70
    rng = np.random.default_rng(21)
    bnds = tuple(np.asarray(a, np.float64) * s for a, s in zip(pr.bounds_arrays(prob, np.float64), (0.2, 0.2, 1.0, 1.0)))
    settings = dict(O.DEFAULT_SETTINGS, check_termination=2, abs_pri_tol=0.5, abs_dua_tol=5.0)
    st = O.new_state(B, nx, nu, N, np.float64)
    for k in STATE_ORDER:
        st[k][:] = rng.standard_normal(st[k].shape) * 0.3
    st["iter"][:] = 4; st["status"][:] = 11
    st["iter"][::3] = 5   # odd: termination_condition must skip these (iter % check_termination != 0)
    st["residuals"][:] = rng.uniform(0, 1, size=(B, 4))
    xref = rng.standard_normal((B, N, nx)) * 0.3
    orc = O.Oracle(prob, np.float64, settings)
    sol = tinympc.TinyBatchSolver64(prob, B, settings=settings)
    sol.set_bounds(*bnds); sol.set_xref(xref)
    ns = native.NativeSolver(prob, settings, dtype=np.float64)
    for k, arr in zip(("x_min", "x_max", "u_min", "u_max"), bnds):
        ns.a[k][:] = arr
    ns.a["Xref"][:] = xref[0]

    def load_native(state):
        for k in STATE_ORDER:
            ns.a[k][:] = state[k][0]
        w = ns.work
        (w.primal_residual_state, w.primal_residual_input, w.dual_residual_state, w.dual_residual_input) = map(float, state["residuals"][0])
        w.iter, w.status = int(state["iter"][0]), int(state["status"][0])

    for fn in O.Oracle.STEP_FUNCTIONS:
        sol.set_state(st); load_native(st)
        ref_rv = orc.step(fn, st, *bnds, xref)
        rv = getattr(sol, fn)()
        rvn = ns.call(fn)
        got = sol.get_state()
        if fn == "termination_condition":
            assert np.array_equal(rv, ref_rv) and bool(rvn) == bool(ref_rv[0])
        for k in STATE_ORDER + ("residuals",):
            assert np.array_equal(got[k], st[k]) and np.array_equal(np.signbit(got[k]), np.signbit(st[k])), f"batched {fn}: {k}"
        for k in STATE_ORDER:
            assert np.array_equal(ns.a[k], st[k][0]), f"native {fn}: {k}"
        assert np.array_equal(ns.residuals, st["residuals"][0]) and ns.work.iter == st["iter"][0] and ns.work.status == st["status"][0], fn
    for max_iter in (3, 200):
        settings2 = dict(settings, max_iter=max_iter, check_termination=1, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
        ns.settings.max_iter, ns.settings.check_termination = max_iter, 1
        ns.settings.abs_pri_tol = ns.settings.abs_dua_tol = 1e-3
        st2 = O.copy_state(st)
        load_native(st2)
        O.Oracle(prob, np.float64, settings2).solve(st2, *bnds, xref)
        rc = ns.tiny_solve()
        assert rc == (1 if st2["status"][0] == 11 else 0)
        for k in STATE_ORDER:
            assert np.array_equal(ns.a[k], st2[k][0]), f"native tiny_solve max_iter={max_iter}: {k}"
        assert ns.work.iter == st2["iter"][0] and ns.work.status == st2["status"][0]
    sol.close()


def test_fp64_native_names_as_shipped_hovering_loop(tinympc, oracle_mod):
    """examples/quadrotor_hovering.cpp exactly as the reference is checked in — typedef double tinytype, N = 10 — written against
    include/tinympc_admm.h with TINYMPC_TINYTYPE_DOUBLE: TinySolver{settings, cache, work} with double members, tiny_solve(&solver)
    in the loop of :90-114.  Iteration counts and controls of all 70 steps equal the compiled example's (1 269 iterations)."""
    from accelerated_tinympc_amd import native
    O = oracle_mod
    meta, prob, solves, z = load_fixture("quad_hover_f64_N10")
    ns = native.NativeSolver(prob, solves[0]["settings"], dtype=np.float64)
    for k, arr in zip(("x_min", "x_max", "u_min", "u_max"), bounds_of(prob, np.float64)):
        ns.a[k][:] = arr
    ns.a["Xref"][:] = solves[0]["xref"]
    orc = O.Oracle(prob, np.float64)
    x0 = solves[0]["pre"]["x"][0, 0].copy()
    iters, u0s = [], []
    for k in range(70):
        ns.a["x"][0] = x0
        ns.a["y"][:] = 0; ns.a["g"][:] = 0
        ns.tiny_solve()
        iters.append(ns.work.iter); u0s.append(ns.a["u"][0].copy())
        x0 = orc.plant_step(x0[None], ns.a["u"][0][None])[0]
    assert np.array_equal(np.array(iters), z["trace_iter"]) and np.array_equal(np.array(u0s), z["trace_u0"][:, :] if z["trace_u0"].ndim == 2 else z["trace_u0"])
    assert sum(iters) == 1269


@pytest.mark.parametrize("nx,nu,N", [(4, 1, 10), (8, 4, 9), (12, 4, 30)])
def test_fp64_device_closed_loop_vs_oracle(tinympc, oracle_mod, nx, nu, N):
    """tiny_batch64_mpc_step over a batch: 12 closed-loop steps equal the oracle's solve + its plant step (pinned against the
    compiled Eigen expression, tests/test_oracle.py) bit for bit — the sequential order for nx < 8, the GEMV order for nx >= 8."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, N) if (nx, nu) == (12, 4) else (pr.cartpole(N, riccati=O.riccati) if nx == 4 else pr.random_system(nx, nu, N, seed=804, riccati=O.riccati))
    B = 37
    rng = np.random.default_rng(N)
    x0 = rng.uniform(-0.2, 0.2, size=(B, nx))
    xref = rng.standard_normal((N, nx)) * 0.05
    bnds = pr.bounds_arrays(prob, np.float64)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=40)
    sol = tinympc.TinyBatchSolver64(prob, B, settings=settings)
    sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_x0(x0)
    orc = O.Oracle(prob, np.float64, settings)
    st = O.new_state(B, nx, nu, N, np.float64); st["x"][:, 0] = x0
    for k in range(12):
        st["y"][:] = 0; st["g"][:] = 0
        orc.solve(st, *bnds, xref, nthreads=8)
        u0 = st["u"][:, 0].copy()
        xn = orc.plant_step(st["x"][:, 0].copy(), u0)
        sol.mpc_step()
        xg, ug = sol.first_columns()
        assert np.array_equal(ug, u0) and np.array_equal(xg, xn) and np.array_equal(np.signbit(xg), np.signbit(xn)), f"step {k}"
        assert np.array_equal(sol.get_status()[0], st["iter"])
        st["x"][:, 0] = xn
    sol.close()


F64_ROWS = {(12, 4, 10), (12, 4, 30), (12, 4, 20), (4, 1, 10), (8, 4, 9)}   # TINY_FOR_EACH_F64ROWS
F64_ROWS_RT = {(12, 4), (4, 1), (8, 4), (12, 2), (4, 2), (4, 4)}            # TINY_FOR_EACH_F64ROWS_RT: any horizon up to 64


def f64_rows_name(nx, nu, N):
    """Name of the sixteen-lane fp64 kernel that serves (nx, nu, N), or None."""
    if (nx, nu, N) in F64_ROWS:
        return f"rows64<{nx},{nu},{N}>"
    if (nx, nu) in F64_ROWS_RT and 2 <= N <= 64:
        return f"rows64<{nx},{nu},n<={32 if N <= 32 else 64}>"
    return None


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("nx,nu,N", [(12, 4, 30), (12, 4, 10), (12, 4, 20), (4, 1, 10), (8, 4, 9), (12, 4, 13), (12, 2, 11), (4, 2, 8), (4, 4, 6), (16, 4, 10),
                                     (12, 4, 2), (12, 4, 32), (12, 4, 33), (12, 4, 64), (4, 1, 47), (8, 4, 40), (12, 4, 65)])
def test_fp64_vs_oracle(tinympc, oracle_mod, nx, nu, N, kernel):
    """The fp64 library against the fp64 oracle (== the compiled reference's fp64 builds, tests/test_oracle.py) on random
    warm states with zeros and negative zeros: ragged batches, warm-started chain with dual resets, sparse termination
    checks, max_iter 0 / 1, bounds off, per-instance bounds and references.  Bitwise, signs of zeros included."""
    O, pr = oracle_mod, tinympc.problems
    if (nx, nu) == (12, 4):
        prob = pr.quadrotor(20, N)
    elif (nx, nu) == (4, 1):
        prob = pr.cartpole(N, riccati=O.riccati)
    else:
        prob = pr.random_system(nx, nu, N, seed=nx * 100 + nu, riccati=O.riccati)
    for B, settings, per_inst in ((1, {}, False), (63, dict(max_iter=30, check_termination=3), True), (130, dict(max_iter=1), False),
                                  (65, dict(max_iter=0), False), (200, dict(max_iter=25, en_state_bound=0, en_input_bound=0), True)):
        settings = dict(O.DEFAULT_SETTINGS, **settings)
        rng = np.random.default_rng(B + nx)
        st = O.new_state(B, nx, nu, N, np.float64)
        for k in STATE_ORDER:
            st[k][:] = rng.standard_normal(st[k].shape) * 0.3
        for k in ("x", "d", "v", "z", "g", "y"):
            st[k][rng.random(st[k].shape) < 0.1] = 0.0
            st[k][rng.random(st[k].shape) < 0.1] = -0.0
        st["residuals"][:] = rng.random((B, 4)); st["iter"][:] = 3; st["status"][:] = 11
        shared = tuple(np.array(v, np.float64) for v in pr.bounds_arrays(prob, np.float64))
        shared[2][0, 0] = 0.2 * shared[3][0, 0]   # a lower input bound above zero at step 0 (the nonexistent u step N-1 must not see it)
        if per_inst:
            bnds = tuple(a[None] * rng.uniform(0.1, 1.0, size=(B,) + a.shape) for a in shared)
            xref = rng.standard_normal((B, N, nx)) * 0.2
        else:
            bnds, xref = shared, rng.standard_normal((N, nx)) * 0.2
        sol = tinympc.TinyBatchSolver64(prob, B, settings=settings)
        rows_name = f64_rows_name(nx, nu, N)
        assert sol.kernel_name() == (rows_name or f"thread64<{nx},{nu}>")   # the automatic choice
        if kernel == 2 and rows_name is None:   # no sixteen-lane kernel for this class / horizon: refused, the thread kernel serves it
            with pytest.raises(tinympc.TinyBatchError):
                sol.select_kernel(2)
            assert sol.kernel_name() == f"thread64<{nx},{nu}>"
        else:
            sol.select_kernel(kernel)
            assert sol.kernel_name() == (rows_name if kernel == 2 else f"thread64<{nx},{nu}>")
        sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_state(st)
        orc = O.Oracle(prob, np.float64, settings)
        for k in range(3):
            if k:
                st["y"][:] = 0; st["g"][:] = 0
                sol.reset_dual_variables()
            rc_ref = orc.solve(st, *bnds, xref, nthreads=8)
            rc = sol.solve()
            assert rc == (1 if rc_ref else 0)
            assert_bitwise(sol.get_state(), st, f"fp64 ({nx},{nu},{N}) B={B} {settings} per_inst={per_inst} k={k}")
        sol.close()
    with pytest.raises(tinympc.TinyBatchError):
        tinympc.TinyBatchSolver64(dict(prob, nx=5), 4)


# The launcher x class pairs of the fp64 kernel units (csrc/admm_f64_*.hip) that no test above and no closed-loop test reaches, each at 5 instances
# (one full group of four and a tail group), max_iter = 10, bitwise against the fp64 oracle.
@pytest.mark.parametrize("nx,nu,N", [(4, 1, 3), (8, 4, 3), (12, 2, 33), (4, 4, 33)])
def test_fp64_rows_bodies_of_the_remaining_classes(tinympc, oracle_mod, nx, nu, N):
    """one solve on the run-time-horizon body at the smallest horizon that selects it: 3 for the capacity of 32, 33 for the capacity of 64"""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.cartpole(N, riccati=O.riccati) if (nx, nu) == (4, 1) else pr.random_system(nx, nu, N, seed=nx * 100 + nu, riccati=O.riccati)
    B, settings = 5, dict(O.DEFAULT_SETTINGS, max_iter=10)
    rng = np.random.default_rng(N + nx)
    st = O.new_state(B, nx, nu, N, np.float64)
    for k in STATE_ORDER:
        st[k][:] = rng.standard_normal(st[k].shape) * 0.3
    st["residuals"][:] = rng.random((B, 4)); st["iter"][:] = 3; st["status"][:] = 11
    bnds = tuple(np.array(v, np.float64) for v in pr.bounds_arrays(prob, np.float64))
    xref = rng.standard_normal((N, nx)) * 0.2
    sol = tinympc.TinyBatchSolver64(prob, B, settings=settings)
    assert sol.kernel_name() == f"rows64<{nx},{nu},n<={32 if N <= 32 else 64}>"
    sol.set_bounds(*bnds); sol.set_xref(xref); sol.set_state(st)
    rc_ref = O.Oracle(prob, np.float64, settings).solve(st, *bnds, xref, nthreads=4)
    assert sol.solve() == (1 if rc_ref else 0)
    assert_bitwise(sol.get_state(), st, f"fp64 ({nx},{nu},{N})")
    sol.close()


@pytest.mark.parametrize("nx,nu", [(12, 2), (4, 2), (4, 4), (16, 4)])
def test_fp64_step_functions_of_the_remaining_classes(tinympc, oracle_mod, nx, nu):
    """the six step functions over a batch, as test_fp64_step_functions_batched_and_native drives them, for the classes it does not hold"""
    O, pr = oracle_mod, tinympc.problems
    N, B = 3, 5
    prob = pr.random_system(nx, nu, N, seed=nx * 100 + nu, riccati=O.riccati)
    rng = np.random.default_rng(nx + nu)
    bnds = tuple(np.asarray(a, np.float64) * s for a, s in zip(pr.bounds_arrays(prob, np.float64), (0.2, 0.2, 1.0, 1.0)))
    settings = dict(O.DEFAULT_SETTINGS, max_iter=10, check_termination=2, abs_pri_tol=0.5, abs_dua_tol=5.0)
    st = O.new_state(B, nx, nu, N, np.float64)
    for k in STATE_ORDER:
        st[k][:] = rng.standard_normal(st[k].shape) * 0.3
    st["iter"][:] = 4; st["status"][:] = 11
    st["iter"][::3] = 5   # odd: termination_condition must skip these
    st["residuals"][:] = rng.uniform(0, 1, size=(B, 4))
    xref = rng.standard_normal((B, N, nx)) * 0.3
    orc = O.Oracle(prob, np.float64, settings)
    sol = tinympc.TinyBatchSolver64(prob, B, settings=settings)
    sol.set_bounds(*bnds); sol.set_xref(xref)
    for fn in O.Oracle.STEP_FUNCTIONS:
        sol.set_state(st)
        ref_rv = orc.step(fn, st, *bnds, xref)
        rv = getattr(sol, fn)()
        got = sol.get_state()
        if fn == "termination_condition":
            assert np.array_equal(rv, ref_rv)
        for k in STATE_ORDER + ("residuals",):
            assert np.array_equal(got[k], st[k]) and np.array_equal(np.signbit(got[k]), np.signbit(st[k])), f"{fn}: {k}"
    sol.close()


# ---------------------------------------------------------------------------------------------------------------------
# one node, several GPUs, from C++ through the C-ABI (one host thread, one handle + stream per device)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,devices", [(4096, "0,0"), (1000, "0,0,0"), (37, "0,0"), (40000, "0,0"), (40000, "all")])
def test_cpp_multi_device_example_equals_the_single_handle_solve(tinympc, tmp_path, B, devices):
    """examples/quadrotor_tracking_multigpu.cpp: the batch block-sharded over several handles (one per listed device; on a
    one-GPU box two or three handles on device 0, which exercises the same code: per-handle set_device, group solve, the
    gather of u.col(0) into one device buffer), compared by the program itself with ONE handle solving the whole batch: u.col(0),
    iteration counts and status bit for bit.  With every visible GPU listed it is the RCCL-free multi-GPU path of the C++ host."""
    import shutil
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if devices == "all":   # DISTINCT devices: the peer-copy branch of tiny_batch_group_gather_u0 (round-3 advisor); needs more than one GPU
        import torch
        n = torch.cuda.device_count()
        if n < 2:
            pytest.skip("one GPU here: the cross-device branch runs where the driver has a multi-GPU node")
        devices = ",".join(str(d) for d in range(min(n, 6)))
    lib_dir = root / "accelerated-tinympc_amd" / "lib"
    exe = tmp_path / "multigpu"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{root / 'include'}", str(root / "examples" / "quadrotor_tracking_multigpu.cpp"),
                        f"-L{lib_dir}", "-ltinympc_hip", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(root / "accelerated-tinympc_amd" / "data" / "quadrotor_20hz.bin"), str(B), devices],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "sharded == single handle, bit for bit" in r.stdout


def test_group_gather_u0_from_python(tinympc):
    """tiny_batch_group_gather_u0 / _get_u0 through ctypes: three handles of different sizes, blocks in handle order."""
    import ctypes as C
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    sizes = [100, 7, 333]
    x0, table, start = pr.tracking_batch(sum(sizes), 30, seed=5)
    sols, off = [], 0
    for n in sizes:
        s = tinympc.TinyBatchSolver(prob, n)
        s.set_bounds(*pr.bounds_arrays(prob)); s.set_xref_window(table, start[off:off + n]); s.set_x0(x0[off:off + n])
        sols.append(s); off += n
    tinympc.solve_group(sols)
    lib = sols[0].lib
    hs = (C.c_void_p * len(sols))(*[s._h for s in sols])
    out = np.zeros((sum(sizes), 4), np.float32)
    assert lib.tiny_batch_group_get_u0(hs, len(sols), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    want = np.concatenate([s.get_u()[:, 0] for s in sols])
    assert np.array_equal(out, want)
    for s in sols:
        s.close()


def test_codegen_random_example_bitwise(tinympc, oracle_mod):
    """The reference's own examples/codegen_random.cpp:19-31 — n = 2, m = 2, N = 3, rho = 0.1, per-row bounds with min > max — on
    the exact kernels of the (2, 2) class (round 3: added to TINY_FOR_EACH_ROWDIMS): golden vectors of the compiled reference with
    gains from the reference's tiny_codegen(), three chained solves, every array bit for bit, on the rolled-loop kernel (the
    automatic choice), the streaming row kernel and the six single-function kernels' fused equivalent."""
    meta, prob, solves, z = load_fixture("codegen_random_f32_2_2_3")
    bnds = [z[k] for k in ("bnd_xmin", "bnd_xmax", "bnd_umin", "bnd_umax")]
    for fam in (0, 2, 3):
        for s in solves:
            B = s["pre"]["x"].shape[0]
            sol = tinympc.TinyBatchSolver(prob, B, settings=s["settings"])
            sol.select_kernel(2); sol.set_row_kernel(fam)
            sol.set_bounds(*bnds); sol.set_xref(s["xref"]); sol.set_state(s["pre"])
            assert sol.kernel_name().startswith(("rowloop<2,2,exact", "rowstream<2,2,exact")), sol.kernel_name()
            rc = sol.solve()
            got = sol.get_state()
            sol.close()
            assert_bitwise(got, s["post"], f"codegen_random fam={fam} k={s['k']}")
            assert rc == (1 if s["rc"] > 0 else 0)


@pytest.mark.parametrize("exact,dispatch", [(True, 0), (True, 1), (False, 1)])
def test_tile16_persistent_queue_at_full_size_equals_row_kernel_bitwise(tinympc, exact, dispatch):
    """The headline kernel as the bench runs it (round 3): one persistent workgroup per CU, every wave drawing SEVERAL tiles from the
    queue, tile-granular longest-first dispatch, a ragged last tile — against the 16-lane kernel on the same 40 037 tracking
    instances: every work array, the residuals, status and the iteration counts of EVERY instance bit for bit, cold start and a
    warm second solve (the instantiation that loads its live-in)."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 40037
    x0, table, start = pr.tracking_batch(B, 30, seed=77)
    res = {}
    for fam in (5, 1):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.select_kernel(2 if exact else 3); sol.set_row_kernel(fam)
        sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.set_dispatch(dispatch)
        assert sol.kernel_name().startswith("tile16<12,4,30" if fam == 5 else "rowlane<12,4,30"), sol.kernel_name()
        sol.set_x0(x0); sol.solve()
        assert sol.dispatch_applied() == dispatch
        cold = sol.get_state()
        sol.set_x0(x0 * np.float32(0.97)); sol.reset_dual_variables(); sol.solve()   # warm start from the first solve's workspace
        res[fam] = (cold, sol.get_state())
        sol.close()
    for k, what in ((0, "cold"), (1, "warm")):
        assert_bitwise(res[5][k], res[1][k], f"tile16 (persistent, dispatch {dispatch}) vs rowlane, exact={exact}, {what}, B={B}")
    assert res[5][0]["iter"].max() >= 30 and res[5][0]["iter"].min() < 20  # the batch really is uneven: waves take different numbers of tiles


@pytest.mark.parametrize("family", [1, 5])
def test_history_order_of_warm_started_launches(tinympc, family):
    """tiny_batch_set_dispatch(2) / the automatic mode on a warm workspace: groups (16-lane kernel) or tiles (sixteen-instances-per-wave kernel) are
    dispatched longest first by the iteration counts the PREVIOUS solve of the same workspace left in iter[] (dispatch_order.hip,
    dispatch_order_history_kernel) — step by step, inside the on-chip closed loop, and with the two-ended tile queue forced on top.  Nothing but
    the time may change: every array, the residuals, status, iteration counts, the u0 trajectory and x0 of a tracking loop must equal the
    index-order run bit for bit; tiny_batch_dispatch_applied() reports 3 only where a history exists (not after a reset, not after an upload of
    iter[], not for launches below 4 096 groups)."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 20000 + 7
    x0, table, start = pr.tracking_batch(B, 30, seed=11)
    outs = {}
    for mode in (0, 2, -1):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.select_kernel(2); sol.set_row_kernel(family); sol.set_dispatch(mode)
        if family == 5 and mode == 2:
            sol.set_tile_queue(3)
        sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.set_x0(x0)
        applied = []
        sol.solve(); applied.append(sol.dispatch_applied())                       # cold: no history
        for _ in range(3):
            sol.mpc_step_async(1); sol.synchronize(); applied.append(sol.dispatch_applied())
        a = sol.get_state(); xa = sol.get_x0()
        traj = sol.mpc_run_traj(6, 1); applied.append(sol.dispatch_applied())       # the on-chip loop (state stays on chip between solves)
        b = sol.get_state(); xb = sol.get_x0()
        it = sol.get_status()[0]
        sol.set_status(iter=it)                                                   # an upload is not a history
        sol.mpc_step_async(1); sol.synchronize(); applied.append(sol.dispatch_applied())
        sol.reset_workspace(); sol.set_x0(x0); sol.solve(); applied.append(sol.dispatch_applied())
        outs[mode] = (a, xa, traj, b, xb, sol.get_state())
        assert applied == {0: [0, 0, 0, 0, 0, 0, 0], 2: [0, 3, 3, 3, 3, 0, 0], -1: [1, 3, 3, 3, 3, 0, 1]}[mode], (mode, applied)
        sol.close()
        # an on-chip closed-loop run that starts from a reset workspace: its tiles / groups by the predictor of its first (cold, longest) solve
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.select_kernel(2); sol.set_row_kernel(family); sol.set_dispatch(mode)
        sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.set_x0(x0)
        first = sol.mpc_run_traj(4, 1)
        assert sol.dispatch_applied() == {0: 0, 2: 0, -1: 1}[mode], (mode, sol.dispatch_applied())
        outs[mode] = outs[mode] + (first, sol.get_state())
        sol.close()
    for mode in (2, -1):
        for k in (0, 3, 5, 7):
            assert_bitwise(outs[mode][k], outs[0][k], f"history order (mode {mode}) vs index order, family {family}, state {k}")
        for k in (1, 2, 4, 6):
            assert np.array_equal(outs[mode][k], outs[0][k]), (mode, k)
    if family == 1:   # fp16 storage (fp32 duals by preference): the history key reads iter[] only, so the order applies there too — same bits as index order
        res = {}
        for mode in (0, 2):
            sol = tinympc.TinyBatchSolver(prob, B)
            sol.select_kernel(2); sol.set_row_kernel(1); sol.set_storage(16); sol.set_dispatch(mode)
            sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start); sol.set_x0(x0)
            sol.solve()
            for _ in range(2):
                sol.mpc_step_async(1)
            sol.synchronize()
            assert sol.dispatch_applied() == (3 if mode == 2 else 0), (mode, sol.dispatch_applied(), sol.kernel_name())
            res[mode] = sol.get_state()
            sol.close()
        assert_bitwise(res[2], res[0], "history order vs index order under fp16 storage")
    if family == 1:   # a launch SEQUENCE enqueued after one preparation (the captured graph of mpc_run on the rolled-loop kernel): its first solve has no
        # history (fresh handle, mode 2 -> index order), its later ones have — the order buffer must exist by then (it was allocated by mode at first)
        p17 = pr.quadrotor(20, 17)
        B17 = 16384 + 16
        x17, t17, s17 = pr.tracking_batch(B17, 17, seed=3)
        res = {}
        for mode in (0, 2):
            sol = tinympc.TinyBatchSolver(p17, B17)
            sol.set_dispatch(mode)
            sol.set_bounds(*pr.bounds_arrays(p17)); sol.set_xref_window(t17, s17); sol.set_x0(x17)
            assert sol.kernel_name().startswith("rowloop"), sol.kernel_name()
            traj = sol.mpc_run_traj(3, 1)
            assert sol.dispatch_applied() == (3 if mode == 2 else 0), (mode, sol.dispatch_applied())
            res[mode] = (traj, sol.get_state())
            sol.close()
        assert np.array_equal(res[0][0], res[2][0])
        assert_bitwise(res[2][1], res[0][1], "graph-replayed closed loop, history order vs index order")
    small = tinympc.TinyBatchSolver(prob, 4096)
    small.select_kernel(2); small.set_row_kernel(1); small.set_dispatch(2)
    small.set_bounds(*pr.bounds_arrays(prob)); small.set_xref_window(table, start[:4096]); small.set_x0(x0[:4096])
    small.solve(); small.mpc_step_async(1); small.synchronize()
    assert small.dispatch_applied() == 0
    small.close()


def test_automatic_dispatch_and_kernel_choice_follow_the_kind_of_launch(tinympc):
    """tiny_batch_set_dispatch(-1), the default since round 4: a launch that starts from a reset (or fresh) workspace is dispatched longest first —
    and, from 160 instances per compute unit on, goes to the sixteen-instances-per-wave kernel, which wins only in that order —; a warm-started
    one keeps the 16-lane kernel and is dispatched longest first by the iteration counts of the solve before it (second session of round 4; index order
    before).  An explicit mode overrides both ways.  None of it changes a bit of the results."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 65536
    x0, table, start = pr.tracking_batch(B, 30)
    outs = {}
    for mode in (None, 0, 1):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start)
        if mode is not None:
            sol.set_dispatch(mode)
        want_cold = "rowlane<12,4,30,exact>" if mode == 0 else "tile16<12,4,30,exact>"
        assert sol.kernel_name() == want_cold, (mode, sol.kernel_name())          # a fresh handle is a reset one
        sol.set_x0(x0); sol.solve()
        assert sol.dispatch_applied() == (0 if mode == 0 else 1), (mode, sol.dispatch_applied())
        cold = sol.get_u()
        want_warm = "tile16<12,4,30,exact>" if mode == 1 else "rowlane<12,4,30,exact>"
        assert sol.kernel_name() == want_warm, (mode, sol.kernel_name())          # the next launch is warm-started
        sol.set_x0(x0 * np.float32(0.98)); sol.reset_dual_variables(); sol.solve()
        assert sol.dispatch_applied() == {None: 3, 0: 0, 1: 1}[mode], (mode, sol.dispatch_applied())   # automatic: by the counts of the solve before it
        warm = sol.get_u()
        sol.reset_workspace()
        assert sol.kernel_name() == want_cold, (mode, sol.kernel_name())
        # a closed-loop run (all MPC steps of a tile inside one launch) takes the sixteen-instances-per-wave kernel from 160 instances per compute unit on
        assert sol.closed_loop_kernel_name() == "tile16<12,4,30,exact>", sol.closed_loop_kernel_name()
        outs[mode] = (cold, warm, sol.get_status()[0])
        sol.close()
    for mode in (0, 1):
        assert np.array_equal(outs[None][0], outs[mode][0]) and np.array_equal(outs[None][1], outs[mode][1]), mode
    small = tinympc.TinyBatchSolver(prob, 32768)
    small.set_bounds(*pr.bounds_arrays(prob)); small.set_xref_window(table, start[:32768])
    assert small.kernel_name() == "rowlane<12,4,30,exact>" and small.closed_loop_kernel_name() == "rowlane<12,4,30,exact>", (small.kernel_name(), small.closed_loop_kernel_name())
    small.close()
    with pytest.raises(tinympc.TinyBatchError):
        s2 = tinympc.TinyBatchSolver(prob, 8)
        try:
            s2.set_dispatch(3)
        finally:
            s2.close()


@pytest.mark.parametrize("N", [10, 20, 25])
def test_tile16_other_horizons_equal_the_row_kernel_bitwise(tinympc, N):
    """admm_tile16.hip is instantiated for the quadrotor horizons 10, 20, 25 and 30 (those whose slack fits its LDS share): each
    against the unrolled 16-lane kernel of the same horizon, both arithmetic modes, ragged batch, cold and warm, bit for bit."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, N)
    B = 1000 + N
    x0, table, start = pr.tracking_batch(B, N, seed=N)
    for variant in (2, 3):
        res = {}
        for fam in (5, 1):
            sol = tinympc.TinyBatchSolver(prob, B)
            sol.select_kernel(variant); sol.set_row_kernel(fam)
            sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start)
            assert sol.kernel_name().startswith(f"tile16<12,4,{N}" if fam == 5 else f"rowlane<12,4,{N}"), sol.kernel_name()
            sol.set_x0(x0); sol.solve()
            cold = sol.get_state()
            sol.set_x0(x0 * np.float32(1.02)); sol.reset_dual_variables(); sol.solve()
            res[fam] = (cold, sol.get_state())
            sol.close()
        for k in (0, 1):
            assert_bitwise(res[5][k], res[1][k], f"tile16 vs rowlane, N={N}, variant {variant}, solve {k}")
