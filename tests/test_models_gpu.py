"""Per-instance models (tiny_batch_set_models / set_systems) and the batched GPU Riccati, against the CPU oracle run once per distinct model
over that model's instances, and against the host tiny_riccati.  Bitwise everywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("x", "u", "q", "r", "p", "d", "v", "vnew", "z", "znew", "g", "y")


def _same(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _setup(T, kind, n_models, B, N, seed=3):
    pr = T.problems
    fam = pr.model_family(kind, n_models, B, seed=seed)
    mods = pr.family_caches(fam)
    probs = [dict(p, N=N, u_min=-0.5 if kind == "quadrotor" else -5.0, u_max=0.5 if kind == "quadrotor" else 5.0, x_min=-5.0, x_max=5.0)
             for p in mods["probs"]]
    return fam, mods, probs


def _inputs(T, probs, B, N, per_instance_bounds, seed=5):
    """x0, reference (window table/start for the quadrotor class, per-instance arrays otherwise) and bounds"""
    pr = T.problems
    p0 = probs[0]
    nx, nu = p0["nx"], p0["nu"]
    rng = np.random.default_rng(seed)
    xmn, xmx, umn, umx = pr.bounds_arrays(p0)
    if per_instance_bounds:
        s = rng.uniform(0.6, 1.0, size=(B, 1, 1)).astype(np.float32)
        xmn, xmx = np.broadcast_to(xmn, (B, N, nx)) * s, np.broadcast_to(xmx, (B, N, nx)) * s
        umn, umx = np.broadcast_to(umn, (B, N - 1, nu)) * s, np.broadcast_to(umx, (B, N - 1, nu)) * s
        xmn, xmx, umn, umx = (np.ascontiguousarray(a, np.float32) for a in (xmn, xmx, umn, umx))
    if nx == 12:
        x0, table, start = pr.tracking_batch(B, N, seed=seed)
        return x0, (table, start), (xmn, xmx, umn, umx)
    # a set point per instance, held along the horizon, near a start of moderate size: most instances converge before max_iter
    x0 = (0.2 * rng.standard_normal((B, nx))).astype(np.float32)
    xref = np.ascontiguousarray(np.broadcast_to(0.05 * rng.standard_normal((B, 1, nx)), (B, N, nx)), np.float32)
    return x0, xref, (xmn, xmx, umn, umx)


def _solver(T, probs, mods, B, x0, ref, bnd, variant=0, family=0):
    s = T.TinyBatchSolver(probs[0], B)
    s.set_models(mods)
    s.set_bounds(*bnd)
    if isinstance(ref, tuple):
        s.set_xref_window(*ref)
    else:
        s.set_xref(ref)
    s.set_x0(x0)
    if variant:
        s.select_kernel(variant)
    if family:
        s.set_row_kernel(family)
    return s


def _oracle(O, T, probs, model, B, N, x0, ref, bnd, st=None):
    nx, nu = probs[0]["nx"], probs[0]["nu"]
    if st is None:
        st = O.new_state(B, nx, nu, N)
        st["x"][:, 0] = x0
    if isinstance(ref, tuple):  # the device's window gather clamps at the last table row
        xref = ref[0][np.minimum(ref[1][:, None].astype(np.int64) + np.arange(N)[None, :], len(ref[0]) - 1)]
    else:
        xref = ref
    for m, p in enumerate(probs):
        idx = np.nonzero(model == m)[0]
        if idx.size == 0:
            continue
        sub = {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}
        b = [a[idx] if a.ndim == 3 else a for a in bnd]
        O.Oracle(p, np.float32).solve(sub, *b, np.ascontiguousarray(xref[idx]), nthreads=8)
        for k in st:
            st[k][idx] = sub[k]
    return st


def _check(s, st, what):
    got = s.get_state()
    for k in STATE + ("residuals", "status", "iter"):
        assert _same(got[k], st[k]), f"{what}: {k} differs from the oracle ({s.kernel_name()})"


CLASSES = [("quadrotor", 12, 4, 30, 4096, 16), ("cartpole", 4, 1, 10, 2048, 16), ("random83", 8, 3, 7, 2048, 16), ("quadrotor", 12, 4, 35, 1024, 16)]


@pytest.mark.parametrize("kind,nx,nu,N,B,nm", CLASSES, ids=[f"{c[0]}_{c[3]}" for c in CLASSES])
@pytest.mark.parametrize("pib", [False, True], ids=["shared_bounds", "inst_bounds"])
def test_heterogeneous_batch_bitwise(tinympc, oracle_mod, kind, nx, nu, N, B, nm, pib):
    T, O = tinympc, oracle_mod
    fam, mods, probs = _setup(T, kind, nm, B, N)
    x0, ref, bnd = _inputs(T, probs, B, N, pib)
    st = _oracle(O, T, probs, fam["model"], B, N, x0, ref, bnd)
    s = _solver(T, probs, mods, B, x0, ref, bnd)
    assert s.models_per_instance()
    kn = s.kernel_name()
    generic = (nx, nu, N) == (12, 4, 35)
    assert kn == (f"generic<{nx},{nu},exact,pm>" if generic else f"rowlane<{nx},{nu},{N},exact,pm>"), kn
    s.solve()
    _check(s, st, "auto")
    s.close()
    if not generic:  # forced exact 16-lane kernel
        f = _solver(T, probs, mods, B, x0, ref, bnd, variant=2, family=1)
        assert f.kernel_name() == kn
        f.solve()
        _check(f, st, "forced rowlane")
        f.close()


@pytest.mark.parametrize("N,variant", [(30, 2), (30, 3), (35, 4)], ids=["rowlane_exact", "rowlane_fma", "generic_exact"])
def test_same_model_everywhere_is_the_shared_path(tinympc, N, variant):
    T = tinympc
    pr = T.problems
    B = 1024
    prob = pr.quadrotor(20, N)
    x0, table, start = pr.tracking_batch(B, N, seed=11)
    bnd = pr.bounds_arrays(prob)
    mods = {k: np.broadcast_to(np.asarray(prob[k]), (B,) + np.asarray(prob[k]).shape) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")}
    mods["Q"] = np.broadcast_to(np.asarray(prob["Q"]), (B, 12))
    mods["rho"] = np.full(B, prob["rho"])
    out = []
    for pm in (False, True):
        s = T.TinyBatchSolver(prob, B)
        s.set_bounds(*bnd)
        s.set_xref_window(table, start)
        s.set_x0(x0)
        s.select_kernel(variant)
        if variant in (2, 3):
            s.set_row_kernel(1)
        if pm:
            s.set_models(mods)
            assert s.kernel_name().endswith(",pm>"), s.kernel_name()
        s.solve()
        out.append(s.get_state())
        s.close()
    for k in STATE + ("residuals", "status", "iter"):
        assert _same(out[0][k], out[1][k]), k


def test_closed_loop_on_chip_and_step_by_step(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    B, N, steps = 1024, 30, 20
    fam, mods, probs = _setup(T, "quadrotor", 16, B, N)
    x0, (table, start), bnd = _inputs(T, probs, B, N, False)
    st = O.new_state(B, 12, 4, N)
    x = x0.copy()
    u0s = []
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        _oracle(O, T, probs, fam["model"], B, N, None, (table, start + k), bnd, st=st)
        u0 = st["u"][:, 0].copy()
        u0s.append(u0)
        xn = np.empty_like(x)
        for m, p in enumerate(probs):
            idx = np.nonzero(fam["model"] == m)[0]
            xn[idx] = O.Oracle(p, np.float32).plant_step(x[idx], u0[idx])
        x = xn
    a = _solver(T, probs, mods, B, x0, (table, start), bnd)
    assert a.closed_loop_kernel_name() == "rowlane<12,4,30,exact,pm>", a.closed_loop_kernel_name()
    traj = a.mpc_run_traj(steps, 1)
    assert _same(traj, np.array(u0s))
    assert _same(a.get_x0(), x)
    st["x"][:, 0] = x  # the plant step after the last solve writes x.col(0)
    _check(a, st, "on-chip loop")
    a.close()
    b = _solver(T, probs, mods, B, x0, (table, start), bnd)
    for k in range(steps):
        b.mpc_step_async(1)
    assert _same(b.get_x0(), x)
    _check(b, st, "step by step")
    b.close()


def test_full_size_cold_start(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    B, N = 65536, 30
    fam, mods, probs = _setup(T, "quadrotor", 64, B, N, seed=21)
    x0, (table, start), bnd = _inputs(T, probs, B, N, False, seed=21)
    T.debug_guards(True)
    try:
        s = _solver(T, probs, mods, B, x0, (table, start), bnd)
        s.solve()
    finally:
        T.debug_guards(False)
    # the predictor reads shared gains: a cold launch with per-instance models keeps index order
    assert s.dispatch_applied() == 0
    assert T.debug_check() == 0
    got = s.get_state()
    rng = np.random.default_rng(0)
    sample = np.concatenate([rng.choice(np.nonzero(fam["model"] == m)[0], 8, replace=False) for m in range(64)])
    sample.sort()
    sub_model = fam["model"][sample]
    st = _oracle(O, T, probs, sub_model, sample.size, N, x0[sample], (table, start[sample]), bnd)
    for k in STATE + ("residuals", "status", "iter"):
        assert _same(got[k][sample], st[k]), k
    # a warm-started solve is ordered by the previous counts
    s.solve()
    assert s.dispatch_applied() == 3
    s.close()


def test_clear_models_and_refusals(tinympc):
    T = tinympc
    pr = T.problems
    B, N = 256, 30
    prob = pr.quadrotor(20, N)
    fam, mods, probs = _setup(T, "quadrotor", 4, B, N)
    x0, table, start = pr.tracking_batch(B, N, seed=2)
    ref = T.TinyBatchSolver(prob, B)
    s = T.TinyBatchSolver(prob, B)
    for h in (ref, s):
        h.set_bounds(*pr.bounds_arrays(prob))
        h.set_xref_window(table, start)
        h.set_x0(x0)
    s.set_models(mods)
    assert s.models_per_instance() and s.kernel_name() == "rowlane<12,4,30,exact,pm>"
    s.clear_models()
    assert not s.models_per_instance()
    ref.solve(); s.solve()
    a, b = ref.get_state(), s.get_state()
    for k in STATE + ("residuals", "status", "iter"):
        assert _same(a[k], b[k]), k
    s.set_models(mods)
    for fn in (s.forward_pass, s.update_slack, s.update_dual, s.update_linear_cost, s.backward_pass_grad, s.termination_condition):
        with pytest.raises(T.TinyBatchError, match="per-instance models"):
            fn()
    s.set_row_kernel(5)  # tile16
    with pytest.raises(T.TinyBatchError, match="tile16"):
        s.solve()
    s.set_row_kernel(0)
    with pytest.raises(T.TinyBatchError, match="streaming MFMA"):
        s.select_kernel(1)
    s.set_optional_terms(True, False)
    with pytest.raises(T.TinyBatchError, match="Uref"):
        s.solve()
    s.set_optional_terms(False, False)
    s.set_storage(16)
    with pytest.raises(T.TinyBatchError, match="fp32 storage"):
        s.solve()
    assert s.lib.tiny_batch_arithmetic(s._h) == -3
    s.set_storage(32)
    s.solve()
    ref.close(); s.close()


def _host_riccati(T, A, B, Q, R, rho):
    return T.riccati(A.shape[0], B.shape[1], A, B, Q, R, rho)


def test_gpu_riccati_bitwise_with_host(tinympc):
    T = tinympc
    pr = T.problems
    groups = [pr.model_family("quadrotor", 700, 700, seed=1), pr.model_family("cartpole", 700, 700, seed=2), pr.model_family("random83", 640, 640, seed=3)]
    for g, fam in enumerate(groups):
        A, Bm, Q, R, rho = (fam[k].copy() for k in ("A", "B", "Q", "R", "rho"))
        if g == 2:  # a singular system in the middle: R = -rho and B = 0 give R1 = 0
            Bm[5] = 0.0
            R[5] = -rho[5]
        nx, nu = A.shape[1], Bm.shape[2]
        got = T.riccati_batch(nx, nu, A, Bm, Q, R, rho)
        for i in range(len(rho)):
            if g == 2 and i == 5:
                assert got["iters"][i] == -1
                assert np.isnan(got["Kinf"][i]).all()
                continue
            h = _host_riccati(T, A[i], Bm[i], Q[i], R[i], rho[i])
            assert got["iters"][i] == h["iters"], (g, i)
            for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "coeff_d2p"):
                assert _same(got[k][i], h[k]), (g, i, k)


def test_gpu_riccati_32_16(tinympc):
    T = tinympc
    p = T.problems.random_system(32, 16, 50)
    A, Bm, Q, R = (np.asarray(p[k])[None] for k in ("Adyn", "Bdyn", "Q_raw", "R"))
    got = T.riccati_batch(32, 16, A, Bm, Q, R, np.array([p["rho"]]))
    h = _host_riccati(T, A[0], Bm[0], Q[0], R[0], p["rho"])
    assert got["iters"][0] == h["iters"]
    for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "coeff_d2p"):
        assert _same(got[k][0], h[k]), k


def test_set_systems_end_to_end(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    B, N = 4096, 30
    fam, mods, probs = _setup(T, "quadrotor", 16, B, N, seed=9)
    x0, ref, bnd = _inputs(T, probs, B, N, False, seed=9)
    a = T.TinyBatchSolver(probs[0], B)
    it = a.set_systems(fam["A"], fam["B"], fam["Q"], fam["R"], fam["rho"])
    assert (it > 0).all() and (it < 1000).all()
    b = _solver(T, probs, mods, B, x0, ref, bnd)
    for h in (a,):
        h.set_bounds(*bnd)
        h.set_xref_window(*ref)
        h.set_x0(x0)
    st = _oracle(O, T, probs, fam["model"], B, N, x0, ref, bnd)
    for h in (a, b):
        h.solve()
        _check(h, st, "set_systems" if h is a else "set_models")
    # a singular system: refused, models unchanged
    R = fam["R"].copy(); Bm = fam["B"].copy()
    Bm[3] = 0.0; R[3] = -fam["rho"][3]
    with pytest.raises(T.TinyBatchError, match="singular"):
        a.set_systems(fam["A"], Bm, fam["Q"], R, fam["rho"])
    a.reset_workspace(); a.set_x0(x0)
    a.solve()
    _check(a, st, "after a refused set_systems")
    a.close(); b.close()
