"""Every per-instance-model kernel path (tiny_batch_set_models) against a reference, with models that differ in every matrix.

Exact arithmetic is pinned bit for bit against the CPU oracle, run once per distinct model over that model's instances.  fma arithmetic has no
bitwise oracle: its reference is the batch-shared 16-lane fma kernel (rowlane<...,fast>), run once per model on that model's instances with the
same x0, reference and bounds.  The batched GPU Riccati is pinned against the host tiny_riccati on the shapes and branches the family tests miss.
tests/test_models_host.py checks that ROWLANE below lists every class of TINY_FOR_EACH_ROWLANE."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("x", "u", "q", "r", "p", "d", "v", "vnew", "z", "znew", "g", "y")
ALL = STATE + ("residuals", "status", "iter")

# TINY_FOR_EACH_ROWLANE: admm_rowlane_pm_kernel is instantiated for each class x {exact, fma} x {one solve, per-instance bounds, on-chip closed loop}
ROWLANE = [(12, 4, 30), (12, 4, 25), (12, 4, 20), (12, 4, 10), (4, 1, 10), (8, 3, 7), (12, 4, 40), (12, 4, 50)]
ARITH = ("exact", "fast")
SOLVE_CASES = [(c, a, bpi) for c in ROWLANE for a in ARITH for bpi in (False, True)]
MPC_CASES = [(c, a) for c in ROWLANE for a in ARITH]
# the run-time-dimension classes of tests/test_parity_gpu.py (GENERIC_DIMS) and a quadrotor horizon without a 16-lane instantiation
GENERIC = [(20, 12, 12), (3, 2, 6), (8, 8, 6), (4, 3, 9), (36, 4, 5), (28, 16, 6), (12, 4, 35)]

# ragged batches (1, 2, 3, 4k+1, 4k+3) and one of a few thousand, and the settings, spread over the 32 one-solve cases
SIZES = [1, 37, 2, 67, 3, 131, 2051]
SETTINGS = [dict(), dict(max_iter=1), dict(check_termination=3), dict(en_state_bound=0), dict(max_iter=6)]


def _same(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _family(T, nx, nu, n_models, B, seed):
    pr = T.problems
    if nx == 12:
        fam = pr.model_family("quadrotor", n_models, B, seed=seed, vary="all")
    elif (nx, nu) == (4, 1):
        fam = pr.model_family("cartpole", n_models, B, seed=seed, vary="all")
    else:
        fam = pr.model_family("random", n_models, B, seed=seed, dims=(nx, nu))
    return fam, pr.family_caches(fam)


def _probs(mods, N, nx):
    um = 0.5 if nx == 12 else 5.0
    return [dict(p, N=N, u_min=-um, u_max=um, x_min=-5.0, x_max=5.0) for p in mods["probs"]]


def _inputs(T, nx, nu, N, B, pib, refmode, seed):
    """x0, reference (a (table, start) window pair or an xref array, shared [N][nx] or per instance) and bounds (shared or per instance)"""
    pr = T.problems
    rng = np.random.default_rng(seed)
    um = 0.5 if nx == 12 else 5.0
    xmn, xmx = np.full((N, nx), -5.0, np.float32), np.full((N, nx), 5.0, np.float32)
    umn, umx = np.full((N - 1, nu), -um, np.float32), np.full((N - 1, nu), um, np.float32)
    if pib:
        s = rng.uniform(0.3, 1.0, size=(B, 1, 1)).astype(np.float32)
        xmn, xmx, umn, umx = (np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape) * s, np.float32) for a in (xmn, xmx, umn, umx))
    if nx == 12 and refmode == "window":
        x0, table, start = pr.tracking_batch(B, N, seed=seed)
        return x0, (table, start), (xmn, xmx, umn, umx)
    x0 = (0.3 * rng.standard_normal((B, nx))).astype(np.float32)
    if refmode == "window":
        table = (0.1 * rng.standard_normal((N + 20, nx))).astype(np.float32)
        return x0, (table, rng.integers(0, 20, size=B).astype(np.int32)), (xmn, xmx, umn, umx)
    if refmode == "shared":
        return x0, (0.05 * rng.standard_normal((N, nx))).astype(np.float32), (xmn, xmx, umn, umx)
    return x0, (0.05 * rng.standard_normal((B, N, nx))).astype(np.float32), (xmn, xmx, umn, umx)


def _sub_ref(ref, idx):
    if isinstance(ref, tuple):
        return ref[0], ref[1][idx]
    return ref[idx] if ref.ndim == 3 else ref


def _expand(ref, N, B):
    if isinstance(ref, tuple):  # the device's window gather clamps at the last table row
        return ref[0][np.minimum(ref[1][:, None].astype(np.int64) + np.arange(N)[None, :], len(ref[0]) - 1)]
    return np.ascontiguousarray(np.broadcast_to(ref, (B,) + ref.shape[-2:]))


def _set_inputs(s, x0, ref, bnd):
    s.set_bounds(*bnd)
    if isinstance(ref, tuple):
        s.set_xref_window(*ref)
    else:
        s.set_xref(ref)
    s.set_x0(x0)


def _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, variant):
    s = T.TinyBatchSolver(probs[0], B, settings=settings)
    s.set_models(mods)
    _set_inputs(s, x0, ref, bnd)
    s.select_kernel(variant)
    if variant in (2, 3):
        s.set_row_kernel(1)
    return s


def _oracle_solve(O, probs, model, st, ref, bnd, settings):
    """one tiny_solve per instance, in place on st, each model's instances with that model"""
    B, N = st["x"].shape[0], st["x"].shape[1]
    xref = _expand(ref, N, B)
    for m, p in enumerate(probs):
        idx = np.nonzero(model == m)[0]
        if idx.size == 0:
            continue
        sub = {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}
        O.Oracle(p, np.float32, settings).solve(sub, *[a[idx] if a.ndim == 3 else a for a in bnd], np.ascontiguousarray(xref[idx]), nthreads=8)
        for k in st:
            st[k][idx] = sub[k]


def _oracle_plant(O, probs, model, x, u0):
    xn = np.empty_like(x)
    for m, p in enumerate(probs):
        idx = np.nonzero(model == m)[0]
        if idx.size:
            xn[idx] = O.Oracle(p, np.float32).plant_step(x[idx], u0[idx])
    return xn


class _SharedFma:
    """The fma reference: the batch-shared 16-lane fma kernel, one handle per model on that model's instances."""

    def __init__(self, T, probs, model, x0, ref, bnd, settings):
        self.B, self.parts = len(model), []
        for m, p in enumerate(probs):
            idx = np.nonzero(model == m)[0]
            if idx.size == 0:
                continue
            s = T.TinyBatchSolver(p, idx.size, settings=settings)
            _set_inputs(s, x0[idx], _sub_ref(ref, idx), tuple(a[idx] if a.ndim == 3 else a for a in bnd))
            s.select_kernel(3)
            s.set_row_kernel(1)
            assert s.kernel_name() == f"rowlane<{p['nx']},{p['nu']},{p['N']},fast>", s.kernel_name()
            self.parts.append((idx, s))

    def call(self, fn, *args):
        return [getattr(s, fn)(*args) for _, s in self.parts]

    def state(self):
        out = None
        for idx, s in self.parts:
            st = s.get_state()
            if out is None:
                out = {k: np.zeros((self.B,) + v.shape[1:], v.dtype) for k, v in st.items()}
            for k in st:
                out[k][idx] = st[k]
        return out

    def gather(self, fn, *args):
        """a per-instance array method (get_x0, mpc_run_traj) of every part, assembled in instance order (instances on axis -2 for traj)"""
        vals = self.call(fn, *args)
        shape = list(vals[0].shape)
        ax = 1 if vals[0].ndim == 3 else 0
        shape[ax] = self.B
        out = np.zeros(shape, vals[0].dtype)
        for (idx, _), v in zip(self.parts, vals):
            if ax:
                out[:, idx] = v
            else:
                out[idx] = v
        return out

    def close(self):
        self.call("close")


def _check(got, want, what):
    for k in ALL:
        assert _same(got[k], want[k]), f"{what}: {k} differs"


def _case_id(c):
    (nx, nu, N), a, bpi = c
    return f"{nx}_{nu}_{N}-{a}-{'inst_bounds' if bpi else 'shared_bounds'}"


@pytest.mark.parametrize("case", SOLVE_CASES, ids=[_case_id(c) for c in SOLVE_CASES])
def test_rowlane_pm_solve_and_warm_chain(tinympc, oracle_mod, case):
    """One admm_rowlane_pm_kernel instantiation (one solve, shared or per-instance bounds): a cold solve, a warm solve from the live-in state,
    then a solve after reset_dual_variables.  Exact: bitwise the oracle.  fma: bitwise the shared fma kernel run per model."""
    T, O = tinympc, oracle_mod
    (nx, nu, N), arith, pib = case
    i = SOLVE_CASES.index(case)
    B = SIZES[i % len(SIZES)]
    settings = dict(O.DEFAULT_SETTINGS, **SETTINGS[i % len(SETTINGS)])
    fam, mods = _family(T, nx, nu, min(B, 6), B, seed=100 + i)
    probs = _probs(mods, N, nx)
    x0, ref, bnd = _inputs(T, nx, nu, N, B, pib, "window" if nx == 12 else ("per_instance", "shared")[i % 2], seed=200 + i)
    s = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, 2 if arith == "exact" else 3)
    assert s.kernel_name() == f"rowlane<{nx},{nu},{N},{arith},pm>", s.kernel_name()
    if arith == "exact":
        st = O.new_state(B, nx, nu, N)
        st["x"][:, 0] = x0
    else:
        ref_h = _SharedFma(T, probs, fam["model"], x0, ref, bnd, settings)
    for step in ("cold", "warm", "duals reset"):
        if step == "duals reset":
            s.reset_dual_variables()
        s.solve()
        if arith == "exact":
            if step == "duals reset":
                st["y"][:] = 0
                st["g"][:] = 0
            _oracle_solve(O, probs, fam["model"], st, ref, bnd, settings)
        else:
            if step == "duals reset":
                ref_h.call("reset_dual_variables")
            ref_h.call("solve")
            st = ref_h.state()
        _check(s.get_state(), st, f"{case} {step}")
    if settings["max_iter"] == 6 and B > 3:  # the cap leaves instances unsolved
        assert (st["status"] != 1).any()
    s.close()
    if arith != "exact":
        ref_h.close()


def _oracle_loop(O, probs, model, x0, ref, bnd, steps, advance, settings=None, st=None):
    """the closed loop of quadrotor_tracking.cpp on the oracle, each instance with its own model: (u0 trajectory, final x0, final state)"""
    B, nx, nu, N = len(x0), probs[0]["nx"], probs[0]["nu"], probs[0]["N"]
    if st is None:
        st = O.new_state(B, nx, nu, N)
    x = x0.copy()
    u0s = []
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        r = (ref[0], ref[1] + k * advance) if isinstance(ref, tuple) else ref
        _oracle_solve(O, probs, model, st, r, bnd, settings)
        u0 = st["u"][:, 0].copy()
        u0s.append(u0)
        x = _oracle_plant(O, probs, model, x, u0)
    st["x"][:, 0] = x  # the plant step after the last solve writes x.col(0)
    return np.array(u0s), x, st


@pytest.mark.parametrize("case", MPC_CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}-{a}" for c, a in MPC_CASES])
def test_rowlane_pm_closed_loop(tinympc, oracle_mod, case):
    """The on-chip closed loop (admm_rowlane_pm_kernel with MPC = true, mpc_run_traj) and k x mpc_step_async (one-solve kernel + plant_step_pm_kernel
    on the ROW layout), with Adyn different in every model: exact against the oracle loop with each model's plant step, fma against the shared
    fma kernel's own closed loop run per model."""
    T, O = tinympc, oracle_mod
    (nx, nu, N), arith = case
    i = MPC_CASES.index(case)
    B, steps = (67, 37, 19)[i % 3], 4
    fam, mods = _family(T, nx, nu, 6, B, seed=300 + i)
    probs = _probs(mods, N, nx)
    x0, ref, bnd = _inputs(T, nx, nu, N, B, False, "window" if nx == 12 else "per_instance", seed=400 + i)
    adv = 1 if isinstance(ref, tuple) else 0
    settings = dict(O.DEFAULT_SETTINGS)
    v = 2 if arith == "exact" else 3
    if arith == "exact":
        u0s, x, st = _oracle_loop(O, probs, fam["model"], x0, ref, bnd, steps, adv, settings)
    else:
        r = _SharedFma(T, probs, fam["model"], x0, ref, bnd, settings)
        u0s, x = r.gather("mpc_run_traj", steps, adv), r.gather("get_x0")
        st = r.state()
        r.close()
    a = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, v)
    assert a.closed_loop_kernel_name() == f"rowlane<{nx},{nu},{N},{arith},pm>", a.closed_loop_kernel_name()
    traj = a.mpc_run_traj(steps, adv)
    assert _same(traj, u0s), "on-chip loop: u0 trajectory"
    assert _same(a.get_x0(), x), "on-chip loop: final x0"
    _check(a.get_state(), st, "on-chip loop")
    a.close()
    b = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, v)
    for _ in range(steps):
        b.mpc_step_async(adv)
    assert _same(b.get_x0(), x), "step by step: final x0"
    _check(b.get_state(), st, "step by step")
    b.close()


GEN_CONFIGS = [(False, "shared"), (True, "per_instance"), (True, "window"), (False, "window")]


@pytest.mark.parametrize("dims", GENERIC, ids=[f"{d[0]}_{d[1]}_{d[2]}" for d in GENERIC])
def test_generic_pm_paths(tinympc, oracle_mod, dims):
    """admm_generic_pm_kernel on every run-time-dimension class: shared and per-instance bounds; shared, per-instance and windowed references; cold,
    warm and duals-reset solves; k x mpc_step_async (plant_step_pm_kernel on the TILE layout) and mpc_run_async (the captured graph), all bitwise
    against the oracle with each instance's own model."""
    T, O = tinympc, oracle_mod
    nx, nu, N = dims
    B = 101  # not a multiple of 64
    g = GENERIC.index(dims)
    fam, mods = _family(T, nx, nu, 5, B, seed=500 + g)
    probs = _probs(mods, N, nx)
    for c, (pib, refmode) in enumerate(GEN_CONFIGS):
        settings = dict(O.DEFAULT_SETTINGS, **SETTINGS[(g + c) % len(SETTINGS)])
        x0, ref, bnd = _inputs(T, nx, nu, N, B, pib, refmode, seed=600 + 10 * g + c)
        s = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, 0)
        assert s.kernel_name() == f"generic<{nx},{nu},exact,pm>", s.kernel_name()
        st = O.new_state(B, nx, nu, N)
        st["x"][:, 0] = x0
        for step in ("cold", "warm", "duals reset"):
            if step == "duals reset":
                s.reset_dual_variables()
                st["y"][:] = 0
                st["g"][:] = 0
            s.solve()
            _oracle_solve(O, probs, fam["model"], st, ref, bnd, settings)
            _check(s.get_state(), st, f"{dims} {pib} {refmode} {step}")
        s.close()
    # closed loop: step by step and from the captured graph
    x0, ref, bnd = _inputs(T, nx, nu, N, B, False, "window", seed=700 + g)
    settings = dict(O.DEFAULT_SETTINGS)
    steps = 3
    u0s, x, st = _oracle_loop(O, probs, fam["model"], x0, ref, bnd, steps, 1, settings)
    a = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, 0)
    b = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, 0)
    for _ in range(steps):
        a.mpc_step_async(1)
    assert _same(a.get_x0(), x)
    _check(a.get_state(), st, f"{dims} step by step")
    b.mpc_run_async(steps, 1)
    assert _same(b.get_x0(), x)
    _check(b.get_state(), st, f"{dims} mpc_run_async")
    # a second run continues the trajectory from the graph
    u0s2, x2, st2 = _oracle_loop(O, probs, fam["model"], x, (ref[0], ref[1] + steps), bnd, 2, 1, settings, st=st)
    b.mpc_run_async(2, 1)
    assert _same(b.get_x0(), x2)
    _check(b.get_state(), st2, f"{dims} second mpc_run_async")
    a.close(); b.close()


def test_rowlane_class_forced_onto_generic_pm(tinympc):
    """variant 4 on a class with a 16-lane instantiation: generic<12,4,exact,pm> equals rowlane<12,4,30,exact,pm> bit for bit."""
    T = tinympc
    B, N = 75, 30
    fam, mods = _family(T, 12, 4, 6, B, seed=11)
    probs = _probs(mods, N, 12)
    x0, ref, bnd = _inputs(T, 12, 4, N, B, True, "window", seed=12)
    out = []
    for v in (2, 4):
        s = _pm_solver(T, probs, mods, B, x0, ref, bnd, None, v)
        s.solve(); s.solve(); s.reset_dual_variables(); s.solve()
        out.append((s.kernel_name(), s.get_state()))
        s.close()
    assert out[0][0] == "rowlane<12,4,30,exact,pm>" and out[1][0] == "generic<12,4,exact,pm>", (out[0][0], out[1][0])
    _check(out[1][1], out[0][1], "generic vs rowlane")


def _dev_models(mods, B, nx):
    """the eight [B] arrays of tiny_batch_set_models as device buffers, in the solver's column-major float32 layout"""
    from test_parity_gpu import DevBuf
    import accelerated_tinympc_amd.solver as S
    arrs = [np.asarray(mods["rho"], np.float32).reshape(B)] + [S._colmajor_batch(mods[k]) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")]
    arrs.append(np.asarray(mods["Q"], np.float32).reshape(B, nx))
    return [DevBuf(a) for a in arrs]


def test_models_lifecycle(tinympc, oracle_mod):
    """set_models twice with new contents (both packed forms re-derived), clear_models then set_models (reallocation), tiny_batch_set_models_device
    through device buffers, and a closed loop that follows new models written at the same record address."""
    import ctypes as C
    T, O = tinympc, oracle_mod
    B, N = 67, 20
    famA, modsA = _family(T, 12, 4, 5, B, seed=21)
    famB, modsB = _family(T, 12, 4, 5, B, seed=22)
    probsA, probsB = _probs(modsA, N, 12), _probs(modsB, N, 12)
    x0, ref, bnd = _inputs(T, 12, 4, N, B, False, "window", seed=23)
    settings = dict(O.DEFAULT_SETTINGS)

    def exact_ref(fam, probs):
        st = O.new_state(B, 12, 4, N)
        st["x"][:, 0] = x0
        _oracle_solve(O, probs, fam["model"], st, ref, bnd, settings)
        return st

    def fma_ref(fam, probs):
        r = _SharedFma(T, probs, fam["model"], x0, ref, bnd, settings)
        r.call("solve")
        st = r.state()
        r.close()
        return st

    def cold(s, variant):
        s.select_kernel(variant)
        s.reset_workspace()
        s.set_x0(x0)
        s.solve()
        return s.get_state()

    eA, eB, fA, fB = exact_ref(famA, probsA), exact_ref(famB, probsB), fma_ref(famA, probsA), fma_ref(famB, probsB)
    s = _pm_solver(T, probsA, modsA, B, x0, ref, bnd, settings, 2)
    _check(cold(s, 2), eA, "models A, exact")
    _check(cold(s, 3), fA, "models A, fma")
    s.set_models(modsB)
    _check(cold(s, 3), fB, "models B, fma")
    _check(cold(s, 2), eB, "models B, exact")
    s.clear_models()
    s.set_models(modsA)
    _check(cold(s, 2), eA, "models A after clear_models")
    _check(cold(s, 3), fA, "models A after clear_models, fma")
    # tiny_batch_set_models_device: the same records as set_models
    bufs = _dev_models(modsB, B, 12)
    try:
        s._check(s.lib.tiny_batch_set_models_device(s._h, *[C.c_void_p(b.ptr) for b in bufs]))
        s.synchronize()
    finally:
        for b in bufs:
            b.free()
    _check(cold(s, 2), eB, "models B through tiny_batch_set_models_device, exact")
    _check(cold(s, 3), fB, "models B through tiny_batch_set_models_device, fma")
    s.close()
    # a closed loop, new models at the same record address, the loop again: the second run follows the new models (exact and fma on-chip loops,
    # the captured graph of the run-time-dimension kernel)
    for v in (2, 3, 4):
        s = _pm_solver(T, probsA, modsA, B, x0, ref, bnd, settings, v)
        s.mpc_run_async(3, 1)
        if v == 3:
            r = _SharedFma(T, probsA, famA["model"], x0, ref, bnd, settings)
            r.call("mpc_run_async", 3, 1)
            assert _same(s.get_x0(), r.gather("get_x0")), "fma: first run"
            _check(s.get_state(), r.state(), "fma: first run")
            r.close()
            mid = s.get_state()
        else:
            _, x, st = _oracle_loop(O, probsA, famA["model"], x0, ref, bnd, 3, 1, settings)
            assert _same(s.get_x0(), x), f"variant {v}: first run"
            _check(s.get_state(), st, f"variant {v}: first run")
        s.set_models(modsB)
        s.mpc_run_async(3, 1)
        if v == 3:  # against a handle that had models B from the start and continues from the same state
            s2 = _pm_solver(T, probsB, modsB, B, x0, (ref[0], ref[1] + 3), bnd, settings, 3)
            s2.set_state(mid)
            s2.mpc_run_async(3, 1)
            assert _same(s.get_x0(), s2.get_x0()), "fma: the run after set_models"
            _check(s.get_state(), s2.get_state(), "fma: the run after set_models")
            s2.close()
        else:
            _, x2, st2 = _oracle_loop(O, probsB, famB["model"], x, (ref[0], ref[1] + 3), bnd, 3, 1, settings, st=st)
            assert _same(s.get_x0(), x2), f"variant {v}: the run after set_models"
            _check(s.get_state(), st2, f"variant {v}: the run after set_models")
        s.close()


@pytest.mark.parametrize("kind", ["cartpole", "generic"])
def test_set_systems_other_classes(tinympc, oracle_mod, kind):
    """tiny_batch_set_systems (GPU Riccati + systems_to_models_kernel) on the cartpole (16-lane kernel) and a run-time-dimension class: bitwise
    set_models with the host caches, and the oracle."""
    T, O = tinympc, oracle_mod
    nx, nu, N = (4, 1, 10) if kind == "cartpole" else (20, 12, 12)
    B = 83
    fam, mods = _family(T, nx, nu, 7, B, seed=31)
    probs = _probs(mods, N, nx)
    x0, ref, bnd = _inputs(T, nx, nu, N, B, True, "per_instance", seed=32)
    settings = dict(O.DEFAULT_SETTINGS)
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = x0
    _oracle_solve(O, probs, fam["model"], st, ref, bnd, settings)
    a = T.TinyBatchSolver(probs[0], B, settings=settings)
    it = a.set_systems(fam["A"], fam["B"], fam["Q"], fam["R"], fam["rho"])
    host_it = [T.riccati(nx, nu, fam["A"][b], fam["B"][b], fam["Q"][b], fam["R"][b], fam["rho"][b])["iters"] for b in range(B)]
    assert np.array_equal(it, host_it)
    _set_inputs(a, x0, ref, bnd)
    assert a.kernel_name() == (f"rowlane<{nx},{nu},{N},exact,pm>" if kind == "cartpole" else f"generic<{nx},{nu},exact,pm>"), a.kernel_name()
    a.solve()
    _check(a.get_state(), st, f"set_systems {kind}")
    a.close()


def test_history_dispatch_with_models(tinympc, oracle_mod):
    """B >= 16 384 + a ragged tail: a warm-started pm solve and an on-chip pm closed loop in history order (dispatch_applied() == 3) equal the
    index-order runs bit for bit, and the oracle on a per-model sample."""
    T, O = tinympc, oracle_mod
    B, N, steps = 16384 + 37, 30, 3
    fam, mods = _family(T, 12, 4, 16, B, seed=41)
    probs = _probs(mods, N, 12)
    x0, ref, bnd = _inputs(T, 12, 4, N, B, False, "window", seed=42)
    settings = dict(O.DEFAULT_SETTINGS)
    rng = np.random.default_rng(43)
    sample = np.sort(np.concatenate([rng.choice(np.nonzero(fam["model"] == m)[0], 6, replace=False) for m in range(16)] + [np.array([B - 1])]))
    sample = np.unique(sample)
    sub_model = fam["model"][sample]
    sub_ref = (ref[0], ref[1][sample])
    outs = []
    for mode in (2, 0):
        s = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, 0)
        s.set_dispatch(mode)
        s.solve()
        assert s.dispatch_applied() == 0  # a cold launch with per-instance models keeps index order
        s.solve()
        assert s.dispatch_applied() == (3 if mode == 2 else 0)
        warm = s.get_state()
        s.close()
        s = _pm_solver(T, probs, mods, B, x0, ref, bnd, settings, 0)
        s.set_dispatch(mode)
        s.solve()  # the history the closed loop is ordered by
        traj = s.mpc_run_traj(steps, 1)
        assert s.dispatch_applied() == (3 if mode == 2 else 0)
        outs.append((warm, traj, s.get_x0(), s.get_state()))
        s.close()
    _check(outs[0][0], outs[1][0], "warm solve: history order vs index order")
    assert _same(outs[0][1], outs[1][1]) and _same(outs[0][2], outs[1][2])
    _check(outs[0][3], outs[1][3], "closed loop: history order vs index order")
    # the oracle on the sample: cold + warm solve, and cold solve + closed loop
    bs = tuple(a for a in bnd)
    st = O.new_state(sample.size, 12, 4, N)
    st["x"][:, 0] = x0[sample]
    _oracle_solve(O, probs, sub_model, st, sub_ref, bs, settings)
    _oracle_solve(O, probs, sub_model, st, sub_ref, bs, settings)
    _check({k: v[sample] for k, v in outs[0][0].items()}, st, "warm solve vs the oracle")
    st = O.new_state(sample.size, 12, 4, N)
    st["x"][:, 0] = x0[sample]
    _oracle_solve(O, probs, sub_model, st, sub_ref, bs, settings)
    # the first MPC step starts from the cold solve's workspace with y = g = 0
    u0s, x, st = _oracle_loop(O, probs, sub_model, x0[sample], sub_ref, bs, steps, 1, settings, st=st)
    assert _same(outs[0][1][:, sample], u0s) and _same(outs[0][2][sample], x)
    _check({k: v[sample] for k, v in outs[0][3].items()}, st, "closed loop vs the oracle")


# ---- the batched GPU Riccati: shapes and branches the family tests do not reach ---------------------------------------------------------------------------

def _host(T, A, Bm, Q, R, rho):
    return T.riccati(A.shape[0], Bm.shape[1], A, Bm, Q, R, rho)


def _assert_like_host(T, got, i, A, Bm, Q, R, rho, what):
    h = _host(T, A, Bm, Q, R, rho)
    assert got["iters"][i] == h["iters"], (what, i, got["iters"][i], h["iters"])
    for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "coeff_d2p"):
        if k in got:
            assert _same(got[k][i], h[k]), (what, i, k)
    return h


def _systems(T, nx, nu, count, seed):
    fam = T.problems.model_family("random", count, count, seed=seed, dims=(nx, nu))
    return [fam["models"][k] for k in ("A", "B", "Q", "R", "rho")]


@pytest.mark.parametrize("nx,nu,count", [(1, 1, 70), (2, 5, 70), (3, 8, 70), (36, 4, 70), (64, 32, 3)])
def test_gpu_riccati_shapes(tinympc, nx, nu, count):
    """nu >= nx (the RHS scratch is nu * max(nx, nu)), a tall (36, 4) and the largest (64, 32): bitwise the host routine, with and without coeff_d2p."""
    T = tinympc
    A, Bm, Q, R, rho = _systems(T, nx, nu, count, seed=nx * 100 + nu)
    got = T.riccati_batch(nx, nu, A, Bm, Q, R, rho)
    for i in range(count):
        _assert_like_host(T, got, i, A[i], Bm[i], Q[i], R[i], rho[i], (nx, nu))
    nod2p = T.riccati_batch(nx, nu, A, Bm, Q, R, rho, coeff_d2p=False)
    assert "coeff_d2p" not in nod2p
    for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "iters"):
        assert _same(nod2p[k], got[k]), k


def test_gpu_riccati_lu_branches_and_iteration_cap(tinympc):
    """The LU row swap (|G(1,0)| > |G(0,0)|), the f == 0 elimination skip (a decoupled system) and the 1000-iteration cap, bitwise the host routine."""
    T = tinympc
    rng = np.random.default_rng(5)
    # row swap: two nearly parallel input columns, the second ten times the first, a small R + rho
    nx, nu = 4, 2
    A = 0.9 * np.eye(nx) + 0.02 * rng.standard_normal((nx, nx))
    b0 = rng.standard_normal(nx)
    Bsw = np.stack([0.1 * b0, 1.0 * b0 + 0.01 * rng.standard_normal(nx)], axis=1)
    sw = (A, Bsw, np.full(nx, 10.0), np.full(nu, 1e-3), 1e-3)
    # f == 0: diagonal A and Q, B's columns act on disjoint states, so G = R1 + B'PB stays diagonal
    dec = (np.diag([0.9, 0.8, 0.95, 0.7]), np.array([[0.5, 0.0], [0.3, 0.0], [0.0, 0.4], [0.0, 0.2]]), np.array([1.0, 2.0, 3.0, 4.0]), np.array([1.0, 0.5]), 0.7)
    # the cap: a marginally stable scalar system that B barely reaches (found by a search over B: the host routine stops at 1000)
    cap = (np.array([[1.0]]), np.array([[1e-3]]), np.array([1.0]), np.array([1.0]), 1.0)
    h = _host(T, *sw)
    G = np.diag(sw[3] + sw[4]) + sw[1].T @ h["Pinf"] @ sw[1]
    assert abs(G[1, 0]) > abs(G[0, 0])  # the first pivot column's largest entry is in row 1: lu_solve swaps
    hd = _host(T, *dec)
    Gd = np.diag(dec[3] + dec[4]) + dec[1].T @ hd["Pinf"] @ dec[1]
    assert Gd[1, 0] == 0.0 and Gd[0, 1] == 0.0  # the elimination factor is exactly 0: the row update is skipped
    assert _host(T, *cap)["iters"] == 1000
    for sysm in (sw, dec):
        got = T.riccati_batch(sysm[0].shape[0], sysm[1].shape[1], *[np.asarray(a)[None] for a in sysm[:4]], np.array([sysm[4]]))
        _assert_like_host(T, got, 0, *sysm, "lu")
    got = T.riccati_batch(1, 1, *[a[None] for a in cap[:4]], np.array([cap[4]]))
    _assert_like_host(T, got, 0, *cap, "cap")
    assert got["iters"][0] == 1000


def test_gpu_riccati_chunk_boundary(tinympc):
    """(64, 32) crosses the 1 GiB scratch chunk: chunk + 70 systems drawn from a pool of 70, each equal to its pool entry solved alone in a small
    call (its result depends on neither its chunk nor its wave slot), a host sample at the wave and chunk edges, one singular system at the edge."""
    T = tinympc
    nx, nu = 64, 32
    E = 4 * nx * nx + 3 * nu * nx + nu * max(nx, nu) + 2 * nu * nu  # riccati_batch_doubles
    chunk = (2 ** 30 // (8 * E)) // 64 * 64  # tiny_batch_riccati_device: systems per launch
    assert chunk == 4992
    count = chunk + 70
    rng = np.random.default_rng(51)
    pool = []
    for _ in range(70):
        A = np.eye(nx) + 0.05 * rng.standard_normal((nx, nx)) / 8
        A = 0.5 * A / np.max(np.abs(np.linalg.eigvals(A)))
        pool.append((A, 0.1 * rng.standard_normal((nx, nu)), 10.0 * rng.uniform(0.5, 2.0, nx), rng.uniform(0.5, 2.0, nu), rng.uniform(0.5, 2.0)))
    which = (np.arange(count) * 37) % 70  # every pool entry lands in many waves, slots and both chunks
    A, Bm, Q, R, rho = (np.array([pool[w][k] for w in which]) for k in range(5))
    alone = T.riccati_batch(nx, nu, *[np.array([p[k] for p in pool]) for k in range(5)])
    assert (alone["iters"] <= 30).all() and (alone["iters"] > 0).all(), alone["iters"]
    bad = chunk  # the first system of the second launch
    Bm[bad] = 0.0
    R[bad] = -rho[bad]
    got = T.riccati_batch(nx, nu, A, Bm, Q, R, rho)
    assert got["iters"][bad] == -1
    for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "coeff_d2p"):
        assert np.isnan(got[k][bad]).all(), k
    ok = np.arange(count) != bad
    for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "coeff_d2p", "iters"):
        assert _same(got[k][ok], alone[k][which[ok]]), k
    for i in (0, 63, 64, chunk - 1, chunk + 1, count - 1):
        _assert_like_host(T, got, i, A[i], Bm[i], Q[i], R[i], rho[i], "chunk edge")
    with pytest.raises(T.TinyBatchError):
        _host(T, A[bad], Bm[bad], Q[bad], R[bad], rho[bad])
