"""Shared helpers for the parity tests (test infrastructure)."""
import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
STATE_ORDER = ("x", "u", "q", "r", "p", "d", "v", "vnew", "z", "znew", "g", "y")
PROB_KEYS = ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn", "Q")


def load_fixture(name):
    z = np.load(GOLDEN / f"{name}.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    prob = dict(nx=meta["nx"], nu=meta["nu"], N=meta["N"], rho=meta["rho"])
    for k in PROB_KEYS:
        prob[k] = z["prob_" + k]
    prob["x_min"], prob["x_max"], prob["u_min"], prob["u_max"] = meta["bounds"]
    solves = []
    for s in range(meta["nsolves"]):
        pre = {k[len(f"s{s}_pre_"):]: z[k] for k in z.files if k.startswith(f"s{s}_pre_")}
        post = {k[len(f"s{s}_post_"):]: z[k] for k in z.files if k.startswith(f"s{s}_post_")}
        st = meta["settings_per_solve"][s] or meta["settings"]
        solves.append(dict(pre=pre, post=post, xref=z[f"s{s}_xref"], rc=meta["rcs"][s], settings=st, k=meta["ks"][s]))
    return meta, prob, solves, z


def bounds_of(prob, dt):
    N, nx, nu = prob["N"], prob["nx"], prob["nu"]
    return (np.full((N, nx), prob["x_min"], dt), np.full((N, nx), prob["x_max"], dt),
            np.full((N - 1, nu), prob["u_min"], dt), np.full((N - 1, nu), prob["u_max"], dt))


def rel_inf(a, b, floor):
    """per-instance relative infinity-norm error of a vs b, normalised by max(|b|_inf, floor)."""
    a = np.asarray(a, np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, np.float64).reshape(b.shape[0], -1)
    return np.max(np.abs(a - b), axis=1) / np.maximum(np.max(np.abs(b), axis=1), floor)


def scale_of(name, prob):
    """Natural magnitude used as the floor of the relative error of each work array."""
    if name in ("u", "z", "znew"):
        return max(abs(prob["u_max"]), abs(prob["u_min"]))
    if name in ("x", "v", "vnew"):
        return 1.0
    return 1.0


# ---- closed-loop drivers shared by tests/test_closed_loop_gpu.py and tests/test_closed_loop_host.py ------------------------------------------

SCALAR_ORDER = ("residuals", "status", "iter")


def same_bits(a, b):
    """equal, the signs of zeros included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b) and (a.dtype.kind != "f" or np.array_equal(np.signbit(a), np.signbit(b)))


def closed_loop_inputs(prob, B, refmode, seed, near_end=False, amp=(0.02, 0.6), bscale=(1.0, 0.1), dtype=np.float32):
    """(x0, ref, bnds) of one closed-loop case.  Every instance has its own x0 amplitude, spread geometrically over `amp`: the small ones converge
    at once and never touch a bound, the large ones sit on the (tightened, `bscale` x the class's stock) bounds and run out of iterations.
    ref: "shared" an [N][nx] array, "inst" a [B][N][nx] array, "window" a (table, start) pair whose windows lie inside the table at step 0 —
    with near_end within 6 rows of its end, so that they reach the device's clamp once they slide."""
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    rng = np.random.default_rng(seed)
    a = np.geomspace(amp[0], amp[1], B) if B > 1 else np.array([amp[1]])
    x0 = (rng.permutation(a)[:, None] * rng.uniform(-1.0, 1.0, size=(B, nx))).astype(dtype)
    bnds = tuple(np.full(shape, v, dtype) for shape, v in (((N, nx), bscale[0] * prob["x_min"]), ((N, nx), bscale[0] * prob["x_max"]),
                                                            ((N - 1, nu), bscale[1] * prob["u_min"]), ((N - 1, nu), bscale[1] * prob["u_max"])))
    if refmode == "window":
        rows = N + 24
        table = (0.02 * rng.standard_normal((rows, nx))).astype(dtype)
        start = (rng.integers(rows - N - 6, rows - N + 1, size=B) if near_end else rng.integers(0, 7, size=B)).astype(np.int32)
        return x0, (table, start), bnds
    shape = (N, nx) if refmode == "shared" else (B, N, nx)
    return x0, (0.02 * rng.standard_normal(shape)).astype(dtype), bnds


def ref_at(ref, k, adv, N, B):
    """the [B][N][nx] (or shared [N][nx]) reference of MPC step k: row i of a window is table[min(start + k*adv + i, rows - 1)], the clamp of the
    device's window gather"""
    if isinstance(ref, tuple):
        table, start = ref
        return np.ascontiguousarray(table[np.minimum(start[:, None].astype(np.int64) + k * adv + np.arange(N)[None, :], len(table) - 1)])
    return ref


def oracle_closed_loop(O, prob, dtype, settings, x0, ref, bnds, steps, adv, st=None):
    """The reference's closed loop (quadrotor_hovering.cpp:90-114 / quadrotor_tracking.cpp:93-118) on the oracle: per step y = g = 0, tiny_solve,
    x = Adyn*x + Bdyn*u.col(0); the work arrays persist (warm start).  Returns u.col(0), iter and status of every step, the final x and workspace."""
    nx, nu, N, B = prob["nx"], prob["nu"], prob["N"], len(x0)
    orc = O.Oracle(prob, dtype, settings)
    if st is None:
        st = O.new_state(B, nx, nu, N, dtype)
    x = np.array(x0, dtype)
    out = dict(u0=[], iter=[], status=[])
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        orc.solve(st, *bnds, ref_at(ref, k, adv, N, B), nthreads=8)
        u0 = st["u"][:, 0].copy()
        out["u0"].append(u0); out["iter"].append(st["iter"].copy()); out["status"].append(st["status"].copy())
        x = orc.plant_step(x, u0)
    st["x"][:, 0] = x  # the plant step after the last solve writes x.col(0)
    return dict(u0=np.array(out["u0"]), iter=np.array(out["iter"]), status=np.array(out["status"]), x=x, st=st)


def host_closed_loop(sol, plant, x0, ref, steps, adv):
    """The same loop driven from the host on a handle `sol` (the reference where the solve has no bitwise oracle: fma arithmetic, fp16 storage):
    set_x0, the window of step k, reset_dual_variables, solve, and the plant step on the host with `plant` (the fp32 oracle's), x carried in fp32.
    A window that has slid past the table's end is uploaded as the clamped per-instance array (set_xref_window refuses such a start)."""
    B, N = sol.B, sol.N
    x = np.array(x0, np.float32)
    out = dict(u0=[], iter=[], status=[])
    for k in range(steps):
        if isinstance(ref, tuple) and (k == 0 or adv):
            start = ref[1] + k * adv
            if int(start.max()) + N <= len(ref[0]):
                sol.set_xref_window(ref[0], start)
            else:
                sol.set_xref(ref_at(ref, k, adv, N, B))
        sol.set_x0(x)
        sol.reset_dual_variables()
        sol.solve()
        u0 = sol.get_u()[:, 0].copy()
        it, stt, _ = sol.get_status()
        out["u0"].append(u0); out["iter"].append(it); out["status"].append(stt)
        x = plant(x, u0)
    sol.set_x0(x)  # the plant step after the last solve writes x.col(0) (rounded into the storage format) and x0buf (fp32)
    return dict(u0=np.array(out["u0"]), iter=np.array(out["iter"]), status=np.array(out["status"]), x=x, st=sol.get_state())


def closed_loop_conditions(out, bnds, settings, what):
    """The conditions a closed-loop case's inputs must meet, checked on the oracle's loop: over the steps some instance runs out of iterations, some
    instance converges before max_iter (where max_iter > 1 leaves room for that), some input bound is active in u.col(0), the final state is finite.
    u is the forward pass's iterate, not the projected slack: where a bound is active ADMM leaves it on or just beyond the bound, so active means
    u.col(0) <= u_min or u.col(0) >= u_max."""
    mi = settings["max_iter"]
    assert ((out["status"] == 11) & (out["iter"] == mi)).any(), f"{what}: no instance reaches max_iter"
    if mi > 1:
        assert ((out["status"] == 1) & (out["iter"] < mi)).any(), f"{what}: no instance converges before max_iter"
    umn, umx = bnds[2][..., 0, :], bnds[3][..., 0, :]
    assert ((out["u0"] <= umn) | (out["u0"] >= umx)).any(), f"{what}: no input bound is active in u.col(0)"
    assert np.isfinite(out["x"]).all() and all(np.isfinite(out["st"][k]).all() for k in STATE_ORDER), f"{what}: the final state is not finite"


def positive_system(prob):
    """`prob` with Adyn and Bdyn entry-wise positive and Kinf entry-wise negative (an artificial cache: the solver is a function of its matrices
    whatever they came from).  From an all-negative-zero state every product of Adyn*x and of Bdyn*u.col(0) is then -0: the reference's GEMV
    accumulator, which starts at +0, returns +0 where a plain sum of the products returns -0, and the negative Kinf carries the sign of x.col(0)
    into the next step's u.col(0)."""
    return dict(prob, Adyn=np.abs(prob["Adyn"]), Bdyn=np.abs(prob["Bdyn"]), Kinf=-np.abs(prob["Kinf"]))


def zero_state_inputs(prob, B, seed, dtype=np.float32):
    """(x0, ref, bnds): instance 0 starts at -0 in every state, instance 1 at +0, the rest at zeros of random signs; one shared all-zero
    reference, the class's stock bounds.  (Every state stays a zero: the artificial gain of positive_system would not stabilise anything else.)"""
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    rng = np.random.default_rng(seed)
    x0 = np.copysign(0.0, rng.standard_normal((B, nx))).astype(dtype)
    x0[0], x0[1] = -0.0, 0.0
    return x0, np.zeros((N, nx), dtype), bounds_of(prob, dtype)


def rows_of_negative_zeros(prob, x, u0):
    """[B][nx]: the rows of x1 = Adyn*x + Bdyn*u0 whose products are -0 one and all (a sum that does not start at +0 gives -0 there)"""
    A, Bm = np.asarray(prob["Adyn"], x.dtype), np.asarray(prob["Bdyn"], x.dtype)
    neg = lambda p: np.all((p == 0) & np.signbit(p), axis=-1)
    return neg(A[None] * x[:, None, :]) & neg(Bm[None] * u0[:, None, :])


def closed_loop_case(pr, O, z, name):
    """(prob, x0, xref_fn(k), steps, settings, window table/start or None) of one scenario of closed_loop_traces.npz"""
    meta = json.loads(bytes(z["meta"]).decode())[name]
    if name in ("hover", "track"):
        prob = pr.quadrotor(20, 30)
    elif name == "cartpole":
        rc = np.load(GOLDEN / "riccati_cartpole.npz")
        prob = dict(pr.cartpole(10, riccati=O.riccati), Kinf=rc["Kinf"], Pinf=rc["Pinf"], Quu_inv=rc["Quu_inv"], AmBKt=rc["AmBKt"])
    else:
        prob = pr.random_system(8, 3, 7, seed=99, riccati=O.riccati)
    N = meta["N"]
    table = start = None
    if name == "hover":
        xr = np.tile(pr.HOVER_XREF, (N, 1)).astype(np.float32)
        fn = lambda k: xr
    elif name == "track":
        table, start = pr.y_axis_line().astype(np.float32), z["track_start"]
        fn = lambda k: pr.expand_windows(table, start + k, N)
    elif name == "cartpole":
        xr = np.zeros((N, 4), np.float32)
        fn = lambda k: xr
    else:
        xr = z["dims837_xref"].astype(np.float32)
        fn = lambda k: xr
    return prob, z[f"{name}_x0"], fn, meta["steps"], meta["settings"], table, start
