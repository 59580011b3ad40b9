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


# ---- the box projection at its edges, shared by tests/test_projection_host.py and tests/test_projection_gpu.py -----------------------------------------

PROJ_CATS = ("slack", "bind_lo", "bind_hi", "tie_lo", "tie_hi", "pinned", "zlo_pos", "zlo_neg", "zhi_pos", "zhi_neg", "infeasible", "inf_lo", "inf_hi")
PROJ_ZERO_CATS = tuple(PROJ_CATS.index(c) for c in ("zlo_pos", "zlo_neg", "zhi_pos", "zhi_neg"))
PROJ_EXACT = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, check_termination=1)


def _beside(t, up, h16):
    """the neighbour of t on the storage grid, above (up) or below; around zero the smallest step that stays clear of fp32 / fp64 subnormals (binary16
    keeps its subnormals in storage, so there the plain neighbour)"""
    if h16:
        return np.nextafter(t.astype(np.float16), np.float16(np.inf if up else -np.inf)).astype(np.float32)
    tiny = t.dtype.type(2.0 ** -60)
    n = np.nextafter(t, t.dtype.type(np.inf if up else -np.inf))
    return np.where(np.abs(t) < tiny, tiny if up else -tiny, n).astype(t.dtype)


def _bounds_of_category(cat, t, lo0, hi0, h16):
    """(lo, hi) of every entry from its category, the pre-projection value t it is crafted around and the class's stock box [lo0, hi0]"""
    C = {c: cat == k for k, c in enumerate(PROJ_CATS)}
    dt = t.dtype
    lo, hi = np.full(t.shape, lo0, dt), np.full(t.shape, hi0, dt)
    far = np.abs(t) + dt.type(1.0)
    lo = np.where(C["bind_lo"], _beside(t, True, h16), lo);   hi = np.where(C["bind_lo"], np.maximum(hi, far), hi)
    hi = np.where(C["bind_hi"], _beside(t, False, h16), hi);  lo = np.where(C["bind_hi"], np.minimum(lo, -far), lo)
    lo = np.where(C["tie_lo"] | C["pinned"], t, lo);          hi = np.where(C["tie_lo"], np.maximum(hi, far), hi)
    hi = np.where(C["tie_hi"] | C["pinned"], t, hi);          lo = np.where(C["tie_hi"], np.minimum(lo, -far), lo)
    lo = np.where(C["zlo_pos"], dt.type(0.0), lo);            lo = np.where(C["zlo_neg"], dt.type(-0.0), lo)
    hi = np.where(C["zhi_pos"], dt.type(0.0), hi);            hi = np.where(C["zhi_neg"], dt.type(-0.0), hi)
    lo = np.where(C["infeasible"], dt.type(0.3) * abs(hi0), lo); hi = np.where(C["infeasible"], -dt.type(0.2) * abs(lo0), hi)
    lo = np.where(C["inf_lo"], -np.inf, lo);                  hi = np.where(C["inf_hi"], np.inf, hi)
    return lo.astype(dt), hi.astype(dt)


def projection_case(O, prob, B, dtype, seed, per_instance):
    """Inputs that put the slack update (admm.cpp:51-60) of ITERATION 1 on the edges of its box: see PROJ_CATS.  dtype: np.float32, np.float64 or
    "h16" / "h16d" (float32 arrays on the binary16 grid, for the fp16-storage kernels).

    The first Z = B // 2 instances are all zeros of random sign (work arrays and Xref; instance 0 all -0, instance 1 all +0, x.col(0) of instances 2 and 3 likewise, and g.col(0) carries the
    sign of x.col(0), so that x + g is -0 wherever x.col(0) is); the rest a random warm state.  t = (x + g, u + y) of iteration 1 comes from the oracle with
    both bounds disabled — it does not depend on the bounds.  Categories follow a cyclic pattern with drawn strides over (instance, step, row): thirteen
    is prime, so every line of thirteen entries along a step, a row or the instances holds every category, the first and last step and row included.
    Then the four zero bounds are laid over the entries where some zero instance has t = -0 (per-instance tables: in that instance's own table, and over
    as many of its t = +0 entries; shared tables: over the entries where the zero instances are most evenly split between -0 and +0).
    per_instance = "const": per-instance tables that do not change along the horizon, crafted around step 0.
    A shared table without a line of thirteen ("dense") takes the nine other categories by turns over its entries instead, the first and last step and
    row first; with fewer than twenty-six entries its four zero bounds have their other side infinite.
    Ties use the instance's own t (per-instance tables) or, for a shared table, the t of a zero instance and of a warm instance by turns.
    Returns dict(st0, xref, bnds = (x_min, x_max, u_min, u_max), t = (tx, tu), cat = (cat_x, cat_u), laid = (laid_x, laid_u), dense = (.., ..), Z)."""
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    h16 = isinstance(dtype, str)
    dt = np.dtype(np.float32 if h16 else dtype)
    R = O.round_h16 if h16 else (lambda a: a)
    rng = np.random.default_rng(seed)
    Z = B // 2
    assert Z >= 4
    st0 = O.new_state(B, nx, nu, N, dt)
    for k in STATE_ORDER:
        st0[k][:] = R((rng.standard_normal(st0[k].shape) * 0.3).astype(dt))
    for k in ("x", "d", "v", "z", "g", "y"):
        st0[k][rng.random(st0[k].shape) < 0.1] = 0.0
        st0[k][rng.random(st0[k].shape) < 0.1] = -0.0
    xref = R((rng.standard_normal((B, N, nx)) * 0.2).astype(dt))
    for k in STATE_ORDER:
        st0[k][:Z] = np.copysign(0.0, rng.standard_normal(st0[k][:Z].shape))
        st0[k][0], st0[k][1] = -0.0, 0.0
    st0["x"][2, 0], st0["x"][3, 0] = -0.0, 0.0     # with instances 0 and 1: every state row has x.col(0) = -0 twice and +0 twice
    st0["g"][:Z, 0] = st0["x"][:Z, 0]
    xref[:Z] = np.copysign(0.0, rng.standard_normal(xref[:Z].shape))
    xref[0], xref[1] = -0.0, 0.0

    free = O.copy_state(st0)
    stock = tuple(np.asarray(b, dt) for b in bounds_of(prob, dt))
    O.Oracle(prob, dtype, dict(PROJ_EXACT, max_iter=1, en_state_bound=0, en_input_bound=0)).solve(free, *stock, xref)
    t = (free["vnew"].copy(), free["znew"].copy())
    assert all(np.all(a[:Z] == 0) for a in t), "a zero instance whose pre-projection values are not zeros"

    strides = rng.integers(1, len(PROJ_CATS), size=3)
    off = rng.integers(0, len(PROJ_CATS), size=2)
    bnds, cats, laids, denses = [], [], [], []
    for a, (tt, lo0, hi0) in enumerate(((t[0], prob["x_min"], prob["x_max"]), (t[1], prob["u_min"], prob["u_max"]))):
        _, S, n = tt.shape
        bi, si, ri = np.meshgrid(np.arange(B if per_instance else 1), np.arange(S), np.arange(n), indexing="ij")
        cat = ((bi * strides[0] + si * strides[1] + ri * strides[2] + off[a]) % len(PROJ_CATS)).astype(np.int32)
        laid, open_side, dense = np.zeros(cat.shape, bool), np.zeros(cat.shape, bool), False
        neg = np.signbit(tt[:Z])
        if per_instance:
            src = tt
            for b in range(Z):
                for sel in (neg[b], ~neg[b]):
                    idx = np.argwhere(sel)[:int(neg[b].sum())]
                    for j, (i, r) in enumerate(idx):
                        cat[b, i, r], laid[b, i, r] = PROJ_ZERO_CATS[(j + b) % 4], True
        else:
            dense = max(S, n) < len(PROJ_CATS)                               # no line of thirteen: the pattern need not reach every category
            small = S * n < 2 * len(PROJ_CATS)                               # ... and not even room for all of them beside the zero bounds
            split = np.minimum(neg.sum(axis=0), (~neg).sum(axis=0))          # how evenly an entry splits the zero instances
            order = np.argsort(-split.ravel(), kind="stable")
            left = 4 if dense and small else 8
            for e in order[split.ravel()[order] >= 2]:
                i, r = divmod(int(e), n)
                if left and (dense or (cat == cat[0, i, r]).sum() > 1):      # never over the only entry of its category
                    left -= 1
                    cat[0, i, r], laid[0, i, r] = PROJ_ZERO_CATS[left % 4], True
            # the source instance of every entry's ties: a zero instance and a warm one by turns
            turn = (si[0] + ri[0]) % 2 == 0
            if dense:   # the other nine categories by turns over the entries left: first step, last step, first row, last row, then the rest, each in a
                        # drawn order; in a small table the zero bounds have their other side infinite
                rank = np.select([si[0] == 0, si[0] == S - 1, ri[0] == 0, ri[0] == n - 1], [0, 1, 2, 3], 4).ravel() + rng.random(S * n)
                rest = [e for e in np.argsort(rank) if not laid.ravel()[e]]
                other = [k for k in range(len(PROJ_CATS)) if k not in PROJ_ZERO_CATS]
                cat.ravel()[rest] = [other[(j + off[a]) % len(other)] for j in range(len(rest))]
                open_side = laid & small
                turn = cat[0] == PROJ_CATS.index("pinned")                    # one tie of each side away from zero, the pinned entry on a zero
            inst = np.where(turn, (si[0] * n + ri[0]) % Z, Z + (si[0] * n + ri[0]) % (B - Z))
            src = np.take_along_axis(tt, inst[None], axis=0)
        if per_instance == "const":   # one row of bounds per instance, crafted around step 0 (where t can be -0) and held along the horizon
            cat, laid = np.repeat(cat[:, :1], S, axis=1), np.repeat(laid[:, :1], S, axis=1)
            src = np.repeat(src[:, :1], S, axis=1)
        lo, hi = _bounds_of_category(cat, src, dt.type(lo0), dt.type(hi0), h16)
        zlo = (cat == PROJ_ZERO_CATS[0]) | (cat == PROJ_ZERO_CATS[1])
        lo, hi = np.where(open_side & ~zlo, -np.inf, lo).astype(dt), np.where(open_side & zlo, np.inf, hi).astype(dt)
        if not per_instance:
            lo, hi = lo[0], hi[0]
        bnds += [R(lo), R(hi)]; cats.append(cat); laids.append(laid); denses.append(dense)
    return dict(st0=st0, xref=xref, bnds=tuple(bnds), t=t, cat=tuple(cats), laid=tuple(laids), dense=tuple(denses), Z=Z)


def med3_model(t, lo, hi):
    """v_med3_f32 as the ISA manual states it, on (t, min(lo, hi), hi) — how the kernels call it: the median through max / min that order -0 below +0
    (NaNs are out of scope).  med3(a, b, c) = max(min(a, b), min(max(a, b), c))."""
    key = lambda v: np.where(v == 0, np.where(np.signbit(v), -1, 1) * np.finfo(v.dtype).tiny / 2, v)   # orders -0 < +0, changes no other comparison
    mx = lambda a, b: np.where(key(a) >= key(b), a, b)
    mn = lambda a, b: np.where(key(a) <= key(b), a, b)
    lo = np.where(lo < hi, lo, hi)
    return mx(mn(t, lo), mn(mx(t, lo), hi))


def compare_select(t, lo, hi):
    """the reference's projection, admm.cpp:51-60 (u_max.cwiseMin(u_min.cwiseMax(t))): (lo < t) ? t : lo, then (t < hi) ? t : hi"""
    t = np.where(lo < t, t, lo)
    return np.where(t < hi, t, hi)


def projection_problem(pr, O, nx, nu, N):
    """the model of a class, as tests/test_oracle.py builds it for the compiled reference of that class"""
    if (nx, nu) == (12, 4):
        return pr.quadrotor(20, N)
    if (nx, nu) == (4, 1):
        return pr.cartpole(N, riccati=O.riccati)
    return pr.random_system(nx, nu, N, seed=nx * 100 + nu, riccati=O.riccati)


# every input set of tests/test_projection_gpu.py: (nx, nu, N, B, dtype, per_instance); the seed is the position in this list
PROJ_INPUTS = [(12, 4, 10, 21, np.float32, False), (12, 4, 10, 21, np.float32, True), (12, 4, 10, 21, np.float32, "const"), (8, 3, 7, 22, np.float32, False),
               (4, 2, 8, 20, np.float32, False), (4, 2, 8, 20, np.float32, True), (8, 4, 9, 20, np.float32, False), (8, 4, 9, 20, np.float32, True),
               (4, 1, 10, 28, np.float32, False), (16, 4, 10, 20, np.float32, False), (16, 4, 10, 20, np.float32, True),
               (32, 16, 6, 19, np.float32, False), (32, 16, 6, 19, np.float32, True), (3, 2, 6, 20, np.float32, True), (8, 8, 6, 20, np.float32, False),
               (12, 4, 10, 20, np.float64, False), (12, 4, 10, 20, np.float64, True), (4, 2, 8, 20, np.float64, False), (4, 2, 8, 20, np.float64, True),
               (12, 4, 10, 20, "h16", False), (12, 4, 10, 20, "h16d", False)]
_proj_cache = {}


def projection_input(pr, O, key):
    """(prob, case) of one entry of PROJ_INPUTS, built once and shared: callers copy what they change"""
    if key not in _proj_cache:
        nx, nu, N, B, dtype, mode = key
        prob = projection_problem(pr, O, nx, nu, N)
        _proj_cache[key] = (prob, projection_case(O, prob, B, dtype, PROJ_INPUTS.index(key), mode))
    return _proj_cache[key]


# ---- inputs on which no operation rounds, shared by tests/test_fma_oracle_host.py and tests/test_fma_oracle_gpu.py --------------------------------------

def _signed_selection(rng, rows, cols):
    """one entry of +-1 per row, in a drawn column"""
    m = np.zeros((rows, cols))
    m[np.arange(rows), rng.integers(0, cols, size=rows)] = rng.choice([-1.0, 1.0], size=rows)
    return m


def rounding_free_case(nx, nu, N, B, seed, terms=False):
    """(prob, settings, x0, xref, bnds, uref): small integers through signed selection matrices, rho = 1, tolerances 0.  Every product is then an
    integer times +-1 and every sum an integer far below 2^24, so for one or two iterations no fp32 operation rounds: a fused multiply-add and a
    multiply followed by an add give the same VALUE (not the same sign of a zero: negated gains flip those).  The caller sets max_iter and proves
    the premise by comparing the fp32 with the fp64 exact oracle: with the optional terms on, the values grow faster along the horizon and about half
    of the seeds round in the second iteration (seed 0 does not, at B = 8 and B = 37, for (12,4,10), (8,3,7), (4,1,10) and (2,2,3)).  terms: integer R and Uref and a signed selection coeff_d2p for the two optional terms."""
    rng = np.random.default_rng(seed)
    prob = dict(name=f"selection_{nx}_{nu}", nx=nx, nu=nu, N=N, rho=1.0, Kinf=_signed_selection(rng, nu, nx), Pinf=_signed_selection(rng, nx, nx),
                Quu_inv=_signed_selection(rng, nu, nu), AmBKt=_signed_selection(rng, nx, nx), Adyn=_signed_selection(rng, nx, nx),
                Bdyn=_signed_selection(rng, nx, nu), Q=rng.integers(1, 4, size=nx).astype(np.float64), u_min=-3.0, u_max=3.0, x_min=-50.0, x_max=50.0)
    settings = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, check_termination=1, en_state_bound=1, en_input_bound=1)
    uref = None
    if terms:
        prob["R"] = rng.integers(1, 4, size=nu).astype(np.float64)
        prob["coeff_d2p"] = _signed_selection(rng, nx, nu)
        uref = rng.integers(-2, 3, size=(B, N - 1, nu)).astype(np.float32)
        settings.update(en_uref=1, en_coeff_d2p=1)
    x0 = rng.integers(-4, 5, size=(B, nx)).astype(np.float32)
    xref = rng.integers(-2, 3, size=(B, N, nx)).astype(np.float32)
    return prob, settings, x0, xref, bounds_of(prob, np.float32), uref


def _signed_band(rng, rows, cols, k=2):
    """0 / +-1 with k entries per row, row r in columns r*k ... r*k + k - 1 (mod cols); k is raised to ceil(cols / rows), so that the rows together
    cover every column, and capped at cols.  The placement is fixed, the signs are drawn."""
    k = min(cols, max(k, -(-cols // rows)))
    m = np.zeros((rows, cols))
    m[np.arange(rows)[:, None], (np.arange(rows)[:, None] * k + np.arange(k)[None, :]) % cols] = rng.choice([-1.0, 1.0], size=(rows, k))
    return m


def dense_selection_model(nx, nu, N, seed):
    """one model of rounding_free_dense_case: every matrix a _signed_band, an integer Q, rho = 1"""
    rng = np.random.default_rng([seed, 0])
    return dict(name=f"dense_selection_{nx}_{nu}", nx=nx, nu=nu, N=N, rho=1.0, Kinf=_signed_band(rng, nu, nx), Pinf=_signed_band(rng, nx, nx),
                Quu_inv=_signed_band(rng, nu, nu), AmBKt=_signed_band(rng, nx, nx), Adyn=_signed_band(rng, nx, nx), Bdyn=_signed_band(rng, nx, nu),
                Q=rng.integers(1, 4, size=nx).astype(np.float64), u_min=-16.0, u_max=16.0, x_min=-32.0, x_max=32.0)


def integer_boxes(nx, nu, N, B, seed, per_instance, xlo=16, ulo=8):
    """(x_min, x_max, u_min, u_max): integer bounds of magnitude xlo ... 2 xlo and ulo ... 2 ulo, drawn per (step, row) and each side on its own;
    per_instance: a table per instance"""
    lead = (B,) if per_instance else ()
    box = lambda tag, sign, lo, shape: (sign * np.random.default_rng([seed, tag]).integers(lo, 2 * lo + 1, size=lead + shape)).astype(np.float32)
    return box(4, -1, xlo, (N, nx)), box(5, 1, xlo, (N, nx)), box(6, -1, ulo, (N - 1, nu)), box(7, 1, ulo, (N - 1, nu))


def nonzero_terminal_reference(xref, N, seed):
    """xref (an array, or a (table, start) window) with every row that can be the LAST of a horizon of N redrawn from -2, -1, 1, 2: Pinf multiplies the
    terminal reference row alone, and a zero there would hide an entry of Pinf from the only instance that reads it"""
    table = np.array(xref[0] if isinstance(xref, tuple) else xref)
    last = table[N - 1:] if isinstance(xref, tuple) else table[..., N - 1:, :]     # a window: any row from N - 1 on, by its start
    last[...] = np.random.default_rng([seed, 8]).choice([-2.0, -1.0, 1.0, 2.0], size=last.shape)
    return (table, xref[1]) if isinstance(xref, tuple) else table


def rounding_free_dense_case(nx, nu, N, B, seed, bounds="shared", ref="inst", models=False):
    """(prob, settings, x0, xref, bnds, uref) as rounding_free_case returns them (uref is None: the optional terms live in the row kernels, which
    the fma oracle pins bit for bit), on the same premise — integers through matrices of 0 / +-1, rho = 1, tolerances 0, both bound flags on, so that no
    fp32 operation rounds and an fma, a multiply-then-add, an MFMA accumulation and any summation order give the same VALUE — but with every term of
    every product in play: each matrix is a _signed_band (at least two entries in every row that is two columns wide, no empty column).
    The gains do not stabilise anything, so the values grow with the horizon and with the iterations: the caller keeps N and max_iter small and proves
    the premise by comparing the fp32 with the fp64 exact oracle (tests/test_fma_oracle_host.py).
    The boxes are integers, |u| bound 8 ... 16 and |x| bound 16 ... 32, drawn per (step, row) and each side on its own: the projections bind on a part of
    the entries.  bounds = "inst": a table per instance.  ref = "inst": a reference per instance; "shared": one [N][nx]; "window": xref is a (table,
    start) pair, an integer table of N + 8 rows and a start per instance.  The reference is drawn from -2 ... 2, its terminal row (every row of a
    table that a start makes the terminal one) without the zero: nonzero_terminal_reference.  models: prob is a LIST of B models, instance b's drawn from seed + 1 + b.
    Every array is drawn from a stream of its own, instance by instance: the first B' instances of a case of B are the case of B'."""
    rng = lambda tag: np.random.default_rng([seed, tag])
    prob = [dense_selection_model(nx, nu, N, seed + 1 + b) for b in range(B)] if models else dense_selection_model(nx, nu, N, seed)
    settings = dict(abs_pri_tol=0.0, abs_dua_tol=0.0, check_termination=1, en_state_bound=1, en_input_bound=1)
    x0 = rng(1).integers(-4, 5, size=(B, nx)).astype(np.float32)
    if ref == "window":
        xref = (rng(2).integers(-2, 3, size=(N + 8, nx)).astype(np.float32), rng(3).integers(0, 9, size=B).astype(np.int32))
    else:
        xref = rng(2).integers(-2, 3, size=(N, nx) if ref == "shared" else (B, N, nx)).astype(np.float32)
    return prob, settings, x0, nonzero_terminal_reference(xref, N, seed), integer_boxes(nx, nu, N, B, seed, bounds == "inst"), None


# ---- the cases of tests/test_fma_values_gpu.py; tests/test_fma_oracle_host.py proves what their inputs are worth, from this same list ------------------

def _vc(kernel, dims, select, family, bounds, ref, Bs, max_iters=(1, 2), gen="dense"):
    """kernel: the name the case must run on.  select / family: select_kernel / set_row_kernel.  gen: "dense" rounding_free_dense_case, "sparse"
    rounding_free_case (where the dense values outgrow fp32 in a second iteration of N = 10); "..._pm": one model per instance."""
    return dict(kernel=kernel, dims=dims, select=select, family=family, bounds=bounds, ref=ref, Bs=Bs, max_iters=max_iters, gen=gen)


_ROWS2 = (("shared", "inst"), ("inst", "window"))
_ROWS4 = _ROWS2 + (("shared", "window"), ("inst", "inst"))
# four lanes per instance, N = 10 only: a wave holds sixteen instances (the quad kernel stages one shared bounds table)
QUADLANE_VALUE_CASES = [_vc("quadlane<4,1,10,fast>", (4, 1, 10), 3, 4, "shared", "inst", (1, 17, 37), (1,)),
                        _vc("quadlane<4,1,10,fast>", (4, 1, 10), 3, 4, "shared", "inst", (1, 17, 37), (1, 2), "sparse")]
# one wavefront per instance; (16, 4) and (24, 4) outgrow fp32 in the second iteration of N = 5 (24, 4: in another order of the sums)
WAVERES_VALUE_CASES = [_vc(f"waveres<{d[0]},{d[1]},fast>", d, 3, 7, b, r, (1, 3, 37), mi)
                       for d, mi in (((32, 16, 5), (1, 2)), ((16, 8, 5), (1, 2)), ((20, 8, 5), (1, 2)), ((24, 4, 4), (1, 2)), ((16, 4, 4), (1, 2)),
                                     ((16, 4, 5), (1,)), ((16, 4, 6), (1,)), ((24, 4, 5), (1,))) for b, r in _ROWS2]
# sixteen instances per workgroup: one live column beside a full tile, and ragged
TILE48_VALUE_CASES = [_vc(f"tile48<32,16,{N},fast>", (32, 16, N), 3, 8, b, r, (1, 17, 37)) for N in (4, 5) for b, r in _ROWS4]
# the MFMA streaming kernel, named by its chunks of four rows: five classes with an instantiation of their own, four served by the smallest
# instantiation that contains them (padding rows and columns); tiles of sixteen instances
STREAM_VALUE_CASES = [_vc(k, d, 1, 0, b, r, (17, 37))
                      for k, d in (("stream<3,1>", (12, 4, 5)), ("stream<1,1>", (4, 1, 6)), ("stream<2,1>", (8, 4, 5)), ("stream<8,4>", (32, 16, 5)),
                                   ("stream<16,8>", (64, 32, 4)), ("stream<8,4>", (5, 5, 5)), ("stream<16,8>", (33, 17, 4)), ("stream<3,1>", (10, 3, 4)),
                                   ("stream<2,1>", (6, 2, 4))) for b, r in _ROWS2]
# every instance its own model
# (most dense models of (12, 4) outgrow fp32 within one iteration of N = 10: the dense case of the 16-lane kernel is (8, 3, 7))
MODELS_VALUE_CASES = [_vc("rowlane<8,3,7,fast,pm>", (8, 3, 7), 3, 1, "shared", "inst", (37,), (1,), "dense_pm"),
                      _vc("rowlane<12,4,10,fast,pm>", (12, 4, 10), 3, 1, "inst", "inst", (37,), (1, 2), "sparse_pm"),
                      _vc("waveres<32,16,fast,pm>", (32, 16, 5), 3, 7, "inst", "window", (37,), (1, 2), "dense_pm"),
                      _vc("waveres<16,8,fast,pm>", (16, 8, 5), 3, 7, "shared", "inst", (37,), (1, 2), "dense_pm")]
FMA_VALUE_CASES = QUADLANE_VALUE_CASES + WAVERES_VALUE_CASES + TILE48_VALUE_CASES + STREAM_VALUE_CASES + MODELS_VALUE_CASES
# quadlane's closed loop on chip: two MPC steps of one iteration each
QUADLANE_LOOP_CASE = dict(_vc("quadlane<4,1,10,fast>", (4, 1, 10), 3, 4, "shared", "inst", (1, 17, 37), (1,), "sparse"), steps=2)


def value_case_id(c):
    return "{}-{}-{}-{}".format(c["kernel"], "_".join(map(str, c["dims"])), c["gen"], c["bounds"] + "_" + c["ref"])


_value_inputs = {}
SPARSE_BOXES = (3, 2)   # through selection matrices the values stay small: boxes this narrow bind on a part of the entries


def value_case_inputs(c, B=None):
    """(prob or the list of B per-instance models, settings without max_iter, x0, xref, bnds) of a case at B instances: the first B of the case built
    once at max(c["Bs"]) — every instance's inputs are its own, so what the host tests prove at the largest batch holds for the smaller ones."""
    key = (c["gen"], c["dims"], c["bounds"], c["ref"], max(c["Bs"]))
    if key not in _value_inputs:
        nx, nu, N = c["dims"]
        Bm, pm = max(c["Bs"]), c["gen"].endswith("_pm")
        if c["gen"].startswith("dense"):
            prob, settings, x0, xref, bnds, _ = rounding_free_dense_case(nx, nu, N, Bm, 0, bounds=c["bounds"], ref=c["ref"], models=pm)
        else:   # the sparse generator draws a per-instance reference; its boxes (+-50, +-3: the states never reach theirs) are replaced
            prob, settings, x0, xref, bnds, _ = rounding_free_case(nx, nu, N, Bm, 0)
            assert c["ref"] == "inst"
            xref = nonzero_terminal_reference(xref, N, 0)
            # one term per row: a zero of x0 would hide the entry of Adyn or Kinf that multiplies it from the only instance that reads the model
            x0 = np.where(x0 == 0, np.random.default_rng([0, 9]).choice([-1.0, 1.0], size=x0.shape), x0).astype(np.float32)
            bnds = integer_boxes(nx, nu, N, Bm, 0, c["bounds"] == "inst", *SPARSE_BOXES)
            if pm:
                # models of seeds 300 ... 336: now and then a selection model outgrows fp32 in the second iteration of N = 10; of these 37 none does
                # (largest magnitude 2.8e5, below 2^19), which tests/test_fma_oracle_host.py proves on the oracle for each of them
                prob = [rounding_free_case(nx, nu, N, 1, 300 + b)[0] for b in range(Bm)]
        _value_inputs[key] = (prob, settings, x0, xref, bnds)
    prob, settings, x0, xref, bnds = _value_inputs[key]
    B = B or max(c["Bs"])
    cut = lambda a, shared_ndim: a if a.ndim == shared_ndim else a[:B]
    xref = (xref[0], xref[1][:B]) if isinstance(xref, tuple) else cut(xref, 2)
    return (prob[:B] if isinstance(prob, list) else prob), settings, x0[:B], xref, tuple(cut(b, 2) for b in bnds)


def models_of(probs):
    """the dict TinyBatchSolver.set_models takes, from one prob-style model per instance"""
    mods = {k: np.array([p[k] for p in probs]) for k in PROB_KEYS}
    mods["rho"] = np.array([p["rho"] for p in probs])
    return mods


def value_case_oracle(O, probs, dtype, settings, x0, xref, bnds, arith="exact"):
    """(rc, state) of one cold solve of a value case on the CPU oracle; a list of models: every instance with its own.  fp64 is the proof that nothing
    rounds, where the order of a sum is immaterial: every dimension is accepted."""
    dt = np.float64 if dtype == np.float64 else np.float32
    B, pm = len(x0), isinstance(probs, list)
    p0 = probs[0] if pm else probs
    nx, nu, N = p0["nx"], p0["nu"], p0["N"]
    xr = np.asarray(ref_at(xref, 0, 0, N, B), dt)
    bnds = [np.asarray(b, dt) for b in bnds]
    st = O.new_state(B, nx, nu, N, dt)
    st["x"][:, 0] = x0
    if not pm:
        return O.Oracle(probs, dtype, settings, arith=arith, allow_unpinned_dims=True).solve(st, *bnds, xr), st
    rc = 0
    for b, p in enumerate(probs):
        sub = {k: np.ascontiguousarray(v[b:b + 1]) for k, v in st.items()}
        rc += O.Oracle(p, dtype, settings, arith=arith, allow_unpinned_dims=True).solve(sub, *[a[b:b + 1] if a.ndim == 3 else a for a in bnds],
                                                                                       np.ascontiguousarray(xr[b:b + 1] if xr.ndim == 3 else xr))
        for k in st:
            st[k][b] = sub[k][0]
    return rc, st
