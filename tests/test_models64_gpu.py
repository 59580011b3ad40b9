"""Per-instance models of the fp64 library (tiny_batch64_set_models / _set_systems / _clear_models), bit for bit against the fp64 oracle run once per
distinct model over that model's instances: the signs of zeros, all twelve work arrays, the four residual fields, status and iter.

One solve on every sixteen-lane family and on the thread-per-instance kernel (two solves per row: cold, then warm from the first's workspace with a
new x0), the replicated model against the shared path, the closed loop driven three ways as tests/test_sim_loop64_gpu.py drives it (against a loop
of one Oracle per distinct model, the plant step from the instance's own model where no plant is set), set_systems against set_models, the refused
step calls.  tests/test_models64_host.py checks on the CPU that every row's inputs meet the conditions the comparisons rely on."""
import numpy as np
import pytest

from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_conditions, closed_loop_inputs, ref_at, same_bits
from test_closed_loop_gpu import BASE, _first_diff
from test_sim_loop64_gpu import K1, STEPS, _slide, plant_fn

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3  # TINY_BATCH_EINVAL, TINY_BATCH_EUNSUPPORTED
MODEL_KEYS = ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn", "Q")


def _solve_row(name, dims, B, nm, settings=None, kernel=0, pib=False):
    """name: what kernel_name() reports with the models set; nm: distinct models; pib: per-instance bounds; kernel: select_kernel's argument"""
    return dict(name=name, dims=dims, B=B, nm=nm, settings=settings or {}, kernel=kernel, pib=pib, ref="inst", adv=0, plant=None, w=False)


SOLVE_ROWS = [
    _solve_row("rows64<12,4,10,pm>", (12, 4, 10), 130, 7),                               # more than one wave, the last one partial
    _solve_row("rows64<12,4,30,pm>", (12, 4, 30), 9, 4, pib=True),                       # slack in LDS, the most scratch
    _solve_row("rows64<12,4,20,pm>", (12, 4, 20), 5, 5),
    _solve_row("rows64<4,1,10,pm>", (4, 1, 10), 130, 7, dict(check_termination=3)),
    _solve_row("rows64<8,4,9,pm>", (8, 4, 9), 5, 3),
    _solve_row("rows64<12,2,n<=32,pm>", (12, 2, 13), 37, 5),
    _solve_row("rows64<4,4,n<=32,pm>", (4, 4, 32), 5, 3),                                # the capacity edge
    _solve_row("rows64<12,4,n<=64,pm>", (12, 4, 40), 5, 3),                              # [p ; d] written through
    _solve_row("thread64<16,4,pm>", (16, 4, 10), 130, 7),
    _solve_row("thread64<12,4,pm>", (12, 4, 10), 65, 4, kernel=1),
    _solve_row("rows64<12,4,10,pm>", (12, 4, 10), 5, 3, dict(max_iter=1)),
]
# max_iter = 0: tiny_solve sets status and iter and computes nothing, so no condition on the inputs can hold; the rows are here for the early return
ZERO_ITER_ROWS = [_solve_row("rows64<12,4,10,pm>", (12, 4, 10), 5, 3, dict(max_iter=0)), _solve_row("thread64<16,4,pm>", (16, 4, 10), 65, 3, dict(max_iter=0))]


def _loop_row(name, dims, B, nm, ref, adv, plant, w, **kw):
    """name: what closed_loop_kernel_name() reports with the models and the row's plant set"""
    return dict(name=name, dims=dims, B=B, nm=nm, settings={}, kernel=0, pib=False, ref=ref, adv=adv, plant=plant, w=w, **kw)


LOOP_ROWS = [
    _loop_row("rows64<12,4,10,mpc,pm>", (12, 4, 10), 130, 7, "window", 1, None, False),
    _loop_row("rows64<12,4,10,sim,pm>", (12, 4, 10), 5, 3, "window", 1, "inst", True),
    _loop_row("rows64<12,4,30,sim,pm>", (12, 4, 30), 5, 3, "window", 2, "shared", True, near_end=True),
    _loop_row("rows64<4,1,10,mpc,pm>", (4, 1, 10), 130, 7, "shared", 0, None, False),    # nx < 8: the lazy order
    _loop_row("rows64<8,4,9,mpc,pm>", (8, 4, 9), 3, 3, "window", 1, None, True),         # w only
    _loop_row("rows64<12,2,n<=32,mpc,pm>", (12, 2, 13), 37, 5, "window", 1, None, False),
    _loop_row("rows64<12,4,n<=64,pm>", (12, 4, 40), 5, 3, "window", 1, None, True),      # launch sequence
    _loop_row("thread64<16,4,pm>", (16, 4, 10), 130, 7, "window", 1, None, False),       # launch sequence, no rows kernel
]
for _i, _r in enumerate(SOLVE_ROWS + ZERO_ITER_ROWS):
    _r["id"] = "solve{}-{}_{}_{}-B{}-nm{}{}".format(_i + 1, *_r["dims"], _r["B"], _r["nm"], "".join(f"-{k}{v}" for k, v in _r["settings"].items()))
for _i, _r in enumerate(LOOP_ROWS):
    _r["id"] = "loop{}-{}_{}_{}-B{}-{}{}-plant_{}{}".format(_i + 1, *_r["dims"], _r["B"], _r["ref"], _r["adv"], _r["plant"], "-w" if _r["w"] else "")

# x0 amplitudes / bound scales (helpers.closed_loop_inputs) where the stock ones do not meet the conditions of tests/test_models64_host.py, found on the
# CPU with the oracle alone
TUNED = {}


# ---- inputs and the reference: shared with tests/test_models64_host.py ----------------------------------------------------------------------------

_inputs = {}


def row_inputs(pr, O, r):
    """everything a row runs on, built once.  The recipe: fam = model_family("random", nm, B, seed = 7 + nx, dims = (nx, nu)), its caches from the
    oracle's Riccati, the class's stock bounds from random_system(nx, nu, N, seed = 100 nx + nu), helpers.closed_loop_inputs on model 0 with seed
    4242 + nx in float64, the settings BASE.  x0b: the second solve's x0.  Per-instance bounds: the shared ones scaled by a draw in [0.6, 1] per
    instance.  Plant (tests/test_sim_loop64_gpu.py's recipe on every instance's own model): A_p = A (1 + 0.05 n), B_p = B (1 + 0.05 n) entry-wise, a
    shared plant is instance 0's; w = 0.01 n."""
    if r["id"] in _inputs:
        return _inputs[r["id"]]
    nx, nu, N = r["dims"]
    B = r["B"]
    fam = pr.model_family("random", r["nm"], B, seed=7 + nx, dims=(nx, nu))
    mods = pr.family_caches(fam, riccati=O.riccati)
    base = pr.random_system(nx, nu, N, seed=100 * nx + nu, riccati=O.riccati)
    probs = [dict(p, N=N, **{k: base[k] for k in ("u_min", "u_max", "x_min", "x_max")}) for p in mods["probs"]]
    seed = 4242 + nx
    tuned = TUNED.get(r["id"], {})
    x0, ref, bnds = closed_loop_inputs(probs[0], B, r["ref"], seed, near_end=bool(r.get("near_end")), dtype=np.float64, **tuned)
    x0b = closed_loop_inputs(probs[0], B, "shared", seed + 17, dtype=np.float64, **tuned)[0]
    rng = np.random.default_rng(seed + 1)
    A, Bm = np.asarray(mods["Adyn"], np.float64), np.asarray(mods["Bdyn"], np.float64)
    Ap = A * (1 + 0.05 * rng.standard_normal(A.shape))
    Bp = Bm * (1 + 0.05 * rng.standard_normal(Bm.shape))
    w = 0.01 * rng.standard_normal((STEPS, B, nx))
    if r["pib"]:
        s = rng.uniform(0.6, 1.0, size=(B, 1, 1))
        bnds = tuple(np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape) * s) for a in bnds)
    plant = None if r["plant"] is None else (Ap[0], Bp[0]) if r["plant"] == "shared" else (Ap, Bp)
    out = dict(fam=fam, mods={k: mods[k] for k in MODEL_KEYS + ("rho",)}, probs=probs, model=fam["model"], settings=dict(BASE, **r["settings"]),
               x0=x0, x0b=x0b, ref=ref, bnds=bnds, plant=plant, w=w if r["w"] else None)
    _inputs[r["id"]] = out
    return out


def oracle_solve(O, probs, model, settings, st, bnds, xref):
    """tiny_solve on the fp64 oracle, once per distinct model over that model's instances, in place"""
    for m, p in enumerate(probs):
        idx = np.nonzero(model == m)[0]
        if idx.size == 0:
            continue
        sub = {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}
        b = [np.ascontiguousarray(a[idx]) if a.ndim == 3 else a for a in bnds]
        O.Oracle(p, np.float64, settings).solve(sub, *b, np.ascontiguousarray(xref[idx]) if xref.ndim == 3 else xref, nthreads=8)
        for k in st:
            st[k][idx] = sub[k]
    return st


def own_plant_step(O, probs, model, x, u0):
    """x.col(0) <- Adyn x.col(0) + Bdyn u.col(0) with every instance's own model, in the oracle's order"""
    xn = np.empty_like(x)
    for m, p in enumerate(probs):
        idx = np.nonzero(model == m)[0]
        if idx.size:
            xn[idx] = O.Oracle(p, np.float64).plant_step(np.ascontiguousarray(x[idx]), np.ascontiguousarray(u0[idx]))
    return xn


def two_solves(O, inp, model=None):
    """the cold solve and the warm one with the new x0; model: the model index of every instance (default: the row's own)"""
    nx, nu, N, B = inp["probs"][0]["nx"], inp["probs"][0]["nu"], inp["probs"][0]["N"], len(inp["x0"])
    model = inp["model"] if model is None else model
    st = O.new_state(B, nx, nu, N, np.float64)
    st["x"][:, 0] = inp["x0"]
    oracle_solve(O, inp["probs"], model, inp["settings"], st, inp["bnds"], inp["ref"])
    first = O.copy_state(st)
    st["x"][:, 0] = inp["x0b"]
    oracle_solve(O, inp["probs"], model, inp["settings"], st, inp["bnds"], inp["ref"])
    return first, st


def models_oracle_loop(O, inp, r, steps=STEPS, model=None):
    """tests/test_sim_loop64_gpu.py's sim_oracle_loop with one Oracle per distinct model: per step y = g = 0, tiny_solve, x = plant(x, u0) — the row's
    plant, or every instance's own Adyn / Bdyn without one — then x = x + w[k]"""
    p0 = inp["probs"][0]
    nx, nu, N, B = p0["nx"], p0["nu"], p0["N"], len(inp["x0"])
    model = inp["model"] if model is None else model
    step = plant_fn(O, p0, inp["plant"]) if inp["plant"] is not None else (lambda x, u0: own_plant_step(O, inp["probs"], model, x, u0))
    st = O.new_state(B, nx, nu, N, np.float64)
    x = np.array(inp["x0"], np.float64)
    out = dict(u0=[], iter=[], status=[], xs=[])
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        oracle_solve(O, inp["probs"], model, inp["settings"], st, inp["bnds"], ref_at(inp["ref"], k, r["adv"], N, B))
        u0 = st["u"][:, 0].copy()
        out["u0"].append(u0); out["iter"].append(st["iter"].copy()); out["status"].append(st["status"].copy())
        x = np.asarray(step(x, u0), np.float64)
        if inp["w"] is not None:
            x = x + np.asarray(inp["w"][k], np.float64)
        out["xs"].append(x.copy())
    st["x"][:, 0] = x
    return dict(u0=np.array(out["u0"]), iter=np.array(out["iter"]), status=np.array(out["status"]), xs=np.array(out["xs"]), x=x, st=st)


_references = {}


def _reference(T, O, r, loop):
    """computed once per row and shared by the tests that need it; nobody writes to it"""
    if r["id"] not in _references:
        inp = row_inputs(T.problems, O, r)
        if loop:
            want = models_oracle_loop(O, inp, r)
            closed_loop_conditions(want, inp["bnds"], inp["settings"], r["id"])
        else:
            want = two_solves(O, inp)
        _references[r["id"]] = (inp, want)
    return _references[r["id"]]


# ---- driving a handle ---------------------------------------------------------------------------------------------------------------------------

def _shared_name(name):
    return name.replace(",pm>", ">")


def _handle(T, r, inp, models=True, plant=True):
    s = T.TinyBatchSolver64(inp["probs"][0], r["B"], settings=inp["settings"])
    s.select_kernel(r["kernel"])
    s.set_bounds(*inp["bnds"])
    if isinstance(inp["ref"], tuple):
        s.set_xref_window(*inp["ref"])
    else:
        s.set_xref(inp["ref"])
    s.set_x0(inp["x0"])
    assert not s.models_per_instance()
    if models:
        s.set_models(inp["mods"])
        assert s.models_per_instance()
    if plant and inp["plant"] is not None:
        s.set_plant(*inp["plant"])
    return s


def _check_state(s, want, what):
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs from the oracle ({s.kernel_name()})"


# ---- 1. heterogeneous one solve -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", SOLVE_ROWS + ZERO_ITER_ROWS, ids=[r["id"] for r in SOLVE_ROWS + ZERO_ITER_ROWS])
def test_heterogeneous_solve_equals_the_oracle_per_model(tinympc, oracle_mod, row):
    inp, (first, second) = _reference(tinympc, oracle_mod, row, loop=False)
    s = _handle(tinympc, row, inp)
    assert s.kernel_name() == row["name"], s.kernel_name()
    rc = s.solve()
    assert rc == int((first["status"] != 1).any())
    _check_state(s, first, row["id"] + " cold")
    s.set_x0(inp["x0b"])
    rc = s.solve()
    assert rc == int((second["status"] != 1).any())
    _check_state(s, second, row["id"] + " warm")
    s.close()


# ---- 2. the same model everywhere is the shared path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [SOLVE_ROWS[0], SOLVE_ROWS[5], SOLVE_ROWS[8]], ids=[SOLVE_ROWS[i]["id"] for i in (0, 5, 8)])
def test_the_replicated_model_is_the_shared_path(tinympc, oracle_mod, row):
    T, r = tinympc, row
    inp = row_inputs(T.problems, oracle_mod, r)
    p0, B = inp["probs"][0], r["B"]
    rep = {k: np.broadcast_to(np.asarray(p0[k], np.float64), (B,) + np.asarray(p0[k]).shape) for k in MODEL_KEYS}
    rep["rho"] = np.full(B, p0["rho"])
    shared = _handle(T, r, inp, models=False)
    assert shared.kernel_name() == _shared_name(r["name"])
    shared.solve()
    want = shared.get_state()
    shared.close()
    s = _handle(T, r, inp, models=False)
    s.set_models(rep)
    assert s.models_per_instance() and s.kernel_name() == r["name"]
    s.solve()
    _check_state(s, want, r["id"] + " replicated")
    # other models in between, then back to the handle's own through clear_models: a cold workspace again
    s.set_models(inp["mods"])
    s.clear_models()
    assert not s.models_per_instance() and s.kernel_name() == _shared_name(r["name"])
    for k in STATE_ORDER:
        s.set_array(k, np.zeros_like(want[k]))
    s.set_state(dict(iter=np.zeros(B, np.int32), status=np.zeros(B, np.int32), residuals=np.zeros((B, 4))))
    s.set_x0(inp["x0"])
    s.solve()
    _check_state(s, want, r["id"] + " after clear_models")
    s.close()


# ---- 3. the closed loop ----------------------------------------------------------------------------------------------------------------------------

def _check_final(s, r, ref, want, what, starts=True):
    _check_state(s, want["st"], what + " after the last step")
    assert same_bits(s.first_columns()[0], want["x"]), f"{what}: x.col(0) differs after the last step"
    if isinstance(ref, tuple) and starts:
        assert np.array_equal(s.xref_start(), ref[1] + STEPS * r["adv"]), f"{what}: the window starts after the run"


def _run(s, r, inp, chunks, want, what):
    us, xs, k, w = [], [], 0, inp["w"]
    for n in chunks:
        u, x = s.mpc_run_sim(n, r["adv"], None if w is None else w[k:k + n])
        k += n
        it, stt, _ = s.get_status()
        assert np.array_equal(it, want["iter"][k - 1]) and np.array_equal(stt, want["status"][k - 1]), f"{what}: iter / status differ after step {k - 1}"
        us.append(u); xs.append(x)
    us, xs = np.concatenate(us), np.concatenate(xs)
    assert same_bits(us, want["u0"]), f"{what}: u.col(0) differs from step {_first_diff(us, want['u0'])} on"
    assert same_bits(xs, want["xs"]), f"{what}: x_traj differs from step {_first_diff(xs, want['xs'])} on"
    _check_final(s, r, inp["ref"], want, what)


def _step(s, r, inp, want, what):
    w, ref, has_window = inp["w"], inp["ref"], isinstance(inp["ref"], tuple)
    for k in range(STEPS):
        rc = s.mpc_step_sim(None if w is None else w[k]) if (w is not None or k % 2) else s.mpc_step()
        assert rc == int((want["status"][k] != 1).any()), f"{what}: the step returns what its solve returns (step {k})"
        it, stt, _ = s.get_status()
        assert np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"{what}: iter / status differ after step {k}"
        x0, u0 = s.first_columns()
        assert same_bits(u0, want["u0"][k]), f"{what}: u.col(0) differs at step {k}"
        assert same_bits(x0, want["xs"][k]), f"{what}: x.col(0) differs after step {k}"
        if isinstance(ref, tuple) and r["adv"]:
            has_window = _slide(s, ref, k + 1, r["adv"], s.N, s.B)
    _check_final(s, r, ref, want, what, starts=has_window)


@pytest.mark.parametrize("row", LOOP_ROWS, ids=[r["id"] for r in LOOP_ROWS])
def test_closed_loop_equals_the_oracle_loop_per_model(tinympc, oracle_mod, row):
    T, r = tinympc, row
    inp, want = _reference(T, oracle_mod, r, loop=True)
    for way, chunks in (("run", (K1, STEPS - K1)), ("step by step", None), ("run with a single step", (K1, 1, STEPS - K1 - 1))):
        s = _handle(T, r, inp)
        assert s.closed_loop_kernel_name() == r["name"], s.closed_loop_kernel_name()
        what = f"{r['id']} {way}"
        if chunks:
            _run(s, r, inp, chunks, want, what)
        else:
            _step(s, r, inp, want, what)
        s.close()


@pytest.mark.parametrize("row", [LOOP_ROWS[0], LOOP_ROWS[7]], ids=[LOOP_ROWS[i]["id"] for i in (0, 7)])
def test_the_nominal_run_calls_take_the_models(tinympc, oracle_mod, row):
    """mpc_run_traj and mpc_run (no w, no x_traj) with models set: the same loop"""
    T, r = tinympc, row
    inp, want = _reference(T, oracle_mod, r, loop=True)
    s = _handle(T, r, inp)
    traj = np.concatenate([s.mpc_run_traj(K1, r["adv"]), s.mpc_run_traj(STEPS - K1, r["adv"])])
    assert same_bits(traj, want["u0"]), f"u.col(0) differs from step {_first_diff(traj, want['u0'])} on"
    _check_final(s, r, inp["ref"], want, r["id"] + " mpc_run_traj")
    s.close()
    s = _handle(T, r, inp)
    s.mpc_run(K1, r["adv"]); s.mpc_run(1, r["adv"]); s.mpc_run(STEPS - K1 - 1, r["adv"])
    _check_final(s, r, inp["ref"], want, r["id"] + " mpc_run")
    s.close()


# ---- 4. set_systems ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [SOLVE_ROWS[0], SOLVE_ROWS[8]], ids=[SOLVE_ROWS[i]["id"] for i in (0, 8)])
def test_set_systems_is_set_models_of_the_host_caches(tinympc, oracle_mod, row):
    """the device Riccati is bitwise the library's host tiny_riccati (not the oracle's restatement, whose caches differ in the last bits): the
    reference is the handle that takes problems.family_caches(fam) through set_models, and the oracle on those caches"""
    T, O, r = tinympc, oracle_mod, row
    inp = row_inputs(T.problems, O, r)
    fam, B = inp["fam"], r["B"]
    mods = T.problems.family_caches(fam)
    probs = [dict(p, **{k: q[k] for k in MODEL_KEYS[:4]}) for p, q in zip(inp["probs"], mods["probs"])]
    first, _ = two_solves(O, dict(inp, probs=probs))
    b = _handle(T, r, dict(inp, mods={k: mods[k] for k in MODEL_KEYS + ("rho",)}))
    b.solve()
    _check_state(b, first, r["id"] + " set_models of the host caches")
    want = b.get_state()
    b.close()
    s = _handle(T, r, inp, models=False)
    it = s.set_systems(fam["A"], fam["B"], fam["Q"], fam["R"], fam["rho"])
    assert s.models_per_instance() and s.kernel_name() == r["name"]
    assert np.array_equal(it, np.array([p["iters"] for p in _host_riccati(T, fam)])[fam["model"]])
    s.solve()
    _check_state(s, want, r["id"] + " set_systems")
    # a singular system (R = -rho and B = 0 give R1 = 0): refused, the models stay
    R, Bm = fam["R"].copy(), fam["B"].copy()
    Bm[3] = 0.0; R[3] = -fam["rho"][3]
    with pytest.raises(T.TinyBatchError, match="singular"):
        s.set_systems(fam["A"], Bm, fam["Q"], R, fam["rho"])
    assert s.lib.tiny_batch64_set_systems(s._h, *[s._dp(np.ascontiguousarray(a)) for a in (fam["A"], Bm, fam["Q"], R, fam["rho"])], None) == EINVAL
    assert s.models_per_instance()
    for k in STATE_ORDER:
        s.set_array(k, np.zeros_like(want[k]))
    s.set_state(dict(iter=np.zeros(B, np.int32), status=np.zeros(B, np.int32), residuals=np.zeros((B, 4))))
    s.set_x0(inp["x0"])
    s.solve()
    _check_state(s, want, r["id"] + " after a refused set_systems")
    s.close()


def _host_riccati(T, fam):
    ms = fam["models"]
    nx, nu = ms["A"].shape[1], ms["B"].shape[2]
    return [T.riccati(nx, nu, ms["A"][m], ms["B"][m], ms["Q"][m], ms["R"][m], ms["rho"][m]) for m in range(len(ms["rho"]))]


def test_set_models_device_takes_device_arrays(tinympc, oracle_mod):
    """tiny_batch64_set_models_device on the eight [B] arrays as device buffers (column-major per instance, as set_models uploads them): the oracle's
    result, and again after the buffers have been overwritten and released — the records are the handle's own"""
    import ctypes as C
    from accelerated_tinympc_amd import solver as S
    T, r = tinympc, SOLVE_ROWS[5]
    inp, (first, _) = _reference(T, oracle_mod, r, loop=False)
    B, mods = r["B"], inp["mods"]
    host = [np.ascontiguousarray(np.asarray(mods["rho"], np.float64).reshape(B))]
    host += [S._colmajor_batch(mods[k], np.float64) for k in MODEL_KEYS[:6]] + [np.ascontiguousarray(np.asarray(mods["Q"], np.float64).reshape(B, r["dims"][0]))]
    hip, dev = S._hip(), []
    s = _handle(T, r, inp, models=False)
    try:
        for a in host:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), a.nbytes) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
            dev.append(p)
        assert s.lib.tiny_batch64_set_models_device(s._h, *dev) == 0
        assert s.models_per_instance() and s.kernel_name() == r["name"]
        s.solve()  # (waits for the gather: the null stream orders them)
        _check_state(s, first, r["id"] + " set_models_device")
        junk = np.full(max(a.size for a in host), np.nan)
        for a, p in zip(host, dev):
            assert hip.hipMemcpy(p, junk.ctypes.data, a.nbytes, 1) == 0
    finally:
        for p in dev:
            hip.hipFree(p)
    assert s.lib.tiny_batch64_set_models_device(s._h, *([None] * 8)) == EINVAL and s.models_per_instance()
    for k in STATE_ORDER:
        s.set_array(k, np.zeros_like(first[k]))
    s.set_state(dict(iter=np.zeros(B, np.int32), status=np.zeros(B, np.int32), residuals=np.zeros((B, 4))))
    s.set_x0(inp["x0"])
    s.solve()
    _check_state(s, first, r["id"] + " after the caller's buffers are gone")
    s.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_the_step_calls_are_refused_while_models_are_set(tinympc, oracle_mod):
    T, r = tinympc, SOLVE_ROWS[4]
    inp = row_inputs(T.problems, oracle_mod, r)
    s = _handle(T, r, inp)
    lib = s.lib
    conv = np.zeros(r["B"], np.int32)
    calls = [lambda: lib.tiny_batch64_forward_pass(s._h), lambda: lib.tiny_batch64_update_slack(s._h), lambda: lib.tiny_batch64_update_dual(s._h),
             lambda: lib.tiny_batch64_update_linear_cost(s._h), lambda: lib.tiny_batch64_backward_pass_grad(s._h),
             lambda: lib.tiny_batch64_termination_condition(s._h, conv.ctypes.data_as(lib.tiny_batch64_termination_condition.argtypes[1]))]
    before = s.get_state()
    for k, fn in enumerate(calls):
        assert fn() == EUNSUPPORTED, k
        assert "per-instance models" in lib.tiny_batch64_last_error().decode(), k
    after = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(before[k], after[k]), f"{k} changed by a refused call"
    s.clear_models()
    for k, fn in enumerate(calls):
        assert fn() == 0, k
    s.close()
