"""Closed-loop runs against a separate plant, with a disturbance and the state trajectory (tiny_batch_set_plant, tiny_batch_mpc_run_sim*,
tiny_batch_mpc_step_sim_async), bit for bit against a loop computed elsewhere: u.col(0) and x0 of every step, iter and status per step, the twelve
work arrays, the residuals and x0 after the last.

The reference of exact arithmetic with fp32 storage is the oracle's loop (sim_oracle_loop: helpers.oracle_closed_loop with the plant step of an
Oracle built on the plant's matrices, then one rounded add of w[k]); fma arithmetic and fp16 storage compare with the loop driven from the host on a
second handle (helpers.host_closed_loop) whose plant callable is that oracle's.  Every case is driven three ways: mpc_run_sim in chunks (3, 5),
8 x mpc_step_sim, and chunks (3, 1, 4) — the off-by-one place of the host's last plant step, w[steps - 1] and x_traj[steps - 1].
tests/test_sim_loop_host.py checks on the CPU that every case's inputs meet the conditions and that its trajectory leaves the nominal one."""
import ctypes as C

import numpy as np
import pytest

import test_closed_loop_gpu as G
from helpers import (GOLDEN, SCALAR_ORDER, STATE_ORDER, closed_loop_case, closed_loop_conditions, closed_loop_inputs, host_closed_loop, oracle_closed_loop,
                     positive_system, ref_at, rows_of_negative_zeros, same_bits, zero_state_inputs)

pytestmark = pytest.mark.gpu

STEPS, K1 = 8, 3
BASE = G.BASE


def _case(name, dims, B, ref, plant, w, row=1, arith="exact", onchip=True, **kw):
    """plant: None (the model's), "shared" or "inst"; w: with a disturbance; row: set_row_kernel's family; onchip: one launch per run"""
    c = dict(name=name, dims=dims, B=B, ref=ref, adv=1 if ref == "window" else 0, plant=plant, w=w, row=row, arith=arith, onchip=onchip, settings={}, **kw)
    c["id"] = "{}-B{}-{}-plant_{}{}".format(name, B, ref, plant, "-w" if w else "") + ("-" + "_".join(f"{k}{v}" for k, v in c["settings"].items()) if c["settings"] else "")
    return c


ONCHIP_CASES = [
    _case("rowlane<12,4,10,exact>", (12, 4, 10), 5, "window", "shared", True),
    _case("rowlane<12,4,10,exact>", (12, 4, 10), 5, "window", "inst", True),
    _case("rowlane<12,4,10,exact>", (12, 4, 10), 5, "window", None, True),                  # the disturbance alone: the model's own rows in the SIM kernel
    _case("rowlane<8,3,7,exact>", (8, 3, 7), 5, "inst", "inst", False),
    _case("rowlane<4,1,10,exact>", (4, 1, 10), 5, "shared", "shared", False),               # nx < 8: the lazy product's order
    dict(_case("rowlane<12,4,30,exact>", (12, 4, 30), 5, "window", "inst", True), settings=dict(max_iter=1)),   # the headline horizon, the spilling instantiation
    _case("rowlane<12,4,10,exact,pm>", (12, 4, 10), 5, "window", "inst", True, pm=True),
]
ONCHIP_CASES[5]["id"] += "-max_iter1"
FMA_CASE = _case("rowlane<12,4,10,fast>", (12, 4, 10), 5, "window", "inst", True, arith="fast", quadrotor=True)
REPLAY_CASES = [
    _case("rowloop<12,4,exact>", (12, 4, 12), 5, "inst", "shared", True, row=2, onchip=False),
    _case("rowloop<4,2,exact>", (4, 2, 8), 130, "shared", "inst", True, row=2, onchip=False),        # past the plant kernel's block of 128
    _case("waveres<16,8,exact>", (16, 8, 10), 3, "shared", "shared", True, row=7, onchip=False),    # both products through the GEMV accumulator
    _case("quadlane<4,1,10,exact>", (4, 1, 10), 5, "shared", "shared", False, row=0, onchip=False),  # its nominal loop is on chip, the simulated one replayed
    _case("rowlane<12,4,30,exact,h16d>", (12, 4, 30), 5, "window", "inst", True, onchip=False, storage=(16, None)),
]
HANDOVER_CASE = _case("tile16<12,4,30,exact>", (12, 4, 30), 17, "window", "shared", True, row=5, loop="rowlane<12,4,30,exact>")
ALL_CASES = ONCHIP_CASES + [FMA_CASE] + REPLAY_CASES + [HANDOVER_CASE]
assert len({c["id"] for c in ALL_CASES}) == len(ALL_CASES)

# x0 amplitudes / bound scales where the stock ones of helpers.closed_loop_inputs do not meet the conditions, found on the CPU with the oracle's loop alone
TUNED = {}
assert set(TUNED) <= {c["id"] for c in ALL_CASES}


def _ids(cases):
    return [c["id"] for c in cases]


# ---- inputs and the reference loop: shared with tests/test_sim_loop_host.py --------------------------------------------------------------------

def case_models(pr, O, c):
    """(probs, model, mods): the distinct models' prob dicts, the model index of every instance and, for a per-instance-model case, set_models' arrays"""
    nx, nu, N = c["dims"]
    if c.get("pm"):
        fam = pr.model_family("quadrotor", 3, c["B"], seed=3)
        mods = pr.family_caches(fam)
        probs = [dict(p, N=N, u_min=-0.5, u_max=0.5, x_min=-5.0, x_max=5.0) for p in mods["probs"]]
        return probs, fam["model"], mods
    return [G.case_problem(pr, O, c)], np.zeros(c["B"], np.int64), None


_cache = {}


def case_inputs(pr, O, c):
    """everything a case runs on, built once: probs / model / mods, settings, x0, ref, bnds, the plant (A_p, B_p) in the case's mode, w.
    The recipe: helpers.closed_loop_inputs with seed 4242 + nx; from default_rng(seed + 1) A_p = A (1 + 0.05 n), B_p = B (1 + 0.05 n) entry-wise per
    instance (a shared plant is instance 0's), w = 0.01 n; all fp32."""
    if c["id"] in _cache:
        return _cache[c["id"]]
    nx, nu, N = c["dims"]
    B = c["B"]
    probs, model, mods = case_models(pr, O, c)
    seed = 4242 + nx
    x0, ref, bnds = closed_loop_inputs(probs[0], B, c["ref"], seed, **TUNED.get(c["id"], {}))
    rng = np.random.default_rng(seed + 1)
    A = np.stack([np.asarray(probs[m]["Adyn"], np.float64) for m in model])
    Bm = np.stack([np.asarray(probs[m]["Bdyn"], np.float64) for m in model])
    Ap = (A * (1 + 0.05 * rng.standard_normal(A.shape))).astype(np.float32)
    Bp = (Bm * (1 + 0.05 * rng.standard_normal(Bm.shape))).astype(np.float32)
    w = (0.01 * rng.standard_normal((STEPS, B, nx))).astype(np.float32)
    plant = None if c["plant"] is None else (Ap[0], Bp[0]) if c["plant"] == "shared" else (Ap, Bp)
    out = dict(probs=probs, model=model, mods=mods, settings=dict(BASE, **c["settings"]), x0=x0, ref=ref, bnds=bnds, plant=plant, w=w if c["w"] else None)
    _cache[c["id"]] = out
    return out


def plant_fn(O, probs, model, plant):
    """x, u0 -> the plant step of every instance in the oracle's (= the reference's) order: Oracle(dict(prob, Adyn = A_p, Bdyn = B_p)).plant_step, one
    oracle for a shared plant, one per instance otherwise; plant = None: every instance's own model"""
    if plant is not None and plant[0].ndim == 2:
        orc = O.Oracle(dict(probs[0], Adyn=plant[0], Bdyn=plant[1]), np.float32)
        return orc.plant_step
    if plant is None:
        if len(probs) == 1:
            return O.Oracle(probs[0], np.float32).plant_step
        orcs = [O.Oracle(p, np.float32) for p in probs]
        each = [orcs[m] for m in model]
    else:
        each = [O.Oracle(dict(probs[0], Adyn=a, Bdyn=b), np.float32) for a, b in zip(*plant)]
    return lambda x, u0: np.concatenate([o.plant_step(x[b:b + 1], u0[b:b + 1]) for b, o in enumerate(each)])


def sim_oracle_loop(O, probs, model, settings, x0, ref, bnds, steps, adv, plant=None, w=None):
    """helpers.oracle_closed_loop against a separate plant: per step y = g = 0, tiny_solve (every instance with its own model), x = plant(x, u0), then
    x = fp32(x + w[k]).  Records xs, the state after every plant step."""
    p0 = probs[0]
    nx, nu, N, B = p0["nx"], p0["nu"], p0["N"], len(x0)
    orcs = [O.Oracle(p, np.float32, settings) for p in probs]
    step = plant_fn(O, probs, model, plant)
    st = O.new_state(B, nx, nu, N, np.float32)
    x = np.array(x0, np.float32)
    out = dict(u0=[], iter=[], status=[], xs=[])
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        xr = ref_at(ref, k, adv, N, B)
        if len(orcs) == 1:
            orcs[0].solve(st, *bnds, xr, nthreads=8)
        else:
            for m, orc in enumerate(orcs):
                idx = np.nonzero(model == m)[0]
                if idx.size:
                    sub = {key: np.ascontiguousarray(v[idx]) for key, v in st.items()}
                    orc.solve(sub, *bnds, np.ascontiguousarray(xr[idx]) if xr.ndim == 3 else xr, nthreads=8)
                    for key in st:
                        st[key][idx] = sub[key]
        u0 = st["u"][:, 0].copy()
        out["u0"].append(u0); out["iter"].append(st["iter"].copy()); out["status"].append(st["status"].copy())
        x = step(x, u0)
        if w is not None:
            x = (x + w[k]).astype(np.float32)
        out["xs"].append(x.copy())
    st["x"][:, 0] = x
    return dict(u0=np.array(out["u0"]), iter=np.array(out["iter"]), status=np.array(out["status"]), xs=np.array(out["xs"]), x=x, st=st)


def case_oracle(O, c, inp, nominal=False):
    """the oracle's loop of a case (nominal: without its plant and disturbance)"""
    kw = {} if nominal else dict(plant=inp["plant"], w=inp["w"])
    return sim_oracle_loop(O, inp["probs"], inp["model"], inp["settings"], inp["x0"], inp["ref"], inp["bnds"], STEPS, c["adv"], **kw)


# ---- driving a handle ---------------------------------------------------------------------------------------------------------------------------

def _handle(T, c, inp, plant=True):
    s = T.TinyBatchSolver(inp["probs"][0], c["B"], settings=inp["settings"])
    if inp["mods"] is not None:
        s.set_models(inp["mods"])
    s.select_kernel(2 if c["arith"] == "exact" else 3)
    s.set_row_kernel(c["row"])
    if c.get("storage"):
        s.set_storage(*c["storage"])
    s.set_bounds(*inp["bnds"])
    if isinstance(inp["ref"], tuple):
        s.set_xref_window(*inp["ref"])
    else:
        s.set_xref(inp["ref"])
    s.set_x0(inp["x0"])
    assert s.kernel_name() == c["name"], s.kernel_name()
    assert s.plant_mode() == 0
    if plant and inp["plant"] is not None:
        s.set_plant(*inp["plant"])
        assert s.plant_mode() == (1 if c["plant"] == "shared" else 2)
    assert s.kernel_name() == c["name"], s.kernel_name()
    return s


def _check_final(s, want, what):
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want["st"][k]), f"{what}: {k} differs after the last step"
    assert same_bits(s.get_x0(), want["x"]), f"{what}: get_x0() differs after the last step"


def _run(s, chunks, adv, w, want, what):
    us, xs, k = [], [], 0
    for n in chunks:
        u, x = s.mpc_run_sim(n, adv, None if w is None else w[k:k + n])
        us.append(u); xs.append(x); k += n
    us, xs = np.concatenate(us), np.concatenate(xs)
    assert same_bits(us, want["u0"]), f"{what}: u.col(0) differs from step {G._first_diff(us, want['u0'])} on"
    assert same_bits(xs, want["xs"]), f"{what}: x_traj differs from step {G._first_diff(xs, want['xs'])} on"
    _check_final(s, want, what)


def _step(s, steps, adv, w, want, what):
    for k in range(steps):
        s.mpc_step_sim(adv, None if w is None else w[k])
        it, stt, _ = s.get_status()
        assert np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"{what}: iter / status differ after step {k}"
        assert same_bits(s.get_u()[:, 0], want["u0"][k]), f"{what}: u.col(0) differs at step {k}"
        assert same_bits(s.get_x0(), want["xs"][k]), f"{what}: x0 differs after step {k}"
    _check_final(s, want, what)


def _three_ways(T, c, inp, want, steps=STEPS, k1=K1):
    """A one-step run is the captured graph on every kernel, as it is for the nominal call: the on-chip cases count 0 captures on the first two ways
    and exactly that one on the third; the replayed cases at least one on the first."""
    for way, chunks in (("run", (k1, steps - k1)), ("step by step", None), ("run with a single step", (k1, 1, steps - k1 - 1))):
        s = _handle(T, c, inp)
        assert s.closed_loop_kernel_name() == c.get("loop", c["name"]), s.closed_loop_kernel_name()
        what = f"{c['id']} {way}"
        if chunks:
            _run(s, chunks, c["adv"], inp["w"], want, what)
        else:
            _step(s, steps, c["adv"], inp["w"], want, what)
        caps = s.lib.tiny_batch_debug_graph_captures(s._h)
        if c["onchip"]:
            assert caps == (1 if chunks and 1 in chunks else 0), (what, caps)
        elif way == "run":
            assert caps >= 1, (what, caps)
        s.close()


def _host_reference(T, O, c, inp):
    """fma arithmetic / fp16 storage: the loop driven from the host on a second handle, the plant step and the disturbance applied on the host"""
    step = plant_fn(O, inp["probs"], inp["model"], inp["plant"])
    xs = []

    def plant(x, u0):
        x = step(x, u0)
        if inp["w"] is not None:
            x = (x + inp["w"][len(xs)]).astype(np.float32)
        xs.append(x.copy())
        return x
    h = _handle(T, c, inp, plant=False)
    want = host_closed_loop(h, plant, inp["x0"], inp["ref"], STEPS, c["adv"])
    h.close()
    want["xs"] = np.array(xs)
    return want


# ---- 1 - 4: the paths -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ONCHIP_CASES, ids=_ids(ONCHIP_CASES))
def test_on_chip_exact(tinympc, oracle_mod, case):
    """The SIM instantiations of the 16-lane kernel, shared and per-instance models, against the oracle's loop; no graph is captured by a run of several steps."""
    inp = case_inputs(tinympc.problems, oracle_mod, case)
    want = case_oracle(oracle_mod, case, inp)
    closed_loop_conditions(want, inp["bnds"], inp["settings"], case["id"])
    _three_ways(tinympc, case, inp, want)


def test_on_chip_fma(tinympc, oracle_mod):
    inp = case_inputs(tinympc.problems, oracle_mod, FMA_CASE)
    closed_loop_conditions(case_oracle(oracle_mod, FMA_CASE, inp), inp["bnds"], inp["settings"], FMA_CASE["id"])
    _three_ways(tinympc, FMA_CASE, inp, _host_reference(tinympc, oracle_mod, FMA_CASE, inp))


@pytest.mark.parametrize("case", REPLAY_CASES, ids=_ids(REPLAY_CASES))
def test_replayed_path(tinympc, oracle_mod, case):
    """solve + plant kernel per step from a captured graph: the rolled-loop, wave and quad kernels, fp16 storage; the plant kernel past one block."""
    inp = case_inputs(tinympc.problems, oracle_mod, case)
    want = case_oracle(oracle_mod, case, inp)
    closed_loop_conditions(want, inp["bnds"], inp["settings"], case["id"])
    if case.get("storage"):
        want = _host_reference(tinympc, oracle_mod, case, inp)
    _three_ways(tinympc, case, inp, want)


def test_tile16_hands_a_simulated_run_over(tinympc, oracle_mod):
    T, O, c = tinympc, oracle_mod, HANDOVER_CASE
    inp = case_inputs(T.problems, O, c)
    s = _handle(T, c, inp, plant=False)
    assert s.kernel_name() == s.closed_loop_kernel_name() == "tile16<12,4,30,exact>"
    s.set_plant(*inp["plant"])
    assert s.closed_loop_kernel_name() == "rowlane<12,4,30,exact>" and s.kernel_name() == "tile16<12,4,30,exact>"
    s.close()
    want = case_oracle(O, c, inp)
    closed_loop_conditions(want, inp["bnds"], inp["settings"], c["id"])
    _three_ways(T, c, inp, want)   # (the steps and the one-step run solve on tile16; the runs are one launch of the 16-lane kernel: no graph)
    # a disturbance without a plant is handed over too (only the call knows: the name stays the nominal run's) — no graph, the oracle's loop
    s = _handle(T, c, inp, plant=False)
    only_w = sim_oracle_loop(O, inp["probs"], inp["model"], inp["settings"], inp["x0"], inp["ref"], inp["bnds"], STEPS, c["adv"], w=inp["w"])
    assert s.closed_loop_kernel_name() == "tile16<12,4,30,exact>"
    _run(s, (K1, STEPS - K1), c["adv"], inp["w"], only_w, c["id"] + " w without a plant")
    assert s.lib.tiny_batch_debug_graph_captures(s._h) == 0
    s.close()
    s = _handle(T, c, inp)
    s.clear_plant()
    assert s.plant_mode() == 0 and s.closed_loop_kernel_name() == "tile16<12,4,30,exact>"
    nominal = oracle_closed_loop(O, inp["probs"][0], np.float32, inp["settings"], inp["x0"], inp["ref"], inp["bnds"], STEPS, c["adv"])
    G._run(s, (K1, STEPS - K1), c["adv"], nominal, c["id"] + " after clear_plant")
    s.close()


# ---- 5: identities ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [ONCHIP_CASES[0], REPLAY_CASES[0]], ids=["on chip", "replayed"])
def test_the_model_as_plant_is_the_nominal_run(tinympc, oracle_mod, case):
    """set_plant(Adyn, Bdyn) without a disturbance equals the run without a plant; the existing calls honour a set plant"""
    T = tinympc
    inp = dict(case_inputs(T.problems, oracle_mod, case), w=None)
    p = inp["probs"][0]
    model = (np.asarray(p["Adyn"], np.float32), np.asarray(p["Bdyn"], np.float32))
    got = {}
    for key, plant in (("none", None), ("model", model), ("other", inp["plant"])):
        s = _handle(T, case, dict(inp, plant=plant))
        u, x = s.mpc_run_sim(STEPS, case["adv"])
        got[key] = (u, x, s.get_state(), s.get_x0())
        s.close()
        if plant is not None:   # the existing calls on a handle with that plant
            s = _handle(T, case, dict(inp, plant=plant))
            assert same_bits(s.mpc_run_traj(STEPS, case["adv"]), u), key
            assert same_bits(s.get_x0(), got[key][3]), key
            s.close()
            s = _handle(T, case, dict(inp, plant=plant))
            for k in range(STEPS):
                s.mpc_step_async(case["adv"])
                assert same_bits(s.get_x0(), x[k]), (key, k)
            s.close()
    for a, b in zip(got["none"][:2] + (got["none"][3],), got["model"][:2] + (got["model"][3],)):
        assert same_bits(a, b)
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got["none"][2][k], got["model"][2][k]), k
    assert not np.array_equal(got["none"][0][1], got["other"][0][1]), "another plant leaves the trajectory where it was"


@pytest.mark.parametrize("name", ["track", "hover"])
def test_the_model_as_plant_equals_the_compiled_reference(tinympc, oracle_mod, name):
    """the first 5 instances and 10 steps of the reference's own closed-loop traces (tests/golden/closed_loop_traces.npz), with the model set as a shared plant"""
    T = tinympc
    z = np.load(GOLDEN / "closed_loop_traces.npz")
    prob, x0, fn, steps, settings, table, start = closed_loop_case(T.problems, oracle_mod, z, name)
    B, steps = 5, 10
    s = T.TinyBatchSolver(prob, B, settings=settings)
    s.select_kernel(2); s.set_row_kernel(1)
    s.set_bounds(*T.problems.bounds_arrays(prob))
    if table is not None:
        s.set_xref_window(table, start[:B])
    else:
        s.set_xref(fn(0))
    s.set_x0(x0[:B])
    s.set_plant(np.asarray(prob["Adyn"], np.float32), np.asarray(prob["Bdyn"], np.float32))
    assert s.closed_loop_kernel_name() == "rowlane<12,4,30,exact>"
    u, x = s.mpc_run_sim(steps, 1 if table is not None else 0)
    s.close()
    assert same_bits(u, z[f"{name}_u0"][:steps, :B]), name   # (the traces hold u.col(0) alone; instances are independent)
    assert np.isfinite(x).all()


def test_a_disturbance_of_zeros(tinympc, oracle_mod):
    """On the all-zero states of helpers.zero_state_inputs: w of -0 is w = None bit for bit; w of +0 turns exactly the -0 products into +0."""
    T, O = tinympc, oracle_mod
    c = dict(dims=(4, 1, 10), quadrotor=False)
    prob = positive_system(G.case_problem(T.problems, O, c))
    B, steps = 37, 4
    x0, ref, bnds = zero_state_inputs(prob, B, 11)
    out = {}
    for key, w in (("none", None), ("neg", np.full((steps, B, 4), -0.0, np.float32)), ("pos", np.zeros((steps, B, 4), np.float32))):
        s = T.TinyBatchSolver(prob, B, settings=dict(BASE))
        s.select_kernel(2); s.set_row_kernel(1)
        s.set_bounds(*bnds); s.set_xref(ref); s.set_x0(x0)
        assert s.closed_loop_kernel_name() == "rowlane<4,1,10,exact>"
        out[key] = s.mpc_run_sim(steps, 0, w)
        s.close()
    assert same_bits(out["none"][0], out["neg"][0]) and same_bits(out["none"][1], out["neg"][1])
    lost = rows_of_negative_zeros(prob, x0, out["none"][0][0])
    assert lost[0].all() and not lost[1].any(), "the inputs do not reach the rows of negative zeros"
    x1n, x1p = out["none"][1][0], out["pos"][1][0]
    assert np.all(x1n == 0) and np.all(x1p == 0)
    assert np.array_equal(np.signbit(x1n), lost), "nx < 8: the lazy product keeps the -0 of a row whose products are all -0"
    assert not np.signbit(x1p).any(), "(-0) + (+0) = +0"
    assert same_bits(out["none"][0][0], out["pos"][0][0]), "u.col(0) of the first solve does not depend on w"


# ---- 6, 7: guard zones, refusals --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 17])
def test_guard_zones_stay_intact(tinympc, oracle_mod, B):
    T = tinympc
    T.solver.debug_guards(True)
    try:
        for case in (ONCHIP_CASES[1], REPLAY_CASES[0]):
            c = dict(case, B=B, id=f"{case['id']} guards B={B}", plant="inst", w=True)
            inp = case_inputs(T.problems, oracle_mod, c)
            s = _handle(T, c, inp)
            u, x = s.mpc_run_sim(STEPS, c["adv"], inp["w"])
            st = s.get_state()
            assert T.solver.debug_check() == 0, c["id"]
            assert np.isfinite(u).all() and np.isfinite(x).all() and all(np.isfinite(st[k]).all() for k in STATE_ORDER), c["id"]
            assert s.lib.tiny_batch_debug_graph_captures(s._h) == (0 if c["onchip"] else 1)
            s.close()
    finally:
        T.solver.debug_guards(False)


def test_refusals(tinympc, oracle_mod):
    T = tinympc
    inp = case_inputs(T.problems, oracle_mod, ONCHIP_CASES[0])
    s = _handle(T, ONCHIP_CASES[0], inp, plant=False)
    EINVAL = -1
    a = np.zeros(144, np.float32)
    fp = a.ctypes.data_as(C.POINTER(C.c_float))
    assert s.lib.tiny_batch_set_plant(s._h, None, fp, 1) == EINVAL and "NULL" in s.lib.tiny_batch_last_error().decode()
    assert s.lib.tiny_batch_set_plant(s._h, fp, None, 1) == EINVAL
    assert s.lib.tiny_batch_set_plant(None, fp, fp, 1) == EINVAL
    assert s.plant_mode() == 0
    for steps in (0, -3):
        assert s.lib.tiny_batch_mpc_run_sim(s._h, steps, 0, None, None, None) == EINVAL
        assert s.lib.tiny_batch_mpc_run_sim_async(s._h, steps, 0, None, None, None) == EINVAL
    err = lambda: s.lib.tiny_batch_last_error().decode()
    assert s.lib.tiny_batch_mpc_run_sim_async(s._h, 0, 0, None, None, None) == EINVAL and err().startswith("tiny_batch_mpc_run_sim_async:"), err()
    assert s.lib.tiny_batch_mpc_run_sim_async(s._h, 2, -1, None, None, None) == EINVAL and err().startswith("tiny_batch_mpc_run_sim_async:"), err()
    assert s.lib.tiny_batch_mpc_run_sim(s._h, 2, -1, None, None, None) == EINVAL and err().startswith("tiny_batch_mpc_run_sim:"), err()
    assert s.lib.tiny_batch_mpc_step_sim_async(s._h, -1, None) == EINVAL and err().startswith("tiny_batch_mpc_step_sim_async:"), err()
    assert s.lib.tiny_batch_mpc_run_async(s._h, 0, 0) == EINVAL and err().startswith("tiny_batch_mpc_run_async:"), err()
    assert s.lib.tiny_batch_mpc_step_async(s._h, -1) == EINVAL and err().startswith("tiny_batch_mpc_step_async:"), err()
    s.set_plant(*inp["plant"]); assert s.plant_mode() == 1
    Ap = np.broadcast_to(inp["plant"][0], (5, 12, 12)); Bp = np.broadcast_to(inp["plant"][1], (5, 12, 4))
    s.set_plant(Ap, Bp); assert s.plant_mode() == 2
    s.clear_plant(); assert s.plant_mode() == 0
    s.clear_plant(); assert s.plant_mode() == 0
    s.close()


def test_equal_blocking_calls_replay_one_graph(tinympc, oracle_mod):
    """tiny_batch_mpc_run_sim keeps its device copies of w, u0_traj and x_traj on the handle: on a replayed kernel a loop of equal calls captures once;
    set_plant — the first one included — and another step count capture again"""
    T, c = tinympc, REPLAY_CASES[0]
    inp = case_inputs(T.problems, oracle_mod, c)
    caps = lambda: s.lib.tiny_batch_debug_graph_captures(s._h)
    s = _handle(T, c, inp, plant=False)
    s.mpc_run_traj(4, c["adv"])
    assert caps() == 1
    s.set_plant(*inp["plant"])
    for _ in range(3):
        s.mpc_run_sim(4, c["adv"], inp["w"][:4])
    assert caps() == 2
    s.mpc_run_sim(3, c["adv"], inp["w"][:3])
    assert caps() == 3
    s.close()


def test_the_montecarlo_example_runs(tinympc, tmp_path):
    """examples/quadrotor_tracking_montecarlo.cpp built with g++ and run: 512 plants in one on-chip run through the C-ABI alone"""
    import re
    import shutil
    import subprocess
    from pathlib import Path
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this box")
    root = Path(__file__).resolve().parents[1]
    lib_dir = root / "accelerated-tinympc_amd" / "lib"
    exe = tmp_path / "montecarlo"
    subprocess.run(["g++", "-std=c++17", "-O1", f"-I{root / 'include'}", str(root / "examples" / "quadrotor_tracking_montecarlo.cpp"), f"-L{lib_dir}",
                    "-ltinympc_hip", f"-Wl,-rpath,{lib_dir}", "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), str(root / "accelerated-tinympc_amd" / "data" / "quadrotor_20hz.bin"), "512", "40"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "solve kernel: rowlane<12,4,30,exact>, closed-loop kernel: rowlane<12,4,30,exact>, 512 plants (plant mode 2), 40 steps" in r.stdout, r.stdout[:300]
    errs = [(float(a), float(b)) for a, b in re.findall(r"mean tracking error ([0-9.eE+-]+), worst ([0-9.eE+-]+)", r.stdout)]
    assert len(errs) == 3 and "(final)" in r.stdout and np.isfinite(errs).all() and all(0 < m <= w for m, w in errs), r.stdout
