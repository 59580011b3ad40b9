"""The fp64 library's closed loop against a separate plant, with a disturbance and the state trajectory (tiny_batch64_set_plant,
tiny_batch64_mpc_run_sim, tiny_batch64_mpc_step_sim), bit for bit against the fp64 oracle's loop, signs of zeros included: u.col(0) and x.col(0) of
every step, iter and status per step, the twelve work arrays, the four residual fields, x.col(0) and the window starts after the last step.

The reference loop is tests/test_sim_loop_gpu.py's sim_oracle_loop restated for np.float64: y = g = 0, the oracle solves, plant_step of an Oracle
built on the plant's matrices (one oracle, or one per instance), then x = x + w[k] in float64.  Twelve rows: the five unrolled SIM instantiations,
the capacity-32 run-time-horizon body up to its edge, and the launch sequence with the simulated plant kernel (the capacity-64 body, a class without a
sixteen-lane kernel, the thread-per-instance kernel by choice).  closed_loop_kernel_name() is asserted on every handle.  Every row runs 8 steps and
is driven three ways: mpc_run_sim in chunks (3, 5); 8 x mpc_step_sim (tiny_batch64_mpc_step_sim advances no window: where the row slides one the host
slides it between two steps, as helpers.host_closed_loop does); chunks (3, 1, 4) — the off-by-one place of the host's last plant step, w[steps - 1]
and x_traj[steps - 1].  tests/test_sim_loop64_host.py checks on the CPU that every row's inputs meet the conditions and leave the nominal loop."""
import ctypes as C

import numpy as np
import pytest

from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_conditions, closed_loop_inputs, oracle_closed_loop, ref_at, same_bits
from test_closed_loop_gpu import BASE, _first_diff

pytestmark = pytest.mark.gpu

STEPS, K1 = 8, 3
EINVAL = -1  # TINY_BATCH_EINVAL


def _row(name, dims, B, ref, adv, plant, w, settings=None, kernel=0, **kw):
    """name: what closed_loop_kernel_name() reports with the row's plant set; plant: None (the model's), "shared" or "inst"; w: with a disturbance;
    kernel: tiny_batch64_select_kernel's argument"""
    return dict(name=name, dims=dims, B=B, ref=ref, adv=adv, plant=plant, w=w, settings=settings or {}, kernel=kernel, **kw)


ROWS = [
    _row("rows64<12,4,10,sim>", (12, 4, 10), 130, "window", 1, "inst", True),        # more than one wave, the last one partial; past the plant kernel's block of 128
    _row("rows64<12,4,10,sim>", (12, 4, 10), 5, "window", 1, "shared", True),
    _row("rows64<12,4,10,mpc>", (12, 4, 10), 5, "window", 1, None, True),            # the disturbance alone: the model's own rows go through the SIM kernel
    _row("rows64<12,4,30,sim>", (12, 4, 30), 5, "window", 2, "inst", True, near_end=True),   # slack in LDS, one wave per SIMD, the most scratch
    _row("rows64<12,4,20,sim>", (12, 4, 20), 5, "inst", 0, "inst", False, dict(max_iter=1)),  # no add is executed
    _row("rows64<4,1,10,sim>", (4, 1, 10), 130, "shared", 0, "shared", True, dict(check_termination=3)),   # nx < 8: the lazy order; nu = 1
    _row("rows64<8,4,9,sim>", (8, 4, 9), 3, "window", 1, "inst", True),
    _row("rows64<12,2,n<=32,sim>", (12, 2, 13), 37, "window", 1, "shared", True),    # the run-time-horizon body
    _row("rows64<4,4,n<=32,sim>", (4, 4, 32), 5, "inst", 0, "inst", False),          # capacity edge
    _row("rows64<12,4,n<=64>", (12, 4, 40), 5, "window", 1, "inst", True),           # launch sequence
    _row("thread64<16,4>", (16, 4, 10), 130, "window", 1, "shared", True),           # launch sequence, no rows kernel
    _row("thread64<12,4>", (12, 4, 10), 1, "shared", 0, "inst", True, kernel=1),     # launch sequence by choice
]
for _i, _r in enumerate(ROWS):
    _r["id"] = "{}-{}_{}_{}-B{}-{}{}-plant_{}{}".format(_i + 1, *_r["dims"], _r["B"], _r["ref"], _r["adv"], _r["plant"], "-w" if _r["w"] else "")
ONCHIP = [r for r in ROWS if r["name"].endswith((",sim>", ",mpc>"))]

# x0 amplitudes / bound scales (helpers.closed_loop_inputs) where the stock ones do not meet the conditions, found on the CPU with the oracle's loop alone
TUNED = {
    "12-12_4_10-B1-shared0-plant_inst-w": dict(amp=(0.02, 0.07)),
}
assert set(TUNED) <= {r["id"] for r in ROWS}


# ---- inputs and the reference loop: shared with tests/test_sim_loop64_host.py -------------------------------------------------------------------

_inputs = {}


def row_inputs(pr, O, r):
    """everything a row runs on, built once: prob, settings, x0, ref, bnds, the plant (A_p, B_p) in the row's mode, w.  The recipe is
    tests/test_sim_loop_gpu.py's in float64: helpers.closed_loop_inputs with seed 4242 + nx; from default_rng(seed + 1) A_p = A (1 + 0.05 n),
    B_p = B (1 + 0.05 n) entry-wise per instance (a shared plant is instance 0's), w = 0.01 n."""
    if r["id"] in _inputs:
        return _inputs[r["id"]]
    nx, nu, N = r["dims"]
    B = r["B"]
    prob = pr.random_system(nx, nu, N, seed=100 * nx + nu, riccati=O.riccati)
    seed = 4242 + nx
    x0, ref, bnds = closed_loop_inputs(prob, B, r["ref"], seed, near_end=bool(r.get("near_end")), dtype=np.float64, **TUNED.get(r["id"], {}))
    rng = np.random.default_rng(seed + 1)
    A = np.broadcast_to(np.asarray(prob["Adyn"], np.float64), (B, nx, nx))
    Bm = np.broadcast_to(np.asarray(prob["Bdyn"], np.float64), (B, nx, nu))
    Ap = A * (1 + 0.05 * rng.standard_normal(A.shape))
    Bp = Bm * (1 + 0.05 * rng.standard_normal(Bm.shape))
    w = 0.01 * rng.standard_normal((STEPS, B, nx))
    plant = None if r["plant"] is None else (Ap[0], Bp[0]) if r["plant"] == "shared" else (Ap, Bp)
    out = dict(prob=prob, settings=dict(BASE, **r["settings"]), x0=x0, ref=ref, bnds=bnds, plant=plant, w=w if r["w"] else None)
    _inputs[r["id"]] = out
    return out


def plant_fn(O, prob, plant):
    """x, u0 -> the plant step of every instance in the oracle's (= the reference's) order: Oracle(dict(prob, Adyn = A_p, Bdyn = B_p), float64).plant_step,
    one oracle for a shared plant, one per instance otherwise; plant = None: the model"""
    if plant is None:
        return O.Oracle(prob, np.float64).plant_step
    if plant[0].ndim == 2:
        return O.Oracle(dict(prob, Adyn=plant[0], Bdyn=plant[1]), np.float64).plant_step
    each = [O.Oracle(dict(prob, Adyn=a, Bdyn=b), np.float64) for a, b in zip(*plant)]
    return lambda x, u0: np.concatenate([o.plant_step(x[b:b + 1], u0[b:b + 1]) for b, o in enumerate(each)])


def sim_oracle_loop(O, prob, settings, x0, ref, bnds, steps, adv, plant=None, w=None):
    """helpers.oracle_closed_loop against a separate plant, in float64: per step y = g = 0, tiny_solve, x = plant(x, u0), then x = x + w[k].
    Records xs, the state after every plant step."""
    nx, nu, N, B = prob["nx"], prob["nu"], prob["N"], len(x0)
    orc = O.Oracle(prob, np.float64, settings)
    step = plant_fn(O, prob, plant)
    st = O.new_state(B, nx, nu, N, np.float64)
    x = np.array(x0, np.float64)
    out = dict(u0=[], iter=[], status=[], xs=[])
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        orc.solve(st, *bnds, ref_at(ref, k, adv, N, B), nthreads=8)
        u0 = st["u"][:, 0].copy()
        out["u0"].append(u0); out["iter"].append(st["iter"].copy()); out["status"].append(st["status"].copy())
        x = np.asarray(step(x, u0), np.float64)
        if w is not None:
            x = x + np.asarray(w[k], np.float64)
        out["xs"].append(x.copy())
    st["x"][:, 0] = x
    return dict(u0=np.array(out["u0"]), iter=np.array(out["iter"]), status=np.array(out["status"]), xs=np.array(out["xs"]), x=x, st=st)


def row_oracle(O, r, inp, nominal=False):
    """the oracle's loop of a row (nominal: without its plant and disturbance)"""
    kw = {} if nominal else dict(plant=inp["plant"], w=inp["w"])
    return sim_oracle_loop(O, inp["prob"], inp["settings"], inp["x0"], inp["ref"], inp["bnds"], STEPS, r["adv"], **kw)


_references = {}


def _reference(T, O, r):
    """computed once per row and shared by the tests that need it; nobody writes to it.  The conditions on the inputs are asserted before anything is
    compared with it."""
    if r["id"] not in _references:
        inp = row_inputs(T.problems, O, r)
        want = row_oracle(O, r, inp)
        closed_loop_conditions(want, inp["bnds"], inp["settings"], r["id"])
        _references[r["id"]] = (inp, want)
    return _references[r["id"]]


# ---- driving a handle ---------------------------------------------------------------------------------------------------------------------------

def _nominal_name(r):
    return r["name"].replace(",sim>", ",mpc>")


def _handle(T, r, inp, plant=True):
    s = T.TinyBatchSolver64(inp["prob"], r["B"], settings=inp["settings"])
    s.select_kernel(r["kernel"])
    s.set_bounds(*inp["bnds"])
    if isinstance(inp["ref"], tuple):
        s.set_xref_window(*inp["ref"])
    else:
        s.set_xref(inp["ref"])
    s.set_x0(inp["x0"])
    assert s.plant_mode() == 0 and s.closed_loop_kernel_name() == _nominal_name(r), s.closed_loop_kernel_name()
    if plant and inp["plant"] is not None:
        s.set_plant(*inp["plant"])
        assert s.plant_mode() == (1 if inp["plant"][0].ndim == 2 else 2)
        assert s.closed_loop_kernel_name() == r["name"], s.closed_loop_kernel_name()
    return s


def _check_final(s, r, ref, want, what, starts=True):
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want["st"][k]), f"{what}: {k} differs after the last step"
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


def _slide(s, ref, k, adv, N, B):
    """the reference of MPC step k set from the host: the window where it still lies inside the table, else the clamped per-instance array
    (set_xref_window refuses such a start); returns whether the handle still has a window"""
    start = ref[1] + k * adv
    if int(start.max()) + N <= len(ref[0]):
        s.set_xref_window(ref[0], start)
        return True
    s.set_xref(ref_at(ref, k, adv, N, B))
    return False


def _step(s, r, inp, want, what):
    w, ref, has_window = inp["w"], inp["ref"], isinstance(inp["ref"], tuple)
    for k in range(STEPS):
        rc = s.mpc_step_sim(None if w is None else w[k])
        assert rc == int((want["status"][k] != 1).any()), f"{what}: mpc_step_sim returns what the step's solve returns (step {k})"
        it, stt, _ = s.get_status()
        assert np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"{what}: iter / status differ after step {k}"
        x0, u0 = s.first_columns()
        assert same_bits(u0, want["u0"][k]), f"{what}: u.col(0) differs at step {k}"
        assert same_bits(x0, want["xs"][k]), f"{what}: x.col(0) differs after step {k}"
        if isinstance(ref, tuple) and r["adv"]:
            has_window = _slide(s, ref, k + 1, r["adv"], s.N, s.B)
    _check_final(s, r, ref, want, what, starts=has_window)


def _three_ways(T, r, inp, want):
    for way, chunks in (("run", (K1, STEPS - K1)), ("step by step", None), ("run with a single step", (K1, 1, STEPS - K1 - 1))):
        s = _handle(T, r, inp)
        what = f"{r['id']} {way}"
        if chunks:
            _run(s, r, inp, chunks, want, what)
        else:
            _step(s, r, inp, want, what)
        s.close()


# ---- the twelve rows --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_simulated_run_equals_the_oracle_loop(tinympc, oracle_mod, row):
    inp, want = _reference(tinympc, oracle_mod, row)
    _three_ways(tinympc, row, inp, want)


# the capacity-32 body's SIM instantiation for the classes no row above holds: 5 instances (one full group of four and a tail group), the smallest
# horizon that selects the body, max_iter = 10.  (4, 2) is also the one class whose simulated plant kernel no row reaches.
REMAINING = [_row(f"rows64<{nx},{nu},n<=32,sim>", (nx, nu, 3), 5, "window", 1, "inst", True, dict(max_iter=10), id=f"{nx}_{nu}_3-B5-window1-plant_inst-w")
             for nx, nu in [(12, 4), (4, 1), (8, 4), (4, 2)]]


@pytest.mark.parametrize("row", REMAINING, ids=[r["id"] for r in REMAINING])
def test_simulated_run_on_the_remaining_capacity_32_classes(tinympc, oracle_mod, row):
    """mpc_run_sim in chunks (3, 5) against the oracle's loop (the inputs are not held to helpers.closed_loop_conditions: the rows are here for the
    instantiation they reach)"""
    inp = row_inputs(tinympc.problems, oracle_mod, row)
    want = row_oracle(oracle_mod, row, inp)
    s = _handle(tinympc, row, inp)
    _run(s, row, inp, (K1, STEPS - K1), want, row["id"])
    s.close()


# ---- identities -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [ROWS[0], ROWS[3]], ids=[ROWS[0]["id"], ROWS[3]["id"]])
def test_the_model_as_plant_with_a_disturbance_of_negative_zeros_is_the_nominal_run(tinympc, oracle_mod, row):
    """plant = the model (shared and per instance), w = -0.0: the bits of mpc_run_traj on a second handle"""
    T, r = tinympc, row
    inp = row_inputs(T.problems, oracle_mod, r)
    prob, B = inp["prob"], r["B"]
    A, Bm = np.asarray(prob["Adyn"], np.float64), np.asarray(prob["Bdyn"], np.float64)
    s = _handle(T, r, inp, plant=False)
    u_nom = s.mpc_run_traj(STEPS, r["adv"])
    nom, x_nom, start_nom = s.get_state(), s.first_columns()[0], s.xref_start()
    s.close()
    w = np.full((STEPS, B, prob["nx"]), -0.0)
    for plant in ((A, Bm), (np.broadcast_to(A, (B,) + A.shape), np.broadcast_to(Bm, (B,) + Bm.shape))):
        s = _handle(T, r, dict(inp, plant=plant))
        u, x = s.mpc_run_sim(STEPS, r["adv"], w)
        assert same_bits(u, u_nom), f"{r['id']}: u.col(0) differs from step {_first_diff(u, u_nom)} on"
        assert same_bits(x[-1], x_nom) and same_bits(s.first_columns()[0], x_nom)
        got = s.get_state()
        for k in STATE_ORDER + SCALAR_ORDER:
            assert same_bits(got[k], nom[k]), k
        assert np.array_equal(s.xref_start(), start_nom)
        s.close()


@pytest.mark.parametrize("row", [ROWS[1], ROWS[5], ROWS[9]], ids=[ROWS[1]["id"], ROWS[5]["id"], ROWS[9]["id"]])
def test_the_nominal_calls_honour_a_plant(tinympc, oracle_mod, row):
    """with a plant set and no w, mpc_run_traj, mpc_run and (where nothing slides) mpc_step equal mpc_run_sim(w = None)"""
    T, r = tinympc, row
    inp = dict(row_inputs(T.problems, oracle_mod, r), w=None)
    s = _handle(T, r, inp)
    u, x = s.mpc_run_sim(STEPS, r["adv"])
    want = dict(st=s.get_state(), x=s.first_columns()[0])
    s.close()
    nominal = row_oracle(oracle_mod, r, inp, nominal=True)
    assert not np.array_equal(u[1], nominal["u0"][1]), "the plant leaves the trajectory where it was"
    assert same_bits(x[-1], want["x"])

    s = _handle(T, r, inp)
    assert same_bits(s.mpc_run_traj(STEPS, r["adv"]), u)
    _check_final(s, r, inp["ref"], want, r["id"] + " mpc_run_traj")
    s.close()
    s = _handle(T, r, inp)
    s.mpc_run(K1, r["adv"]); s.mpc_run(1, r["adv"]); s.mpc_run(STEPS - K1 - 1, r["adv"])
    _check_final(s, r, inp["ref"], want, r["id"] + " mpc_run")
    s.close()
    if r["adv"] == 0 and not isinstance(inp["ref"], tuple):
        s = _handle(T, r, inp)
        for k in range(STEPS):
            s.mpc_step()
            assert same_bits(s.first_columns()[0], x[k]), (r["id"], k)
        _check_final(s, r, inp["ref"], want, r["id"] + " mpc_step")
        s.close()


def test_clear_plant_restores_the_nominal_run(tinympc, oracle_mod):
    T, O, r = tinympc, oracle_mod, ROWS[1]
    inp = row_inputs(T.problems, O, r)
    s = _handle(T, r, inp, plant=False)
    assert s.plant_mode() == 0 and s.closed_loop_kernel_name() == "rows64<12,4,10,mpc>"
    s.set_plant(*inp["plant"])
    assert s.plant_mode() == 1 and s.closed_loop_kernel_name() == "rows64<12,4,10,sim>" and s.kernel_name() == "rows64<12,4,10>"
    Ap, Bp = (np.broadcast_to(m, (r["B"],) + m.shape) for m in inp["plant"])
    s.set_plant(Ap, Bp)
    assert s.plant_mode() == 2 and s.closed_loop_kernel_name() == "rows64<12,4,10,sim>"
    s.clear_plant()
    assert s.plant_mode() == 0 and s.closed_loop_kernel_name() == "rows64<12,4,10,mpc>"
    s.clear_plant()
    assert s.plant_mode() == 0
    nominal = oracle_closed_loop(O, inp["prob"], np.float64, inp["settings"], inp["x0"], inp["ref"], inp["bnds"], STEPS, r["adv"])
    traj = np.concatenate([s.mpc_run_traj(K1, r["adv"]), s.mpc_run_traj(STEPS - K1, r["adv"])])
    assert same_bits(traj, nominal["u0"]), f"u.col(0) differs from step {_first_diff(traj, nominal['u0'])} on"
    _check_final(s, r, inp["ref"], nominal, r["id"] + " after clear_plant")
    s.close()


def test_argument_checks(tinympc, oracle_mod):
    T, r = tinympc, ROWS[1]
    inp = row_inputs(T.problems, oracle_mod, r)
    s = _handle(T, r, inp, plant=False)
    lib, err = s.lib, lambda: s.lib.tiny_batch64_last_error().decode()
    a = np.zeros(144)
    dp = a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.tiny_batch64_set_plant(s._h, None, dp, 1) == EINVAL and "NULL" in err()
    assert lib.tiny_batch64_set_plant(s._h, dp, None, 1) == EINVAL
    assert lib.tiny_batch64_set_plant(None, dp, dp, 1) == EINVAL
    assert lib.tiny_batch64_plant_mode(None) == EINVAL and lib.tiny_batch64_clear_plant(None) == EINVAL and lib.tiny_batch64_mpc_step_sim(None, None) == EINVAL
    assert s.plant_mode() == 0
    s.set_plant(*inp["plant"])
    s.mpc_run_sim(2, 1, inp["w"][:2])
    before, start_before = s.get_state(), s.xref_start()
    for steps, adv in ((0, 0), (-3, 1), (1, -1), (4, -1)):
        assert lib.tiny_batch64_mpc_run_sim(s._h, steps, adv, None, None, None) == EINVAL, (steps, adv)
        xt = np.zeros((max(steps, 1), s.B, s.nx))
        assert lib.tiny_batch64_mpc_run_sim(s._h, steps, adv, s._dp(xt), None, s._dp(xt)) == EINVAL, (steps, adv)
    after = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(before[k], after[k]), f"{k} changed by a refused call"
    assert np.array_equal(start_before, s.xref_start()) and s.plant_mode() == 1
    s.close()
