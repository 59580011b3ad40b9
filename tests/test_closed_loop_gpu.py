"""Every device closed-loop path of the batch-shared library (tiny_batch_mpc_step_async, tiny_batch_mpc_run_traj, tiny_batch64_mpc_step) against a
closed loop computed elsewhere, bit for bit: u.col(0), iter and status of every step, the twelve work arrays, the residuals and x0 after the last.

Two references.  (1) Exact arithmetic with fp32 storage, and the fp64 library: the CPU oracle's closed loop (helpers.oracle_closed_loop: y = g = 0,
tiny_solve, the oracle's plant step, warm start), whose solve and plant step are pinned to the compiled reference in tests/test_oracle.py.
(2) fma arithmetic and fp16 storage have no bitwise oracle for the solve: the reference is the loop driven from the host on a second handle of the
same configuration (helpers.host_closed_loop), with the plant step of the fp32 oracle on the host — which pins the device plant step to the
reference's order under fma and fp16 as well.

Every configuration is driven three ways from identical inputs: mpc_run_traj(K1) + mpc_run_traj(STEPS - K1) (the on-chip loop or the captured graph,
and the continuation across calls), STEPS x mpc_step_async, and a run with one mpc_run_traj(1) in the middle (the other branch of
tiny_batch_mpc_run_traj_async).  kernel_name() / closed_loop_kernel_name() are asserted on every handle, so no case can run on another kernel.
The inputs of every case must make some instance run out of iterations, some converge early and some input sit on its bound
(helpers.closed_loop_conditions, checked on the oracle's loop).  A plant step that loses the +0 its GEMV accumulator starts from shows only in the
sign of a zero, which those inputs never produce: test_plant_step_starts_its_accumulator_at_positive_zero drives states of signed zeros for it.
tests/test_closed_loop_host.py checks that the tables below name every compiled class."""
import numpy as np
import pytest

from helpers import (SCALAR_ORDER, STATE_ORDER, closed_loop_conditions, closed_loop_inputs, host_closed_loop, oracle_closed_loop, positive_system, ref_at,
                     rows_of_negative_zeros, same_bits, zero_state_inputs)

pytestmark = pytest.mark.gpu

STEPS, K1 = 8, 3
BASE = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=30, check_termination=1, en_state_bound=1, en_input_bound=1)
# the settings of a family's cases by position: most check every iteration; one case stops after one iteration, a few check every 2nd / 3rd
VARIED = {1: dict(max_iter=1), 2: dict(check_termination=2), 4: dict(check_termination=3, max_iter=24)}
ARITH = ("exact", "fast")

ROWLANE = [(12, 4, 30), (12, 4, 25), (12, 4, 20), (12, 4, 10), (4, 1, 10), (8, 3, 7), (12, 4, 40), (12, 4, 50)]  # TINY_FOR_EACH_ROWLANE
QUADLANE = [10]                                                                                                    # TINY_FOR_EACH_QUADLANE
TILE16 = [30, 25, 20, 10]                                                                                          # TINY_FOR_EACH_TILE16
ROWLOOP = [(8, 4, 9), (12, 2, 11), (4, 2, 8), (4, 4, 6), (2, 2, 3), (12, 4, 17), (4, 1, 23), (8, 3, 12), (12, 4, 45)]  # every TINY_FOR_EACH_ROWDIMS pair
ROWLOOP_FMA = [(12, 4, 17), (8, 4, 9), (2, 2, 3)]
WAVE = [(32, 16, 12), (16, 8, 10), (16, 4, 10), (20, 8, 10), (24, 4, 10)]                                          # TINY_FOR_EACH_WAVEDIMS
GENERIC = [(20, 12, 12), (3, 2, 6), (8, 8, 6), (4, 3, 9), (36, 4, 5), (28, 16, 6), (12, 4, 35)]                    # GENERIC_DIMS of test_parity_gpu.py + one
F64 = [(12, 4, 10), (4, 1, 33), (8, 4, 9), (12, 2, 10), (4, 2, 33), (4, 4, 9), (16, 4, 10)]                        # TINY_FOR_EACH_F64DIMS
F64_ROWS_UNROLLED = {(12, 4, 10), (12, 4, 30), (12, 4, 20), (4, 1, 10), (8, 4, 9)}                                 # TINY_FOR_EACH_F64ROWS
F64_NO_ROWS = {(16, 4)}                                                                                            # not in TINY_FOR_EACH_F64ROWS_RT


def _case(fam, dims, arith, B, ref, adv=0, row=0, name="", variant=None, **kw):
    """one configuration: `row` = set_row_kernel's family, `variant` = select_kernel's (default: 2 exact / 3 fma), `name` = the kernel it must run on"""
    return dict(fam=fam, dims=dims, arith=arith, B=B, ref=ref, adv=adv, row=row, name=name, variant=variant if variant is not None else (2 if arith == "exact" else 3), **kw)


def _settle(cases):
    """the position in the family decides seed and settings"""
    for i, c in enumerate(cases):
        c.setdefault("settings", VARIED.get(i, {}))
        c["seed"] = 1000 * (1 + sum(map(ord, c["fam"]))) + i
        c["id"] = "{}-{}_{}_{}-{}-B{}-{}{}".format(c["name"].split("<")[0], *c["dims"], c["arith"], c["B"], c["ref"], c["adv"] if c["ref"] == "window" else "") + \
                  ("-end" if c.get("near_end") else "") + ("-" + "_".join(f"{k}{v}" for k, v in c["settings"].items()) if c["settings"] else "") + \
                  ("-h{}_{}".format(*c["storage"]) if c.get("storage") else "")
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


def _rowlane_cases():
    out = []
    sizes = (1, 3, 37, 130)  # ragged against the four instances of a wave and the 128 threads of a plant block
    for a, arith in enumerate(ARITH):
        todo = [(d, 1) for d in ROWLANE] + [((4, 1, N), 0) for N in QUADLANE]  # (4, 1, 10): forced onto the 16-lane kernel, and the automatic quad kernel
        for i, (d, row) in enumerate(todo):
            nx, nu, N = d
            B = sizes[(i + a) % 4]
            kern = "rowlane" if row else "quadlane"
            if nx == 12:
                ref, adv = "window", (i + a) % 3
            else:
                ref, adv = ("shared", "inst")[(i + a) % 2], 0
            # (12, 4, 25): the windows start within 6 rows of the table's end and clamp while the run slides them
            near_end = d == (12, 4, 25)
            out.append(_case("rowlane", d, arith, B, ref, 2 if near_end else adv, row, f"{kern}<{nx},{nu},{N},{arith}>", near_end=near_end))
    return _settle(out)


def _tile16_cases():
    out = []
    sizes = (17, 65, 130)  # past the tile of sixteen, past the workgroup of four tiles
    for a, arith in enumerate(ARITH):
        for i, N in enumerate(TILE16):
            ref = ("window", "shared")[(i + a) % 2]
            out.append(_case("tile16", (12, 4, N), arith, sizes[(i + a) % 3], ref, 1 + i % 2 if ref == "window" else 0, 5, f"tile16<12,4,{N},{arith}>"))
    out.append(_case("tile16", (12, 4, 30), "exact", 65, "window", 2, 5, "tile16<12,4,30,exact>", near_end=True, settings={}))
    out.append(_case("tile16", (12, 4, 10), "fast", 17, "window", 1, 5, "tile16<12,4,10,fast>", near_end=True, settings={}))
    return _settle(out)


def _rowloop_cases():
    out = []
    for arith, dims in (("exact", ROWLOOP), ("fast", ROWLOOP_FMA)):
        for i, d in enumerate(dims):
            ref = ("window", "shared", "inst")[i % 3]
            out.append(_case("rowloop", d, arith, (3, 37)[(i + (arith == "fast")) % 2], ref, 1 if ref == "window" else 0, 2, "rowloop<{},{},{}>".format(*d[:2], arith)))
    return _settle(out)


def _rowstream_cases():
    return _settle([_case("rowstream", (12, 4, 65), "exact", 37, "window", 1, 0, "rowstream<12,4,exact>", settings={}),   # N > 64: the automatic choice
                    _case("rowstream", (8, 4, 9), "exact", 3, "inst", 0, 3, "rowstream<8,4,exact>", settings=dict(check_termination=2))])


def _wave_cases():
    out = []
    todo = [(d, "exact", k) for k in ("wavestream", "waveres", "tile48") for d in WAVE if k != "tile48" or d[:2] == (32, 16)]
    todo += [((16, 8, 10), "fast", "waveres"), ((32, 16, 12), "fast", "tile48")]
    for i, (d, arith, k) in enumerate(todo):
        nx, nu, N = d
        ref = ("shared", "window", "inst")[i % 3]
        name = f"tile48<{nx},{nu},{N},{arith}>" if k == "tile48" else f"{k}<{nx},{nu},{arith}>"
        out.append(_case("wave", d, arith, (3, 18)[i % 2], ref, 1 if ref == "window" else 0, dict(wavestream=6, waveres=7, tile48=8)[k], name))
    return _settle(out)


def _generic_cases():
    # one thread per instance with the state in HBM: the larger classes take seconds per hundred iterations, so they get fewer of them and two ways
    out = []
    slow = {(20, 12, 12): dict(max_iter=10), (36, 4, 5): dict(check_termination=3, max_iter=9), (28, 16, 6): dict(max_iter=8), (12, 4, 35): dict(max_iter=8)}
    for i, d in enumerate(GENERIC):
        ref = ("inst", "window", "shared")[i % 3]
        out.append(_case("generic", d, "exact", 37, ref, 1 if ref == "window" else 0, 0, "generic<{},{},exact>".format(*d[:2]), variant=4, ways=2))
        if d in slow:
            out[-1]["settings"] = slow[d]
    return _settle(out)


def _stream_cases():
    # the MFMA streaming kernel (variant 1, fma): the quadrotor, and a class it pads to its chunks of four whose plant-step order is pinned
    return _settle([_case("stream", (12, 4, 10), "fast", 37, "window", 1, 0, "stream<3,1>", variant=1, quadrotor=True, settings={}),
                    _case("stream", (8, 3, 7), "fast", 18, "inst", 0, 0, "stream<2,1>", variant=1, settings=dict(check_termination=2))])


def _fp16_cases():
    out = []
    for arith in ARITH:
        for storage in ((16, None), (16, 16)):
            sfx = ",h16d" if storage[1] is None else ",h16"
            out.append(_case("fp16", (12, 4, 30), arith, 37, "window", 1, 1, f"rowlane<12,4,30,{arith}{sfx}>", storage=storage))
            out.append(_case("fp16", (12, 4, 17), arith, 18, "shared", 0, 2, f"rowloop<12,4,{arith},h16>", storage=storage))
            out.append(_case("fp16", (4, 1, 10), arith, 3, "inst", 0, 1, f"rowlane<4,1,10,{arith}{sfx}>", storage=storage))
    for i, c in enumerate(out):
        c["settings"] = dict(max_iter=1) if i == 4 else dict(check_termination=2) if i == 7 else {}
    return _settle(out)


def _f64_cases():
    out = []
    for i, d in enumerate(F64):
        for k in (1, 2):
            if k == 2 and d[:2] in F64_NO_ROWS:
                continue
            nx, nu, N = d
            name = f"thread64<{nx},{nu}>" if k == 1 else (f"rows64<{nx},{nu},{N}>" if d in F64_ROWS_UNROLLED else f"rows64<{nx},{nu},n<={32 if N <= 32 else 64}>")
            out.append(_case("f64", d, "exact", 130, ("shared", "inst")[(i + k) % 2], 0, 0, name, variant=k))
    return _settle(out)


ROWLANE_CASES, TILE16_CASES, ROWLOOP_CASES, ROWSTREAM_CASES = _rowlane_cases(), _tile16_cases(), _rowloop_cases(), _rowstream_cases()
WAVE_CASES, GENERIC_CASES, STREAM_CASES, FP16_CASES, F64_CASES = _wave_cases(), _generic_cases(), _stream_cases(), _fp16_cases(), _f64_cases()
ALL_CASES = ROWLANE_CASES + TILE16_CASES + ROWLOOP_CASES + ROWSTREAM_CASES + WAVE_CASES + GENERIC_CASES + STREAM_CASES + FP16_CASES + F64_CASES

# x0 amplitudes (smallest, largest instance) where the default (0.02 ... 0.6) does not meet the conditions on the inputs, found on the CPU with the
# oracle's loop alone: a batch of one has to run out of iterations in its first, cold solve and converge in a later one; the (2, 2, 3) class converges
# within a few iterations unless it starts far out
TUNED = {"rowlane-12_4_30-exact-B1-window0": dict(amp=(0.02, 0.3)),
         "rowlane-4_1_10-exact-B1-shared-check_termination3_max_iter24": dict(amp=(0.02, 0.3)),
         "quadlane-4_1_10-exact-B1-shared": dict(amp=(0.02, 1.5)),
         "rowlane-12_4_10-fast-B1-window1": dict(amp=(0.02, 0.08)),
         "rowlane-12_4_50-fast-B1-window2": dict(amp=(0.02, 0.08)),
         "rowloop-2_2_3-exact-B3-shared-check_termination3_max_iter24": dict(amp=(0.02, 1.0)),
         "rowloop-2_2_3-fast-B37-inst": dict(amp=(0.02, 2.5))}
assert set(TUNED) <= {c["id"] for c in ALL_CASES}


def case_problem(pr, O, c):
    nx, nu, N = c["dims"]
    if c.get("quadrotor"):
        return pr.quadrotor(20, N)
    return pr.random_system(nx, nu, N, seed=100 * nx + nu, riccati=O.riccati)


def case_inputs(pr, O, c, B=None):
    """(prob, settings, x0, ref, bnds) of a case, in the library's precision"""
    prob = case_problem(pr, O, c)
    dt = np.float64 if c["fam"] == "f64" else np.float32
    x0, ref, bnds = closed_loop_inputs(prob, B or c["B"], c["ref"], c["seed"], near_end=bool(c.get("near_end")), dtype=dt, **TUNED.get(c["id"], {}))
    return prob, dict(BASE, **c["settings"]), x0, ref, bnds


def _handle(T, c, prob, settings, x0, ref, bnds):
    s = T.TinyBatchSolver(prob, len(x0), settings=settings)
    s.select_kernel(c["variant"])
    if c["variant"] in (2, 3):
        s.set_row_kernel(c["row"])
    if c.get("storage"):
        s.set_storage(*c["storage"])
    s.set_bounds(*bnds)
    if isinstance(ref, tuple):
        s.set_xref_window(*ref)
    else:
        s.set_xref(ref)
    s.set_x0(x0)
    assert s.kernel_name() == c["name"], s.kernel_name()
    assert s.closed_loop_kernel_name() == c.get("loop", c["name"]), s.closed_loop_kernel_name()
    return s


def _check_final(s, want, what, idx=None):
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(pick(got[k]), want["st"][k]), f"{what}: {k} differs after the last step"
    assert same_bits(pick(s.get_x0()), want["x"]), f"{what}: get_x0() differs after the last step"


def _first_diff(a, b):
    return int(np.argmax(np.any((a != b) | (np.signbit(a) != np.signbit(b)), axis=(1, 2))))


def _run(s, chunks, adv, want, what, idx=None):
    """mpc_run_traj in `chunks`: u.col(0) of every step, then iter, status, the workspace and x0 after the last"""
    traj = np.concatenate([s.mpc_run_traj(n, adv) for n in chunks])
    if idx is not None:
        traj = traj[:, idx]
    assert same_bits(traj, want["u0"]), f"{what}: u.col(0) differs from step {_first_diff(traj, want['u0'])} on"
    _check_final(s, want, what, idx)


def _step(s, steps, adv, want, what, idx=None):
    """steps x mpc_step_async: u.col(0), iter and status after every step, then the workspace and x0"""
    for k in range(steps):
        s.mpc_step_async(adv)
        it, stt, _ = s.get_status()
        u0 = s.get_u()[:, 0]
        if idx is not None:
            it, stt, u0 = it[idx], stt[idx], u0[idx]
        assert np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"{what}: iter / status differ after step {k}"
        assert same_bits(u0, want["u0"][k]), f"{what}: u.col(0) differs at step {k}"
    _check_final(s, want, what, idx)


def _reference(T, O, c, prob, settings, x0, ref, bnds, steps=STEPS, orc=None):
    """the case's reference loop; the conditions on the inputs are checked on the oracle's loop whichever reference the case has"""
    if orc is None:
        orc = oracle_closed_loop(O, prob, np.float32, settings, x0, ref, bnds, steps, c["adv"])
        closed_loop_conditions(orc, bnds, settings, c["id"])
    if c["arith"] == "exact" and not c.get("storage"):
        return orc
    h = _handle(T, c, prob, settings, x0, ref, bnds)
    want = host_closed_loop(h, O.Oracle(prob, np.float32).plant_step, x0, ref, steps, c["adv"])
    h.close()
    return want


def _three_ways(T, c, prob, settings, x0, ref, bnds, want, steps=STEPS, k1=K1):
    ways = (("run", (k1, steps - k1)), ("step by step", None), ("run with a single step", (k1, 1, steps - k1 - 1)))
    for way, chunks in ways[:c.get("ways", 3)]:  # (the third where it is cheap)
        s = _handle(T, c, prob, settings, x0, ref, bnds)
        what = f"{c['id']} {way}"
        if chunks:
            _run(s, chunks, c["adv"], want, what)
        else:
            _step(s, steps, c["adv"], want, what)
        s.close()


def _closed_loop(T, O, c):
    prob, settings, x0, ref, bnds = case_inputs(T.problems, O, c)
    want = _reference(T, O, c, prob, settings, x0, ref, bnds)
    _three_ways(T, c, prob, settings, x0, ref, bnds, want)
    return prob, settings, x0, ref, bnds, want


def _ids(cases):
    return [c["id"] for c in cases]


@pytest.mark.parametrize("case", ROWLANE_CASES, ids=_ids(ROWLANE_CASES))
def test_rowlane_on_chip_loop(tinympc, oracle_mod, case):
    """The on-chip loop of every 16-lane class and of the quad kernel, exact and fma, at batches ragged against the wave's four instances and the plant
    block: sliding windows (advance 0, 1, 2, clamping at the table's end), shared and per-instance reference arrays."""
    _closed_loop(tinympc, oracle_mod, case)


@pytest.mark.parametrize("case", TILE16_CASES, ids=_ids(TILE16_CASES))
def test_tile16_on_chip_loop(tinympc, oracle_mod, case):
    """The on-chip loop of every tile16 horizon, exact and fma, past one tile and past one workgroup; the fma loop also equals the 16-lane fma loop."""
    T = tinympc
    prob, settings, x0, ref, bnds, want = _closed_loop(T, oracle_mod, case)
    if case["arith"] == "fast":
        nx, nu, N = case["dims"]
        r = _handle(T, dict(case, row=1, name=f"rowlane<{nx},{nu},{N},fast>"), prob, settings, x0, ref, bnds)
        _run(r, (K1, STEPS - K1), case["adv"], want, f"{case['id']}: the 16-lane fma loop")
        r.close()


@pytest.mark.parametrize("arith", ARITH)
def test_tile16_on_chip_loop_second_tile_per_wave(tinympc, oracle_mod, arith):
    """16 384 + 21 instances, N = 20: the persistent waves take a second tile and the run is dispatched longest first.  fma: from a reset workspace
    (the predictor's order), against the 16-lane fma loop on the whole batch.  exact: in history order after a warm-up solve, against the oracle on a
    sample that includes the last three instances."""
    T, O = tinympc, oracle_mod
    B, N = 16384 + 21, 20
    c = dict(_case("tile16", (12, 4, N), arith, B, "window", 1, 5, f"tile16<12,4,{N},{arith}>"), seed=77, settings={}, id=f"tile16 {arith} B={B}")
    prob, settings, x0, ref, bnds = case_inputs(T.problems, O, c)
    warm = arith == "exact"
    idx = np.unique(np.r_[np.arange(0, B, 271), B - 3, B - 2, B - 1])
    assert idx.size <= 64
    sref, sx0 = (ref[0], ref[1][idx]), x0[idx]
    if warm:
        st = O.new_state(idx.size, 12, 4, N)
        st["x"][:, 0] = sx0
        O.Oracle(prob, np.float32, settings).solve(st, *bnds, ref_at(sref, 0, 0, N, idx.size), nthreads=8)  # the warm-up solve
        want = oracle_closed_loop(O, prob, np.float32, settings, sx0, sref, bnds, STEPS, 1, st=st)
        closed_loop_conditions(want, bnds, settings, c["id"])
    else:
        closed_loop_conditions(oracle_closed_loop(O, prob, np.float32, settings, sx0, sref, bnds, STEPS, 1), bnds, settings, c["id"])
        idx = None
        r = _handle(T, dict(c, row=1, name=f"rowlane<12,4,{N},fast>"), prob, settings, x0, ref, bnds)
        want = dict(u0=np.concatenate([r.mpc_run_traj(K1, 1), r.mpc_run_traj(STEPS - K1, 1)]), st=r.get_state(), x=r.get_x0())
        r.close()
    for way in ("run", "step by step"):
        s = _handle(T, c, prob, settings, x0, ref, bnds)
        if warm:
            s.set_dispatch(2)
            s.solve()
        if way == "run":
            traj = [s.mpc_run_traj(K1, 1)]
            assert s.dispatch_applied() == (3 if warm else 1), s.dispatch_applied()
            traj = np.concatenate(traj + [s.mpc_run_traj(STEPS - K1, 1)])
            assert same_bits(traj if idx is None else traj[:, idx], want["u0"]), f"{c['id']}: u.col(0) differs"
        else:
            for _ in range(STEPS):
                s.mpc_step_async(1)
        _check_final(s, want, f"{c['id']} {way}", idx)
        s.close()


@pytest.mark.parametrize("case", ROWLOOP_CASES + ROWSTREAM_CASES, ids=_ids(ROWLOOP_CASES + ROWSTREAM_CASES))
def test_rowloop_and_rowstream_loop(tinympc, oracle_mod, case):
    """The rolled-loop and the streaming row kernel (graph replay and step by step) with plant_step_kernel on every row class: the lazy-product orders
    of nx = 2, 4, 8, 12 and the GEMV order of Adyn for nx >= 8."""
    _closed_loop(tinympc, oracle_mod, case)


@pytest.mark.parametrize("case", WAVE_CASES, ids=_ids(WAVE_CASES))
def test_wave_kernels_loop(tinympc, oracle_mod, case):
    """wavestream, waveres and tile48 on every wave class; (32, 16), (16, 8) and (20, 8) take the GEMV branch of Bdyn*u in the plant step."""
    _closed_loop(tinympc, oracle_mod, case)


@pytest.mark.parametrize("case", GENERIC_CASES, ids=_ids(GENERIC_CASES))
def test_generic_loop(tinympc, oracle_mod, case):
    """The run-time-dimension exact kernel with shared models (TILE layout of the plant step)."""
    _closed_loop(tinympc, oracle_mod, case)


@pytest.mark.parametrize("case", STREAM_CASES, ids=_ids(STREAM_CASES))
def test_stream_loop(tinympc, oracle_mod, case):
    """The MFMA streaming kernel (fma, TILE layout) against the host-driven loop on a second handle."""
    _closed_loop(tinympc, oracle_mod, case)


@pytest.mark.parametrize("case", FP16_CASES, ids=_ids(FP16_CASES))
def test_fp16_storage_loop(tinympc, oracle_mod, case):
    """fp16 storage with fp32 and with fp16 duals: x.col(0) rounded into storage, x0buf kept fp32, the plant step in the fp32 oracle's order."""
    _closed_loop(tinympc, oracle_mod, case)


# the kernels whose plant step has a GEMV accumulator (nx >= 8): the on-chip loops, the plant kernel on both layouts, Bdyn's GEMV branch (nu >= 8)
ZERO_NAMES = ("rowlane<12,4,10,exact>", "rowlane<12,4,10,fast>", "rowlane<8,3,7,exact>", "tile16<12,4,10,exact>", "tile16<12,4,10,fast>", "rowloop<12,4,exact>",
              "rowloop<8,4,fast>", "waveres<16,4,exact>", "wavestream<32,16,exact>", "tile48<32,16,12,exact>", "generic<20,12,exact>")
ZERO_CASES = [next(c for c in ALL_CASES if c["name"] == n and not c.get("near_end")) for n in ZERO_NAMES]


@pytest.mark.parametrize("case", ZERO_CASES, ids=[c["name"] for c in ZERO_CASES])
def test_plant_step_starts_its_accumulator_at_positive_zero(tinympc, oracle_mod, case):
    """States of signed zeros on a system with positive dynamics (helpers.positive_system): where every product of a row of Adyn*x + Bdyn*u.col(0) is
    -0 the reference returns +0, because Eigen's GEMV accumulator starts at +0; a plant step that starts from the first product returns -0, which
    the negative gain turns into another sign of the next u.col(0).  Four steps, the first plant step inside the on-chip loop where there is one."""
    T, O = tinympc, oracle_mod
    c = dict(case, ref="shared", adv=0, settings={}, id=case["name"] + " signed zeros")
    prob = positive_system(case_problem(T.problems, O, c))
    settings, steps = dict(BASE), 4
    x0, ref, bnds = zero_state_inputs(prob, 37, case["seed"])
    orc = oracle_closed_loop(O, prob, np.float32, settings, x0, ref, bnds, steps, 0)
    lost = rows_of_negative_zeros(prob, x0, orc["u0"][0])
    assert lost[0].all() and not lost[1].any(), "the inputs do not reach the rows of negative zeros"
    want = _reference(T, O, c, prob, settings, x0, ref, bnds, steps, orc=orc)
    _three_ways(T, c, prob, settings, x0, ref, bnds, want, steps, 2)


@pytest.mark.parametrize("case", F64_CASES, ids=_ids(F64_CASES))
def test_fp64_mpc_step(tinympc, oracle_mod, case):
    """tiny_batch64_mpc_step on both fp64 kernels for every compiled class, against the fp64 oracle's closed loop."""
    T, O = tinympc, oracle_mod
    prob, settings, x0, ref, bnds = case_inputs(T.problems, O, case)
    want = oracle_closed_loop(O, prob, np.float64, settings, x0, ref, bnds, STEPS, 0)
    closed_loop_conditions(want, bnds, settings, case["id"])
    s = T.TinyBatchSolver64(prob, case["B"], settings=settings)
    s.select_kernel(case["variant"])
    s.set_bounds(*bnds)
    s.set_xref(ref)
    s.set_x0(x0)
    assert s.kernel_name() == case["name"], s.kernel_name()
    for k in range(STEPS):
        s.mpc_step()
        it, stt, _ = s.get_status()
        assert np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"{case['id']}: iter / status differ after step {k}"
        x, u0 = s.first_columns()
        assert same_bits(u0, want["u0"][k]), f"{case['id']}: u.col(0) differs at step {k}"
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want["st"][k]), f"{case['id']}: {k} differs after the last step"
    assert same_bits(x, want["x"]), f"{case['id']}: x.col(0) differs after the last step"
    s.close()
