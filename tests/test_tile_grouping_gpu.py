"""Tile grouping of the 16-instances-per-wave kernel (tiny_batch_set_tile_grouping; admm_tile16.hip's instance map, dispatch_order.hip's counting
sort by window start).  Grouping changes which sixteen instances share a wave and nothing else: every work array, the iteration counts, status
and residuals must equal those of index-order tiles and of the 16-lane kernel bit for bit; the map must be a permutation sorted by window start,
rebuilt exactly when the starts have moved and absent where grouping does not apply; and on the benchmark batch the tiles the GPU formed must
waste as little lock step as the CPU replay (tests/fuzz/sim_tile_regroup.py) says."""
import numpy as np
import pytest

from helpers import STATE_ORDER
from test_tile_grouping import load_sim

pytestmark = pytest.mark.gpu

SCALARS = ("iter", "status", "residuals")


def assert_bitwise(got, ref, what):
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} is not bitwise equal"
        if got[k].dtype.kind == "f":
            assert np.array_equal(np.signbit(got[k]), np.signbit(ref[k])), f"{what}: {k} differs in the sign of a zero"


def check_map(sol, start, B):
    m, builds = sol.tile_map()
    assert m is not None and m.shape == ((B + 15) // 16 * 16,)
    assert np.array_equal(np.sort(m[:B]), np.arange(B)), "the map is not a permutation of the instances"
    assert (m[B:] == -1).all(), "padding entries go last"
    assert (np.diff(start[m[:B]]) >= 0).all(), "the map is not sorted by window start"
    return m, builds


def cold(sol, x0):
    sol.reset_workspace(); sol.set_x0(x0)
    rc = sol.solve()
    return rc, sol.get_state()


# (N, B, starts, settings): B a multiple of 16 and not, more than one workgroup of four tiles, shuffled / equal starts, the deferred sweep's stores
CASES = {
    "n30_b160_consecutive": (30, 160, "batch", {}),
    "n30_b203_shuffled": (30, 203, "shuffled", {}),
    "n20_b77_shuffled": (20, 77, "shuffled", {}),
    "n30_b50_equal": (30, 50, "equal", {}),
    "n30_b40_max_iter_1": (30, 40, "shuffled", dict(max_iter=1)),
    "n30_b40_max_iter_2": (30, 40, "shuffled", dict(max_iter=2)),
    "n30_b40_max_iter_0": (30, 40, "shuffled", dict(max_iter=0)),
    "n30_b16389_predicted": (30, 16389, "shuffled", {}),   # at least 4 096 groups: the predictor's keys are read through the map
}


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fma"])
@pytest.mark.parametrize("case", list(CASES))
def test_grouping_on_equals_off_and_the_16_lane_kernel_bitwise(tinympc, case, exact):
    pr = tinympc.problems
    N, B, kind, settings = CASES[case]
    prob = pr.quadrotor(20, N)
    x0, table, start = pr.tracking_batch(B, N, seed=B)
    rng = np.random.default_rng(B)
    if kind == "shuffled":
        start = rng.integers(0, len(table) - N + 1, B).astype(np.int32)
        x0 = (table[start] + rng.uniform(-0.05, 0.05, (B, 12))).astype(np.float32)
    elif kind == "equal":
        start = np.full(B, 137, np.int32)
        x0 = (table[start] + rng.uniform(-0.05, 0.05, (B, 12))).astype(np.float32)
    base = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1)
    sol = tinympc.TinyBatchSolver(prob, B, settings=dict(base, **settings))
    sol.select_kernel(2 if exact else 3); sol.set_row_kernel(5); sol.set_dispatch(1)
    sol.set_bounds(*pr.bounds_arrays(prob))
    sol.set_xref_window(table, start)
    assert sol.kernel_name() == f"tile16<12,4,{N},{'exact' if exact else 'fast'}>", sol.kernel_name()
    sol.set_tile_grouping(0)
    rc_off, off = cold(sol, x0)
    assert not sol.tile_grouping_applied() and sol.tile_map()[0] is None
    sol.set_tile_grouping(1)
    rc_on, on = cold(sol, x0)
    runs = settings.get("max_iter", 100) > 0   # (max_iter 0 only sets status and iter: a launch without a cold start, index-order tiles)
    assert sol.tile_grouping_applied() == runs
    if runs:
        check_map(sol, start, B)
    assert sol.dispatch_applied() == (1 if B >= 16384 else 0)
    assert rc_on == rc_off
    assert_bitwise(on, off, f"{case}: grouping on vs off")
    sol.set_row_kernel(1)
    rc_row, row = cold(sol, x0)
    assert sol.kernel_name().startswith("rowlane<") and not sol.tile_grouping_applied()
    assert rc_row == rc_on
    assert_bitwise(on, row, f"{case}: grouped tile16 vs the 16-lane kernel")
    sol.close()


def test_map_follows_the_window_starts_and_clamped_windows(tinympc):
    """The map is built once per set of starts: not again for a second solve, again after set_xref_window with new starts and after mpc_step has slid
    the windows — here past the end of the table, where the kernel clamps them — followed by a reset and a cold solve; results stay those of
    index-order tiles."""
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 150
    x0, table, _ = pr.tracking_batch(B, 30, seed=5)
    rng = np.random.default_rng(5)
    last = len(table) - 30
    start = rng.integers(last - 6, last + 1, B).astype(np.int32)   # at the end of the table: two slides of 4 push every window past it
    states = {}
    for mode in (1, 0):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.select_kernel(2); sol.set_row_kernel(5); sol.set_dispatch(-1); sol.set_tile_grouping(mode)
        sol.set_bounds(*pr.bounds_arrays(prob))
        sol.set_xref_window(table, start)
        _, s0 = cold(sol, x0)
        if mode:
            _, b0 = check_map(sol, start, B)
            cold(sol, x0)
            assert sol.tile_map()[1] == b0, "no rebuild while the starts stand"
            start2 = start[::-1].copy()
            sol.set_xref_window(table, start2)
            cold(sol, x0)
            _, b1 = check_map(sol, start2, B)
            assert b1 == b0 + 1
            sol.set_xref_window(table, start)
            cold(sol, x0)
            assert sol.tile_map()[1] == b1 + 1
        sol.mpc_step_async(4); sol.mpc_step_async(4); sol.synchronize()   # warm-started steps: index-order tiles
        assert not sol.tile_grouping_applied()
        _, s1 = cold(sol, x0)
        if mode:
            assert sol.tile_grouping_applied()
            _, b2 = check_map(sol, start + 8, B)
            assert b2 == b1 + 2
        states[mode] = (s0, s1)
        sol.close()
    assert_bitwise(states[1][0], states[0][0], "first cold solve")
    assert_bitwise(states[1][1], states[0][1], "cold solve on clamped windows")
    assert not np.array_equal(states[1][0]["x"], states[1][1]["x"])   # the slide moved the reference


def test_no_map_where_grouping_does_not_apply(tinympc):
    import ctypes
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B = 120
    x0, table, start = pr.tracking_batch(B, 30, seed=2)
    bnds = pr.bounds_arrays(prob)

    def make(mode=1):
        sol = tinympc.TinyBatchSolver(prob, B)
        sol.select_kernel(2); sol.set_row_kernel(5); sol.set_dispatch(1); sol.set_tile_grouping(mode)
        return sol

    # a shared reference
    sol = make(); sol.set_bounds(*bnds); sol.set_xref(pr.expand_windows(table, start, 30)[0])
    cold(sol, x0)
    assert sol.kernel_name().startswith("tile16<") and not sol.tile_grouping_applied() and sol.tile_map() == (None, 0)
    sol.close()
    # per-instance tables (the pi instantiations)
    sol = make(); sol.set_bounds(*[np.repeat(b[None], B, 0) * np.float32(1.01) for b in bnds]); sol.set_xref_window(table, start)
    cold(sol, x0)
    assert sol.kernel_name().endswith(",pi>") and not sol.tile_grouping_applied() and sol.tile_map() == (None, 0)
    sol.close()
    # a caller's order
    hip = ctypes.CDLL("libamdhip64.so")   # (the HIP runtime the library itself links: no torch in these tests)
    order, d_order = np.arange((B + 3) // 4, dtype=np.int32), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d_order), ctypes.c_size_t(order.nbytes)) == 0
    assert hip.hipMemcpy(d_order, ctypes.c_void_p(order.ctypes.data), ctypes.c_size_t(order.nbytes), 1) == 0
    sol = make(); sol.set_bounds(*bnds); sol.set_xref_window(table, start); sol.set_dispatch_order_device(d_order.value)
    cold(sol, x0)
    assert sol.kernel_name().startswith("tile16<") and not sol.tile_grouping_applied() and sol.tile_map() == (None, 0)
    sol.close()
    hip.hipFree(d_order)
    # the automatic choice below three tiles per wave slot; and switched off
    for mode in (-1, 0):
        sol = make(mode); sol.set_bounds(*bnds); sol.set_xref_window(table, start)
        cold(sol, x0)
        assert sol.kernel_name().startswith("tile16<") and not sol.tile_grouping_applied() and sol.tile_map() == (None, 0)
        sol.close()
    with pytest.raises(Exception):
        make(2)


def test_tiles_the_gpu_formed_waste_what_the_replay_says(tinympc, oracle_mod):
    """The benchmark batch as bench.py runs it (automatic kernel, dispatch and grouping).  From the iteration counts the GPU returned and the map it
    used: the mean over tiles of the largest count is no larger than in index order, and its ratio to the mean count is within 0.01 of the CPU
    replay's figure for the same batch (1.094 against 1.125 in index order), which comes from the oracle's counts and the replay's own sort."""
    sim = load_sim()
    pr = tinympc.problems
    prob = pr.quadrotor(20, 30)
    B, seed = sim.BENCH
    x0, table, start = pr.tracking_batch(B, 30, seed=seed)
    sol = tinympc.TinyBatchSolver(prob, B)
    sol.set_bounds(*pr.bounds_arrays(prob))
    sol.set_xref_window(table, start)
    sol.reset_workspace(); sol.set_x0(x0)
    assert sol.kernel_name() == "tile16<12,4,30,exact>"   # (of the cold-start launch: asked before it)
    sol.solve()
    assert sol.dispatch_applied() == 1
    it = sol.get_status()[0].astype(np.int64)
    grouped = sol.tile_grouping_applied()
    m = check_map(sol, start, B)[0] if grouped else sim.identity_map(B)
    sol.close()
    it_cpu, _, start_cpu = sim.workload(B, seed, nthreads=16)
    assert np.array_equal(start_cpu, start)
    expect = sim.lock_step(it_cpu, sim.group_by_start(start_cpu))
    index_order = sim.lock_step(it_cpu, sim.identity_map(B))
    got = sim.lock_step(it, m)
    print(f"lock step: GPU tiles {got:.4f} (grouped: {grouped}), replay by window start {expect:.4f}, index order {index_order:.4f}, mean count {it.mean():.3f}")
    assert grouped, "the automatic choice groups the benchmark launch (four tiles per wave slot)"
    assert sim.tile_counts(it, m).mean() <= sim.tile_counts(it, sim.identity_map(B)).mean()
    assert abs(got - expect) <= 0.01
    assert abs(expect - 1.094) <= 0.01
