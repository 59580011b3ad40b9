"""The headline instantiation admm_tile16_kernel<30, exact, cold> runs each sweep of an ADMM iteration under one narrowed EXEC: an instance that
has converged is switched off for whole sweeps instead of being masked at each state update (admm_tile16.hip: exec_narrow).  What that could break
is the state of a column that is off while its neighbours in the tile go on — so every work array, iter, status and the residuals are compared
bit for bit, zero signs included, with the 16-lane kernel and with the oracle, on batches of 53 (three whole tiles and a padded one) and 16
instances, in settings that keep EXEC partial for many iterations.  Every case also asserts, on the oracle's own counts, that it is the case it
claims to be (`claim`)."""
import numpy as np
import pytest

from helpers import STATE_ORDER

pytestmark = pytest.mark.gpu

N = 30
SCALARS = ("iter", "status", "residuals")
BASE = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1)
BATCHES = (53, 16)


def assert_bitwise(got, ref, what):
    for k in STATE_ORDER + SCALARS:
        assert np.array_equal(got[k], ref[k]), f"{what}: {k} is not bitwise equal"
        if got[k].dtype.kind == "f":
            assert np.array_equal(np.signbit(got[k]), np.signbit(ref[k])), f"{what}: {k} differs in the sign of a zero"


def clamped_windows(table, start, n=N):
    """the window the kernels read: rows beyond the table's end are its last row"""
    idx = np.minimum(start[:, None].astype(np.int64) + np.arange(n)[None, :], len(table) - 1)
    return np.ascontiguousarray(table[idx])


def spread_batch(pr, B, seed, scale=0.05, start=None):
    """window starts spread over the table, the last six at its end; x0 beside the window's first row, at a distance of `scale` (per instance)"""
    _, table, _ = pr.tracking_batch(B, N, seed=seed)
    rng = np.random.default_rng(seed)
    last = len(table) - N
    if start is None:
        start = rng.integers(0, last + 1, B).astype(np.int32)
        start[-6:] = last - np.arange(6, dtype=np.int32)
    sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))[:, None]
    x0 = (table[start] + sc * rng.uniform(-1.0, 1.0, (B, 12))).astype(np.float32)
    return x0, table, start


# ---- the cases: (pr, B) -> inputs, settings, what the GPU run does, and the claim about the oracle's result ----
def case_windows(pr, B):
    """(a) starts spread over the table, the last six at its end"""
    x0, table, start = spread_batch(pr, B, seed=B)
    return dict(x0=x0, table=table, start=start, claim=lambda ref: (ref["status"] == 1).all() and len(set(ref["iter"].tolist())) >= 3)


def case_windows_past_the_end(pr, B):
    """(a) ... and after two slides of four rows: the last six windows reach past the table's end (the clamped rows)"""
    c = case_windows(pr, B)
    assert (c["start"] + 8 > len(c["table"]) - N).sum() >= 6
    return dict(c, slides=2)


def case_windows_beyond_the_table(pr, B):
    """(a) ... and after two slides of twenty rows: every window that started in the table's last 40 rows now STARTS at or beyond its last row
    (the clamp of the start itself, not only of the rows behind it)"""
    c = case_windows(pr, B)
    assert (c["start"] + 40 >= len(c["table"])).sum() >= 6
    return dict(c, slides=2, advance=20)


def hover_batch(B, seed, scale, n=N):
    """a zero reference (hover at the origin) read through windows of a zero table; x0 at a distance of `scale` (per instance) from it: the
    iteration count of an instance then follows its distance (on the tracking table the moving reference alone takes 13 iterations or more)"""
    table = np.zeros((64, 12), np.float32)
    rng = np.random.default_rng(seed)
    start = rng.integers(0, len(table) - n + 1, B).astype(np.int32)
    sc = np.broadcast_to(np.asarray(scale, np.float64), (B,))[:, None]
    return (sc * rng.uniform(-1.0, 1.0, (B, 12))).astype(np.float32), table, start


def case_staggered(pr, B, n=N):
    """(b) max_iter 12 and distances from the reference between 1e-4 and 0.5 inside every tile: columns converge one after the other while others
    run to max_iter — EXEC is partial for most iterations, and the deferred backward sweep runs in the epilogue.  (One window start: the tiles
    are the index-order ones with the grouping on and off.)"""
    x0, table, start = hover_batch(B, 100 + B, np.geomspace(1e-4, 0.5, 16)[np.arange(B) % 16], n)
    start[:] = 7

    def claim(ref):
        ok = True
        for t in range(0, (B // 16) * 16, 16):
            it, stt = ref["iter"][t:t + 16], ref["status"][t:t + 16]
            print(f"tile {t // 16}: iterations {it.tolist()} solved {(stt == 1).astype(int).tolist()}")
            ok = ok and len(set(it[stt == 1].tolist())) >= 3 and bool(((stt != 1) & (it == 12)).any())
        return ok
    return dict(x0=x0, table=table, start=start, settings=dict(BASE, max_iter=12), groupings=(0, 1), claim=claim)


def case_max_iter(max_iter):
    def case(pr, B):
        """(c) the deferred sweep alone (max_iter 1) and behind one sweep of the loop (2); every third column starts on the reference and converges at once"""
        x0, table, start = hover_batch(B, 200 + B, np.where(np.arange(B) % 3 == 0, 0.0, 0.05))
        claim = lambda ref: (ref["status"][::3] == 1).all() and (ref["iter"][::3] == 1).all() and (ref["status"] != 1).any() and ref["iter"].max() == max_iter
        return dict(x0=x0, table=table, start=start, settings=dict(BASE, max_iter=max_iter), claim=claim)
    return case


def case_check_every_third(pr, B):
    """(d) check_termination 3: the residuals are stale between checks, and columns leave at iterations 3, 6, 9, ... only"""
    x0, table, start = spread_batch(pr, B, seed=300 + B, scale=np.geomspace(1e-4, 0.1, 16)[np.arange(B) % 16])

    def claim(ref):
        it = ref["iter"][ref["status"] == 1]
        return it.size > 0 and (it % 3 == 0).all() and len(set(it.tolist())) >= 2
    return dict(x0=x0, table=table, start=start, settings=dict(BASE, check_termination=3), claim=claim)


def case_zeros_in_x0(pr, B):
    """(e) rows of x0 that are exactly zero, of either sign: products and sums of zeros keep their signs"""
    x0, table, start = spread_batch(pr, B, seed=400 + B)
    rng = np.random.default_rng(B)
    zero = rng.random((B, 12)) < 0.4
    x0[zero] = 0.0
    x0[zero & (rng.random((B, 12)) < 0.5)] = -0.0
    assert (zero.sum(1) >= 2).mean() > 0.8
    return dict(x0=x0, table=table, start=start, claim=lambda ref: (ref["iter"] > 1).any())


def case_first_iteration(pr, B):
    """(f) a zero reference; every other instance starts on it (all residuals zero: solved in iteration 1, off for the rest of its tile's solve)"""
    x0, table, start = hover_batch(B, 500 + B, np.where(np.arange(B) % 2 == 0, 0.0, 0.05))
    claim = lambda ref: (ref["iter"][::2] == 1).all() and (ref["status"][::2] == 1).all() and (ref["iter"][1::2] > 1).all()
    return dict(x0=x0, table=table, start=start, groupings=(0, 1), claim=claim)


def case_second_solve(pr, B):
    """(g) two cold solves on one handle, with the tile grouping on and off: the second starts from the reset workspace like the first"""
    x0, table, start = spread_batch(pr, B, seed=600 + B)
    return dict(x0=x0, table=table, start=start, groupings=(0, 1), solves=2, claim=lambda ref: (ref["iter"] > 1).all())


CASES = {"a_windows": case_windows, "a_windows_past_the_end": case_windows_past_the_end,
         "a_windows_beyond_the_table": case_windows_beyond_the_table, "b_staggered": case_staggered,
         "c_max_iter_1": case_max_iter(1), "c_max_iter_2": case_max_iter(2), "d_check_every_third": case_check_every_third,
         "e_zeros_in_x0": case_zeros_in_x0, "f_first_iteration": case_first_iteration, "g_second_solve": case_second_solve}


def oracle_state(O, pr, prob, case, n=N):
    x0 = case["x0"]
    st = O.new_state(len(x0), 12, 4, n)
    st["x"][:, 0] = x0
    xref = clamped_windows(case["table"], case["start"] + case.get("advance", 4) * case.get("slides", 0), n)
    O.Oracle(prob, np.float32, case.get("settings", BASE)).solve(st, *pr.bounds_arrays(prob), xref, nthreads=8)
    return st


def cold(sol, x0):
    sol.reset_workspace(); sol.set_x0(x0)
    sol.solve()
    return sol.get_state()


def gpu_states(T, prob, case, n=N):
    """{(kernel, grouping, solve number): state}: the headline kernel with the tile grouping as the case asks, and the 16-lane kernel"""
    pr, x0 = T.problems, case["x0"]
    out = {}
    for row_kernel, modes in ((5, case.get("groupings", (1,))), (1, (0,))):
        for mode in modes:
            sol = T.TinyBatchSolver(prob, len(x0), settings=case.get("settings", BASE))
            sol.select_kernel(2); sol.set_row_kernel(row_kernel); sol.set_dispatch(1); sol.set_tile_grouping(mode)
            sol.set_bounds(*pr.bounds_arrays(prob))
            sol.set_xref_window(case["table"], case["start"])
            if row_kernel == 5:
                assert sol.kernel_name() == f"tile16<12,4,{n},exact>", sol.kernel_name()
            for _ in range(case.get("slides", 0)):   # warm-started MPC steps, each sliding every window by four (`advance`) rows
                sol.mpc_step_async(case.get("advance", 4))
            sol.synchronize()
            for k in range(case.get("solves", 1)):
                out[("tile16" if row_kernel == 5 else "rowlane", mode, k)] = cold(sol, x0)
            if row_kernel == 1:
                assert sol.kernel_name().startswith("rowlane<"), sol.kernel_name()
            sol.close()
    return out


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", list(CASES))
def test_headline_kernel_equals_the_16_lane_kernel_and_the_oracle_bitwise(tinympc, oracle_mod, name, B):
    pr = tinympc.problems
    prob = pr.quadrotor(20, N)
    case = CASES[name](pr, B)
    ref = oracle_state(oracle_mod, pr, prob, case)
    assert case["claim"](ref), f"{name}: the oracle's result is not the case the test describes"
    for key, st in gpu_states(tinympc, prob, case).items():
        assert_bitwise(st, ref, f"{name}, batch {B}: {key} vs the oracle")


@pytest.mark.parametrize("n", [25, 20, 10])
def test_the_other_horizons_with_staggered_convergence(tinympc, oracle_mod, n):
    """the exact cold-start instantiations of the other horizons run their sweeps the same way: case (b) on each, 53 instances"""
    pr = tinympc.problems
    prob = pr.quadrotor(20, n)
    case = case_staggered(pr, 53, n)
    ref = oracle_state(oracle_mod, pr, prob, case, n)
    assert case["claim"](ref), f"N = {n}: the oracle's result is not the case the test describes"
    for key, st in gpu_states(tinympc, prob, case, n).items():
        assert_bitwise(st, ref, f"staggered convergence, N = {n}: {key} vs the oracle")
