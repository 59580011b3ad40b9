"""The frame of tiny_solve around the sweeps (rowlane_math.h: SolveFrame, RowResiduals, RowXref), once per kernel that uses it and per lane
geometry, at the smallest shapes where a frame bug shows: a batch that fills one wave and leaves a ragged one, a warm start whose residual
fields are live-in, a window reference that is clamped to the table's last row for some instances and not for others.

Four settings per case:
  (a) check_termination = 7, max_iter = 5: no termination check happens, so the residual fields must come back as the live-in bits,
      with status 11, iter 5 and all B instances counted unsolved (exact arithmetic: everything bitwise; fma arithmetic: these fields)
  (b) check_termination = 3, max_iter = 40: checks every third iteration, with tolerances (TOL_B below) at which the oracle converges
      some instances — necessarily at a multiple of 3 — and leaves others running or converging at another count
      and once more on the same handle from a reset workspace: the residual fields are zero, not what the first solve left in memory
  (c) max_iter = 0: nothing is written but status 11 / iter 1, B instances counted unsolved
  (d) max_iter = 1
Exact arithmetic is compared bitwise with the oracle: every work array, iter, status, residuals and the count the solve returns.
The unmarked test at the end asserts those input conditions on the oracle alone (no GPU), so that no GPU case is vacuous."""
import numpy as np
import pytest

from helpers import STATE_ORDER

# case -> (set_row_kernel family, kernel_name prefix, (nx, nu, N), batch).  A wave holds 4 instances of the 16-lane kernels, 16 of the
# quad-lane kernel and one of the wave kernels.
CASES = {
    "rowlane_8_3_7": (1, "rowlane<8,3,7", (8, 3, 7), 5),
    "rowlane_12_4_10": (1, "rowlane<12,4,10", (12, 4, 10), 5),
    "quadlane_4_1_10": (4, "quadlane<4,1,10", (4, 1, 10), 17),
    "waveres_16_4_10": (7, "waveres<16,4", (16, 4, 10), 3),
    "wavestream_16_4_10": (6, "wavestream<16,4", (16, 4, 10), 3),
    "rowloop_4_2_8": (2, "rowloop<4,2", (4, 2, 8), 5),
    "rowstream_8_4_9": (3, "rowstream<8,4", (8, 4, 9), 5),
}
SLIDE = 2  # rows by which the windows are slid past what set_xref_window accepts (see test_frame_vs_oracle)
SEED = 7  # one seed for every case: inputs below
# tolerances of setting (b), per class: picked by running the ORACLE alone on the seeded inputs (never the code under test) so that within 40
# iterations some instances converge and some do not or converge at another count; test_frame_cases_are_not_vacuous holds them to that
# (oracle iteration counts at seed 7: (8,3,7) 6 6 6 6 9; (12,4,10) 24 24 24 40 24; (4,1,10) 3 ... 24 ... 39, four at 40; (16,4,10) 6 6 9; (4,2,8) 6 6 6 6 9;
# (8,4,9) 6 6 12 6 9)
TOL_B = {(8, 3, 7): 2e-2, (12, 4, 10): 3e-3, (4, 1, 10): 2e-2, (16, 4, 10): 2e-2, (4, 2, 8): 1e-2, (8, 4, 9): 2e-2}
SETTINGS = {"a": dict(check_termination=7, max_iter=5), "b": dict(check_termination=3, max_iter=40),
            "c": dict(max_iter=0), "d": dict(max_iter=1)}


def settings_of(O, dims, key):
    s = dict(O.DEFAULT_SETTINGS, **SETTINGS[key])
    if key == "b":
        s.update(abs_pri_tol=TOL_B[dims], abs_dua_tol=TOL_B[dims])
    return s


def problem_of(pr, dims):
    nx, nu, N = dims
    return pr.quadrotor(20, N) if (nx, nu) == (12, 4) else pr.cartpole(N) if (nx, nu) == (4, 1) else pr.random_system(nx, nu, N)


def inputs_of(O, pr, dims, B):
    """Warm start: x0, random small d, v, z, y, g, residual fields in (0, 1); a table of N + 2 rows with window starts 2, 3, 4, 2, ...:
    start 2 ends on the table's last row, the others run one and two rows past it and are clamped."""
    nx, nu, N = dims
    rng = np.random.default_rng(SEED)
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = rng.uniform(-0.2, 0.2, size=(B, nx)).astype(np.float32)
    st["residuals"][:] = rng.uniform(0, 1, size=(B, 4)).astype(np.float32)
    for k in ("d", "v", "z", "y", "g"):
        st[k][:] = (rng.standard_normal(st[k].shape) * 0.05).astype(np.float32)
    rows = N + 2
    table = (rng.standard_normal((rows, nx)) * 0.1).astype(np.float32)
    start = (SLIDE + np.arange(B) % 3).astype(np.int32)
    xref = table[np.minimum(start[:, None] + np.arange(N)[None, :], rows - 1)]
    return st, table, start, np.ascontiguousarray(xref)


@pytest.fixture(scope="module")
def frame_refs(oracle_mod, tinympc):
    """(dims, B) -> problem, live-in, window and, per setting, the oracle's live-out and its count of unsolved instances.  Computed once."""
    O, pr = oracle_mod, tinympc.problems
    refs = {}
    for _fam, _name, dims, B in CASES.values():
        if (dims, B) in refs:
            continue
        prob = problem_of(pr, dims)
        pre, table, start, xref = inputs_of(O, pr, dims, B)
        bnds = pr.bounds_arrays(prob)
        post = {}
        for key in SETTINGS:
            st = O.copy_state(pre)
            n = O.Oracle(prob, np.float32, settings_of(O, dims, key)).solve(st, *bnds, xref, nthreads=1)
            post[key] = (st, int(n))
        # (a) once more from a reset workspace: a cold start zeroes the residual fields, whatever the previous solve left in them
        st = O.new_state(B, *dims); st["x"][:, 0] = pre["x"][:, 0]
        n = O.Oracle(prob, np.float32, settings_of(O, dims, "a")).solve(st, *bnds, xref, nthreads=1)
        post["a_cold"] = (st, int(n))
        refs[(dims, B)] = dict(prob=prob, pre=pre, table=table, start=start, bnds=bnds, post=post)
    return refs


def assert_same_bits(got, ref, keys, what):
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].tobytes() == np.ascontiguousarray(ref[k]).tobytes(), f"{what}: {k} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_frame_vs_oracle(tinympc, oracle_mod, frame_refs, case):
    O = oracle_mod
    fam, name, dims, B = CASES[case]
    R = frame_refs[(dims, B)]
    pre = R["pre"]
    for key, fma in [(k, False) for k in SETTINGS] + [("a", True)]:
        if fma and fam == 6:
            continue  # the streaming wave kernel has no fma instantiation (fma arithmetic of its classes is another kernel)
        sol = tinympc.TinyBatchSolver(R["prob"], B, settings=settings_of(O, dims, key))
        sol.select_kernel(3 if fma else 2)
        sol.set_row_kernel(fam)
        assert sol.kernel_name().startswith(name) and sol.kernel_name().endswith("fast>" if fma else "exact>"), sol.kernel_name()
        # set_xref_window accepts windows inside the table only: they get past its end the way a closed loop's do, slid by one MPC step,
        # whose own solve and plant step the live-in then overwrites
        sol.set_bounds(*R["bnds"]); sol.set_xref_window(R["table"], R["start"] - SLIDE)
        sol.mpc_step_async(SLIDE)
        sol.set_state(pre)
        sol.solve_async()
        n = sol.wait()
        got = sol.get_state()
        if key == "a" and not fma:  # the same handle from a reset workspace: the live-in residual bits are still in device memory
            sol.reset_workspace(); sol.set_x0(pre["x"][:, 0])
            sol.solve_async()
            n_cold = sol.wait()
            cold, (ref_cold, n_ref_cold) = sol.get_state(), R["post"]["a_cold"]
            assert not cold["residuals"].any(), f"{case} (a) cold start: residual fields {cold['residuals']}"
            assert_same_bits(cold, ref_cold, STATE_ORDER + ("iter", "status", "residuals"), f"{case} (a) cold start")
            assert n_cold == n_ref_cold == B
        sol.close()
        ref, n_ref = R["post"][key]
        what = f"{case} ({key}){' fma' if fma else ''}"
        print(what, "iter", got["iter"].tolist(), "status", got["status"].tolist(), "unsolved", n)
        if key == "a":  # no check happened: the live-in residual bits, whatever the arithmetic
            assert_same_bits(got, pre, ("residuals",), what)
            assert (got["status"] == 11).all() and (got["iter"] == 5).all() and n == B, what
        if key == "c":  # nothing but status / iter is written
            assert_same_bits(got, pre, STATE_ORDER + ("residuals",), what)
            assert (got["status"] == 11).all() and (got["iter"] == 1).all() and n == B, what
        if not fma:
            assert_same_bits(got, ref, STATE_ORDER + ("iter", "status", "residuals"), what)
            assert n == n_ref, (what, n, n_ref)


def test_frame_cases_are_not_vacuous(oracle_mod, frame_refs):
    """The conditions the GPU cases rely on, on the oracle alone."""
    for (dims, B), R in frame_refs.items():
        N = dims[2]
        pre, post = R["pre"], R["post"]
        # the clamp is reached by some windows and not by others
        last = R["start"] + N - 1
        assert (last > N + 1).any() and (last <= N + 1).any(), (dims, R["start"])
        assert (pre["residuals"] > 0).all() and (pre["residuals"] < 1).all()
        # (a): the oracle itself returns the live-in residuals
        assert not post["a_cold"][0]["residuals"].any() and post["a_cold"][1] == B
        a, n_a = post["a"]
        assert a["residuals"].tobytes() == pre["residuals"].tobytes() and (a["iter"] == 5).all() and (a["status"] == 11).all() and n_a == B, dims
        # (b): some instance converges (at a multiple of 3), and some instance runs out of iterations or converges at another count
        b, n_b = post["b"]
        conv = b["status"] == 1
        assert conv.any() and (b["iter"][conv] % 3 == 0).all(), (dims, b["iter"], b["status"])
        assert (~conv).any() or len(set(b["iter"][conv].tolist())) > 1, (dims, b["iter"], b["status"])
        assert n_b == int((~conv).sum()) and ((b["iter"] == 40) == ~conv).all(), dims
        assert b["residuals"].tobytes() != pre["residuals"].tobytes()
        # (c), (d)
        c, n_c = post["c"]
        assert (c["status"] == 11).all() and (c["iter"] == 1).all() and n_c == B
        assert all(c[k].tobytes() == pre[k].tobytes() for k in STATE_ORDER + ("residuals",)), dims
        d, n_d = post["d"]
        assert (d["iter"] == 1).all() and d["residuals"].tobytes() != pre["residuals"].tobytes(), dims
