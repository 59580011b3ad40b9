"""The fp64 library's multi-step closed loop (tiny_batch64_mpc_run / _traj with tiny_batch64_set_xref_window) against the fp64 oracle's closed loop, bit
for bit, signs of zeros included: u.col(0) of every step, iter and status, x.col(0), the twelve work arrays, the four residual fields and the window
starts after the last step.

Eleven rows: the unrolled on-chip instantiations (two waves per SIMD, slack in registers, slack in LDS, nu = 1 with the sequential plant sum), the
capacity-32 run-time-horizon body up to its edge, and the launch sequence (the capacity-64 body, a class without a sixteen-lane kernel, the
thread-per-instance kernel by choice).  closed_loop_kernel_name() is asserted on every handle, so no row can run on another path.  Every row is
driven four ways: one run of eight steps; a run of three and a run of five (the hand-over of x0, the workspace and the window between two runs);
eight runs of one step; and, where nothing slides, eight calls of the existing tiny_batch64_mpc_step.  The inputs of every row make some instance
run out of iterations, some converge early and some input sit on its bound (helpers.closed_loop_conditions; tests/test_closed_loop64_host.py checks
the same on the CPU alone)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from helpers import SCALAR_ORDER, STATE_ORDER, closed_loop_conditions, closed_loop_inputs, oracle_closed_loop, ref_at, same_bits
from test_closed_loop_gpu import BASE

pytestmark = pytest.mark.gpu

STEPS, K1 = 8, 3
EINVAL = -1  # TINY_BATCH_EINVAL


def _row(name, dims, B, ref, adv, settings=None, kernel=0, **kw):
    return dict(name=name, dims=dims, B=B, ref=ref, adv=adv, settings=settings or {}, kernel=kernel, **kw)


# name: what closed_loop_kernel_name() must report; kernel: tiny_batch64_select_kernel's argument; seed = 6400 + position
ROWS = [
    _row("rows64<12,4,10,mpc>", (12, 4, 10), 130, "window", 1),                                               # two waves per SIMD
    _row("rows64<12,4,30,mpc>", (12, 4, 30), 37, "window", 2, near_end=True),                                 # slack in LDS; clamps while sliding
    _row("rows64<12,4,20,mpc>", (12, 4, 20), 5, "inst", 0, dict(max_iter=1)),                                 # every solve ends through keep_d
    _row("rows64<4,1,10,mpc>", (4, 1, 10), 130, "shared", 0, dict(check_termination=3, max_iter=24)),         # residual fields carried; nu = 1
    _row("rows64<8,4,9,mpc>", (8, 4, 9), 3, "window", 0),
    _row("rows64<12,2,n<=32,mpc>", (12, 2, 13), 37, "window", 1, dict(check_termination=2)),
    _row("rows64<4,4,n<=32,mpc>", (4, 4, 32), 5, "inst", 0),                                                  # capacity edge
    _row("rows64<12,4,n<=64>", (12, 4, 40), 5, "window", 1),                                                  # launch sequence
    _row("thread64<16,4>", (16, 4, 10), 130, "window", 2, near_end=True),                                     # launch sequence, no rows kernel
    _row("thread64<12,4>", (12, 4, 10), 1, "shared", 0, kernel=1, amp=(0.02, 0.3)),
    _row("rows64<12,4,10,mpc>", (12, 4, 10), 1, "window", 1, amp=(0.02, 0.3)),
]
for _i, _r in enumerate(ROWS):
    _r["seed"] = 6400 + _i
    _r["id"] = "{}-{}_{}_{}-B{}-{}{}".format(_i, *_r["dims"], _r["B"], _r["ref"], _r["adv"])


def row_inputs(pr, O, r):
    """(prob, settings, x0, ref, bnds) of a row in float64"""
    nx, nu, N = r["dims"]
    prob = pr.random_system(nx, nu, N, seed=100 * nx + nu, riccati=O.riccati)
    kw = dict(amp=r["amp"]) if "amp" in r else {}
    x0, ref, bnds = closed_loop_inputs(prob, r["B"], r["ref"], r["seed"], near_end=bool(r.get("near_end")), dtype=np.float64, **kw)
    return prob, dict(BASE, **r["settings"]), x0, ref, bnds


def row_reference(pr, O, r):
    """the oracle's closed loop of a row; the conditions on its inputs are asserted before anything is compared with it"""
    prob, settings, x0, ref, bnds = row_inputs(pr, O, r)
    want = oracle_closed_loop(O, prob, np.float64, settings, x0, ref, bnds, STEPS, r["adv"])
    closed_loop_conditions(want, bnds, settings, r["id"])
    return prob, settings, x0, ref, bnds, want


_REFERENCES = {}


def _reference(T, O, r):
    """computed once per row and shared by the tests that need it; nobody writes to it"""
    if r["id"] not in _REFERENCES:
        _REFERENCES[r["id"]] = row_reference(T.problems, O, r)
    return _REFERENCES[r["id"]]


def _handle(T, r, prob, settings, x0, ref, bnds, name=None):
    s = T.TinyBatchSolver64(prob, len(x0), settings=settings)
    s.select_kernel(r["kernel"])
    s.set_bounds(*bnds)
    if isinstance(ref, tuple):
        s.set_xref_window(*ref)
    else:
        s.set_xref(ref)
    s.set_x0(x0)
    assert s.closed_loop_kernel_name() == (name or r["name"]), s.closed_loop_kernel_name()
    return s


def _check_final(s, r, ref, want, what):
    got = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(got[k], want["st"][k]), f"{what}: {k} differs after the last step"
    assert same_bits(s.first_columns()[0], want["x"]), f"{what}: x.col(0) differs after the last step"
    if isinstance(ref, tuple):
        assert np.array_equal(s.xref_start(), ref[1] + STEPS * r["adv"]), f"{what}: the window starts after the run"


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_mpc_run_equals_the_oracle_loop(tinympc, oracle_mod, row):
    T, O, r = tinympc, oracle_mod, row
    prob, settings, x0, ref, bnds, want = _reference(T, O, r)
    adv = r["adv"]

    # 1. one run of all steps
    s = _handle(T, r, prob, settings, x0, ref, bnds)
    traj = s.mpc_run_traj(STEPS, adv)
    assert same_bits(traj, want["u0"]), f"{r['id']}: u.col(0) of the run differs"
    it, stt, _ = s.get_status()
    assert np.array_equal(it, want["iter"][-1]) and np.array_equal(stt, want["status"][-1]), f"{r['id']}: iter / status of the last step"
    _check_final(s, r, ref, want, r["id"] + " one run")
    s.close()

    # 2. two runs: x0, the workspace and the window are handed over
    s = _handle(T, r, prob, settings, x0, ref, bnds)
    rc = s.mpc_run(K1, adv)
    assert rc == int((want["status"][K1 - 1] != 1).any()), f"{r['id']}: mpc_run returns what the last step's solve returns"
    traj = s.mpc_run_traj(STEPS - K1, adv)
    assert same_bits(traj, want["u0"][K1:]), f"{r['id']}: u.col(0) of the second run differs"
    _check_final(s, r, ref, want, r["id"] + " two runs")
    s.close()

    # 3. step by step through mpc_run(1)
    s = _handle(T, r, prob, settings, x0, ref, bnds)
    for k in range(STEPS):
        rc = s.mpc_run(1, adv)
        it, stt, _ = s.get_status()
        assert np.array_equal(it, want["iter"][k]) and np.array_equal(stt, want["status"][k]), f"{r['id']}: iter / status differ after step {k}"
        assert rc == int((want["status"][k] != 1).any())
    _check_final(s, r, ref, want, r["id"] + " runs of one step")
    s.close()

    # 4. the existing closed-loop step, where nothing slides and the reference is an array
    if adv == 0 and not isinstance(ref, tuple):
        s = _handle(T, r, prob, settings, x0, ref, bnds)
        for k in range(STEPS):
            s.mpc_step()
        _check_final(s, r, ref, want, r["id"] + " tiny_batch64_mpc_step")
        s.close()


# the capacity-32 body's on-chip loop for the classes no row above holds: 5 instances (one full group of four and a tail group), the smallest horizon
# that selects the body, max_iter = 10.  (4, 2) is also the one class whose run-time plant kernel no row reaches.
REMAINING = [_row(f"rows64<{nx},{nu},n<=32,mpc>", (nx, nu, 3), 5, "window", 1, dict(max_iter=10), seed=6450 + i, id=f"{nx}_{nu}_3-B5-window1")
             for i, (nx, nu) in enumerate([(12, 4), (4, 1), (8, 4), (4, 2)])]


@pytest.mark.parametrize("row", REMAINING, ids=[r["id"] for r in REMAINING])
def test_mpc_run_on_the_remaining_capacity_32_classes(tinympc, oracle_mod, row):
    """a run of three and a run of five steps against the oracle's loop (the inputs are not held to helpers.closed_loop_conditions: the rows are here
    for the instantiation they reach)"""
    T, O, r = tinympc, oracle_mod, row
    prob, settings, x0, ref, bnds = row_inputs(T.problems, O, r)
    want = oracle_closed_loop(O, prob, np.float64, settings, x0, ref, bnds, STEPS, r["adv"])
    s = _handle(T, r, prob, settings, x0, ref, bnds)
    traj = np.concatenate([s.mpc_run_traj(K1, r["adv"]), s.mpc_run_traj(STEPS - K1, r["adv"])])
    assert same_bits(traj, want["u0"]), f"{r['id']}: u.col(0) of the runs differs"
    it, stt, _ = s.get_status()
    assert np.array_equal(it, want["iter"][-1]) and np.array_equal(stt, want["status"][-1]), f"{r['id']}: iter / status of the last step"
    _check_final(s, r, ref, want, r["id"])
    s.close()


@pytest.mark.parametrize("kernel", [1, 2])
def test_window_reference_outside_a_run(tinympc, oracle_mod, kernel):
    """solve() with a window equals solve() with the gathered [B][N][nx] array uploaded through set_xref; set_xref after a window returns to the array."""
    T, O = tinympc, oracle_mod
    r = _row("", (12, 4, 10), 5, "window", 0, kernel=kernel)
    r["seed"], r["id"] = 6450, "window-solve"
    prob, settings, x0, (table, start), bnds = row_inputs(T.problems, O, r)
    other = np.ascontiguousarray(table[::-1][:10] * 0.5)[None].repeat(5, axis=0)

    def solved(set_ref):
        s = T.TinyBatchSolver64(prob, 5, settings=settings)
        s.select_kernel(kernel)
        s.set_bounds(*bnds)
        set_ref(s)
        s.set_x0(x0)
        s.solve()
        st = s.get_state()
        s.close()
        return st

    def window_then_array(s):
        s.set_xref_window(table, start)
        s.set_xref(other)

    win = solved(lambda s: s.set_xref_window(table, start))
    arr = solved(lambda s: s.set_xref(ref_at((table, start), 0, 0, 10, 5)))
    back = solved(window_then_array)
    plain = solved(lambda s: s.set_xref(other))
    assert not same_bits(arr["q"], plain["q"]), "the two references must differ for this test to show anything"
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(win[k], arr[k]), f"{k}: window and gathered array differ"
        assert same_bits(back[k], plain[k]), f"{k}: set_xref after a window does not return to the array"


def test_argument_checks(tinympc, oracle_mod):
    T, O = tinympc, oracle_mod
    r = ROWS[0]
    prob, settings, x0, (table, start), bnds = row_inputs(T.problems, O, r)
    s = _handle(T, r, prob, settings, x0, (table, start), bnds)
    s.mpc_run(2, 1)
    before, start_before = s.get_state(), s.xref_start()
    traj = np.zeros((1, s.B, s.nu))
    for steps, adv in ((0, 0), (-3, 1), (1, -1), (4, -1)):
        assert s.lib.tiny_batch64_mpc_run(s._h, steps, adv) == EINVAL, (steps, adv)
        assert s.lib.tiny_batch64_mpc_run_traj(s._h, steps, adv, s._dp(traj)) == EINVAL, (steps, adv)
    after = s.get_state()
    for k in STATE_ORDER + SCALAR_ORDER:
        assert same_bits(before[k], after[k]), f"{k} changed by a refused call"
    assert np.array_equal(start_before, s.xref_start())
    N = prob["N"]
    with pytest.raises(T.TinyBatchError, match="rc=-1"):
        s.set_xref_window(table[:N - 1], np.zeros(s.B, np.int32))                 # rows < N
    with pytest.raises(T.TinyBatchError, match="rc=-1"):
        s.set_xref_window(table, np.full(s.B, len(table) - N + 1, np.int32))      # start + N > rows
    bad = start.copy(); bad[-1] = -1
    with pytest.raises(T.TinyBatchError, match="rc=-1"):
        s.set_xref_window(table, bad)
    assert np.array_equal(start_before, s.xref_start()), "a refused window leaves the old one in place"
    s.set_xref_window(table, np.full(s.B, len(table) - N, np.int32))              # the last window that fits is accepted
    s.close()
    # without a window the advance is ignored and there are no starts to read
    r = ROWS[3]
    prob, settings, x0, ref, bnds, want = _reference(T, O, r)
    s = _handle(T, r, prob, settings, x0, ref, bnds)
    traj = s.mpc_run_traj(STEPS, 3)
    assert same_bits(traj, want["u0"])
    with pytest.raises(T.TinyBatchError, match="rc=-1"):
        s.xref_start()
    s.close()


def test_fuzz_mpc64_short_run():
    """a few seconds of tests/fuzz/fuzz_mpc64.py with a fixed seed: keeps the tool working and replays the cases it draws"""
    root = Path(__file__).resolve().parents[1]
    r = subprocess.run([sys.executable, str(root / "tests" / "fuzz" / "fuzz_mpc64.py"), "--seconds", "5", "--seed", "1"], capture_output=True, text=True,
                       timeout=300, cwd=root)
    assert r.returncode == 0 and "fuzz ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
