"""What the per-step solver log of a closed-loop run costs (tiny_batch_mpc_run_log_async, tiny_batch64_mpc_run_log; run on an MI355X).

    python tools/run_log_cost.py [--batch 65536] [--reps 7] [--root DIR] [--skip64]

fp32: quadrotor tracking instances, N = 30, exact arithmetic, 20 MPC steps per run with window advance 1, on the matrix-core kernel (tile16) and on
the 16-lane kernel (rowlane), ms per MPC step (wall, run + synchronize): the median of `reps` runs behind one warm-up run, and their spread
(min .. max).  Every run starts from the same x0 and window starts on a warm workspace and records u0_traj on the device.
  traj        tiny_batch_mpc_run_traj_async: the call every build has — the figure to compare between two builds (--root another tree)
  NULL logs   tiny_batch_mpc_run_log_async with both logs NULL: what `traj` has become
  logs        ... with both logs
fp64: the same instances at N = 10 on rows64<12,4,10,mpc>, tiny_batch64_mpc_run_traj against tiny_batch64_mpc_run_log with both logs (blocking
calls with host arrays: the read-back of the logs is in the figure).
The script uses nothing a build without the feature lacks unless the symbol is there: on such a build it prints the `traj` rows alone."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

STEPS = 20


def dev_alloc(hip, nbytes):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), nbytes) == 0
    return p


def timed32(T, B, reps, row, mode):
    pr = T.problems
    prob = pr.quadrotor(20, 30)
    x0, table, start = pr.tracking_batch(B, 30, seed=1)
    s = T.TinyBatchSolver(prob, B)
    s.set_bounds(*pr.bounds_arrays(prob))
    s.select_kernel(2)
    s.set_row_kernel(row)
    hip = T.solver._hip()
    du = dev_alloc(hip, STEPS * B * 4 * 4)
    dl = [dev_alloc(hip, STEPS * B * 4) for _ in range(2)] if mode == "logs" else [None, None]
    if mode != "traj":
        fn = s.lib.tiny_batch_mpc_run_log_async
        fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5, C.c_int
    ms = []
    for _ in range(reps + 1):
        s.set_xref_window(table, start)
        s.set_x0(x0)
        s.synchronize()
        t0 = time.perf_counter()
        if mode == "traj":
            s._check(s.lib.tiny_batch_mpc_run_traj_async(s._h, STEPS, 1, du))
        else:
            s._check(fn(s._h, STEPS, 1, None, du, None, dl[0], dl[1]))
        s.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    name, caps, x_end = s.closed_loop_kernel_name(), s.lib.tiny_batch_debug_graph_captures(s._h), s.get_x0()
    unsolved = None
    if mode == "logs":
        st = np.zeros((STEPS, B), np.int32)
        assert hip.hipMemcpy(st.ctypes.data, dl[1], st.nbytes, 2) == 0
        unsolved = int((st == 11).sum())
    s.close()
    for p in [du] + dl:
        if p:
            hip.hipFree(p)
    ms = ms[1:]
    return name, caps, float(np.median(ms)), min(ms), max(ms), x_end, unsolved


def timed64(T, B, reps, logs):
    pr = T.problems
    prob = pr.quadrotor(20, 10)
    x0, table, start = pr.tracking_batch(B, 10)
    x0, table = np.asarray(x0, np.float64), np.asarray(table, np.float64)
    s = T.TinyBatchSolver64(prob, B, settings=dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1))
    s.set_bounds(*pr.bounds_arrays(prob, np.float64))
    zero = s.get_state()
    ms = []
    for _ in range(reps + 1):
        s.set_state(zero); s.set_xref_window(table, start); s.set_x0(x0)
        t0 = time.perf_counter()
        if logs:
            s.mpc_run_log(STEPS, 1)
        else:
            s.mpc_run_traj(STEPS, 1)
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    name = s.closed_loop_kernel_name()
    s.close()
    ms = ms[1:]
    return name, float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--skip64", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import accelerated_tinympc_amd as T
    lib = T.load_library()
    have = hasattr(lib, "tiny_batch_mpc_run_log_async")
    print(f"tree {a.root}: tiny_batch_mpc_run_log_async {'present' if have else 'absent'}", flush=True)
    for row, fam in ((5, "tile16"), (1, "rowlane")):
        base = None
        for mode in ("traj", "NULL logs", "logs") if have else ("traj",):
            name, caps, med, lo, hi, x_end, unsolved = timed32(T, a.batch, a.reps, row, mode)
            base = (med, x_end) if base is None else base
            same = bool(np.array_equal(x_end, base[1]))
            print(f"fp32 B={a.batch} {fam:8s} {mode:>9}: {name:24s} {med:8.4f} ms per MPC step ({lo:.4f} .. {hi:.4f}), x {med / base[0]:5.3f} of traj, graphs captured {caps}, "
                  f"final state {'equal to' if same else 'DIFFERS from'} the traj run's" + (f", {unsolved} unsolved entries in the log" if unsolved is not None else ""), flush=True)
    if a.skip64:
        return
    base = None
    for logs in (False, True) if hasattr(lib, "tiny_batch64_mpc_run_log") else (False,):
        name, med, lo, hi = timed64(T, a.batch, a.reps, logs)
        base = med if base is None else base
        print(f"fp64 B={a.batch} N=10 {'logs' if logs else 'traj':>9}: {name:24s} {med:8.4f} ms per MPC step ({lo:.4f} .. {hi:.4f}), x {med / base:5.3f} of traj", flush=True)


if __name__ == "__main__":
    main()
