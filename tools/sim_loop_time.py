"""The simulated closed loop (tiny_batch_set_plant, tiny_batch_mpc_run_sim_async) against the nominal on-chip loop and against the same run step by step.

    python tools/sim_loop_time.py [--batches 65536 16] [--reps 7] [--root DIR]

Quadrotor tracking instances, N = 30, exact 16-lane kernel forced, 20 MPC steps per run, ms per MPC step (wall, run + synchronize): the median of
`reps` runs behind one warm-up run, and their spread (min .. max).  Every run starts from the same x0 and window starts on a warm workspace.
The plant is the model's own Adyn / Bdyn (once shared, once replicated per instance) and the disturbance is an array of -0, so that every variant
does the SAME ADMM work (bitwise the nominal trajectory): the differences are the cost of the feature, not of another trajectory.
  nominal        tiny_batch_mpc_run_async, no plant                       (one launch)
  shared plant   set_plant(shared)                                         (one launch, admm_rowsim.hip)
  inst plants    set_plant(per instance)
  + w            ... with the disturbance
  + w + x_traj   ... and the state trajectory
  step by step   the last variant as 20 x tiny_batch_mpc_step_sim_async    (solve + plant kernel per step; x_traj is not available there)
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

STEPS, N = 20, 30


class DevBuf:
    def __init__(self, hip, nbytes, host=None):
        self.hip, self.p = hip, C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), nbytes) == 0
        if host is not None:
            assert hip.hipMemcpy(self.p, host.ctypes.data, nbytes, 1) == 0

    def at(self, byte_offset):
        return C.c_void_p(self.p.value + byte_offset)

    def free(self):
        self.hip.hipFree(self.p)


def timed(T, B, reps, plant=None, w=False, xtraj=False, stepwise=False):
    pr = T.problems
    prob = pr.quadrotor(20, N)
    x0, table, start = pr.tracking_batch(B, N, seed=1)
    s = T.TinyBatchSolver(prob, B)
    s.set_bounds(*pr.bounds_arrays(prob))
    s.select_kernel(2)
    s.set_row_kernel(1)
    A, Bm = np.asarray(prob["Adyn"], np.float32), np.asarray(prob["Bdyn"], np.float32)
    if plant == "shared":
        s.set_plant(A, Bm)
    elif plant == "inst":
        s.set_plant(np.broadcast_to(A, (B, 12, 12)), np.broadcast_to(Bm, (B, 12, 4)))
    hip = T.solver._hip()
    row = B * 12 * 4
    dw = DevBuf(hip, STEPS * row, np.full((STEPS, B, 12), -0.0, np.float32)) if w else None
    dx = DevBuf(hip, STEPS * row) if xtraj else None
    ms = []
    for _ in range(reps + 1):
        s.set_xref_window(table, start)
        s.set_x0(x0)
        s.synchronize()
        t0 = time.perf_counter()
        if stepwise:
            for k in range(STEPS):
                s._check(s.lib.tiny_batch_mpc_step_sim_async(s._h, 1, dw.at(k * row) if dw else None))
        elif plant is None and not w and not xtraj:
            s.mpc_run_async(STEPS, 1)
        else:
            s._check(s.lib.tiny_batch_mpc_run_sim_async(s._h, STEPS, 1, dw.p if dw else None, None, dx.p if dx else None))
        s.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
    name, caps, x_end = s.closed_loop_kernel_name(), s.lib.tiny_batch_debug_graph_captures(s._h), s.get_x0()
    s.close()
    for b in (dw, dx):
        if b:
            b.free()
    ms = ms[1:]
    return name, caps, float(np.median(ms)), min(ms), max(ms), x_end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import accelerated_tinympc_amd as T
    rows = [("nominal", {}), ("shared plant", dict(plant="shared")), ("inst plants", dict(plant="inst")), ("inst plants + w", dict(plant="inst", w=True)),
            ("inst plants + w + x_traj", dict(plant="inst", w=True, xtraj=True)), ("step by step (inst + w)", dict(plant="inst", w=True, stepwise=True))]
    for B in a.batches:
        base = None
        for label, kw in rows:
            name, caps, med, lo, hi, x_end = timed(T, B, a.reps, **kw)
            base = (med, x_end) if base is None else base
            same = bool(np.array_equal(x_end, base[1]))
            print(f"B={B:6d} {label:>26}: {name:24s} {med * 1e3:9.1f} us per MPC step ({lo * 1e3:.1f} .. {hi * 1e3:.1f}), x {med / base[0]:5.2f} of nominal, "
                  f"graphs captured {caps}, final state {'equal to' if same else 'DIFFERS from'} the nominal run's", flush=True)


if __name__ == "__main__":
    main()
