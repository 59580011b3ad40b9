"""The fp64 library's simulated closed loop (tiny_batch64_set_plant, tiny_batch64_mpc_run_sim) against the nominal on-chip loop and against the same
run step by step.

    python tools/sim_loop64_time.py [--batches 65536 16] [--horizons 10 30] [--reps 7] [--steps K] [--root DIR]

Quadrotor tracking instances, window advance 1, ms per MPC step (wall around the blocking calls): the median of `reps` runs behind one warm-up run, and
their spread (min .. max).  Every run starts from the same x0 and window starts on a warm workspace.  The plant is the model's own Adyn / Bdyn (once
shared, once replicated per instance) and the disturbance is an array of -0, so that every variant does the SAME ADMM work (bitwise the nominal
trajectory): the differences are the cost of the feature, not of another trajectory.
  nominal              tiny_batch64_mpc_run, no plant                           (one launch, rows64<...,mpc>)
  shared plant         set_plant(shared), tiny_batch64_mpc_run                  (one launch, rows64<...,sim>)
  inst plants          set_plant(per instance), tiny_batch64_mpc_run
  + w + x_traj         ... tiny_batch64_mpc_run_sim with the disturbance and the state trajectory (both cross the host boundary: blocking calls on host pointers)
  step by step         the same simulated run as K x tiny_batch64_mpc_step_sim   (solve + plant kernel per step; the host slides no window: advance 0)
--classes times every SIM instantiation (seeded random systems, one plant per instance, no host arrays) on chip and with TINYMPC_F64_LOOP=sequence,
the launch sequence over its one-solve kernel: the yardstick that decides whether a SIM instantiation keeps the on-chip path."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np


def timed(T, B, N, steps, reps, plant=None, sim=False, stepwise=False):
    pr = T.problems
    prob = pr.quadrotor(20, N)
    x0, table, start = pr.tracking_batch(B, N, seed=1)
    x0, table = np.asarray(x0, np.float64), np.asarray(table, np.float64)
    s = T.TinyBatchSolver64(prob, B)
    s.set_bounds(*pr.bounds_arrays(prob, np.float64))
    A, Bm = np.asarray(prob["Adyn"], np.float64), np.asarray(prob["Bdyn"], np.float64)
    if plant == "shared":
        s.set_plant(A, Bm)
    elif plant == "inst":
        s.set_plant(np.broadcast_to(A, (B, 12, 12)), np.broadcast_to(Bm, (B, 12, 4)))
    w = np.full((steps, B, 12), -0.0) if sim or stepwise else None
    u0 = np.zeros((steps, B, 4))
    xt = np.zeros((steps, B, 12))
    dp = s._dp
    ms = []
    for _ in range(reps + 1):
        s.set_xref_window(table, start)
        s.set_x0(x0)
        s.first_columns()  # blocks until the device is idle
        t0 = time.perf_counter()
        if stepwise:
            for k in range(steps):
                s._check(s.lib.tiny_batch64_mpc_step_sim(s._h, dp(w[k])))
        elif sim:
            s._check(s.lib.tiny_batch64_mpc_run_sim(s._h, steps, 1, dp(w), None, dp(xt)))
        else:
            s.mpc_run(steps, 1)
        x_end = s.first_columns()[0]
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    name = s.closed_loop_kernel_name()
    s.close()
    ms = ms[1:]
    return name, float(np.median(ms)), min(ms), max(ms), x_end


# the SIM instantiations as (nx, nu, N): the unrolled horizons, and the capacity-32 body of every sixteen-lane class at N = 13
CLASSES = [(12, 4, 10), (12, 4, 30), (12, 4, 20), (4, 1, 10), (8, 4, 9), (12, 4, 13), (4, 1, 13), (8, 4, 13), (12, 2, 13), (4, 2, 13), (4, 4, 13)]


def timed_class(T, dims, B, steps, reps, sequence):
    """ms per MPC step of mpc_run(steps, 1) on a seeded random system with one plant per instance (the model's own matrices): the SIM instantiation in
    one launch, or — sequence — the launch sequence over its one-solve kernel with the simulated plant kernel per step"""
    import os
    nx, nu, N = dims
    pr = T.problems
    prob = pr.random_system(nx, nu, N, seed=100 * nx + nu)
    rng = np.random.default_rng(64)
    table = 0.05 * rng.standard_normal((301, nx))
    start = (np.arange(B) % (301 - N)).astype(np.int32)
    x0 = table[start] + rng.uniform(-0.05, 0.05, size=(B, nx))
    os.environ.pop("TINYMPC_F64_LOOP", None)
    if sequence:
        os.environ["TINYMPC_F64_LOOP"] = "sequence"
    s = T.TinyBatchSolver64(prob, B)
    s.set_bounds(*pr.bounds_arrays(prob, np.float64))
    A, Bm = np.asarray(prob["Adyn"], np.float64), np.asarray(prob["Bdyn"], np.float64)
    s.set_plant(np.broadcast_to(A, (B, nx, nx)), np.broadcast_to(Bm, (B, nx, nu)))
    name = s.closed_loop_kernel_name()
    ms = []
    for _ in range(reps + 1):
        s.set_xref_window(table, start)
        s.set_x0(x0)
        s.first_columns()
        t0 = time.perf_counter()
        s.mpc_run(steps, 1)
        s.first_columns()
        ms.append((time.perf_counter() - t0) * 1e3 / steps)
    s.close()
    os.environ.pop("TINYMPC_F64_LOOP", None)
    ms = ms[1:]
    return name, float(np.median(ms)), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[65536, 16])
    ap.add_argument("--horizons", type=int, nargs="+", default=[10, 30])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=0, help="MPC steps per run (default: 8 at 65 536 instances and above 1024, 64 below)")
    ap.add_argument("--classes", action="store_true", help="every SIM instantiation on chip against the launch sequence over its one-solve kernel, at the first of --batches")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import accelerated_tinympc_amd as T
    rows = [("nominal", {}), ("shared plant", dict(plant="shared")), ("inst plants", dict(plant="inst")), ("inst plants + w + x_traj", dict(plant="inst", sim=True)),
            ("step by step (inst + w)", dict(plant="inst", stepwise=True))]
    # (None where the object files did not travel with the library)
    print(f"device_isa_sha: rows64<...,mpc> {T.build.kernel_isa_sha('rows64<12,4,10,mpc>')}, rows64<...,sim> {T.build.kernel_isa_sha('rows64<12,4,10,sim>')}", flush=True)
    if a.classes:
        B = a.batches[0]
        for dims in CLASSES:
            on, seq = timed_class(T, dims, B, a.steps or 8, a.reps, False), timed_class(T, dims, B, a.steps or 8, a.reps, True)
            print(f"B={B:6d} {str(dims):>12}: {on[0]:24s} {on[1]:8.4f} ms per MPC step ({on[2]:.4f} .. {on[3]:.4f}) | sequence {seq[0]:18s} {seq[1]:8.4f} ({seq[2]:.4f} .. {seq[3]:.4f})"
                  f" | on chip / sequence {on[1] / seq[1]:5.2f}", flush=True)
        return
    for N in a.horizons:
        for B in a.batches:
            steps = a.steps or (8 if B > 1024 else 64)
            base = None
            for label, kw in rows:
                name, med, lo, hi, x_end = timed(T, B, N, steps, a.reps, **kw)
                base = (med, x_end) if base is None else base
                same = bool(np.array_equal(x_end, base[1])) if not kw.get("stepwise") else None   # (the step-by-step run slides no window: another trajectory)
                print(f"N={N:2d} B={B:6d} steps={steps:2d} {label:>26}: {name:22s} {med * 1e3:9.1f} us per MPC step ({lo * 1e3:.1f} .. {hi * 1e3:.1f}), x {med / base[0]:5.2f} of nominal"
                      + ("" if same is None else f", final state {'equal to' if same else 'DIFFERS from'} the nominal run's"), flush=True)


if __name__ == "__main__":
    main()
