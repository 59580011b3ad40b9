"""Per-instance models at equal and at unequal work, the shared kernels' on-chip closed loop, and the batched GPU Riccati.

    python tools/models_time.py [--batch 65536] [--host-sample 256]
    python tools/models_time.py --shared-only --root DIR     # the shared-model rows only, with the package found under DIR (e.g. another checkout)

Rows (65 536 quadrotor tracking instances, N = 30 unless stated, exact 16-lane kernel forced): ms per cold solve (kernel, median of 5) and per warm
on-chip MPC step (wall, second of two 20-step runs), with the mean iteration count of the cold solve:
  * shared                 — one model for the batch (tiny_batch_set_cache / set_dynamics);
  * shared as per-instance — the SAME model replicated through tiny_batch_set_models: equal work, so the difference is the cost of the feature;
  * 64 / B models          — a model_family() batch with caches from tiny_batch_set_systems: different models, different iteration counts.
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np


def run(T, prob, B, N, mods, exact=True, reps=5):
    pr = T.problems
    x0, table, start = pr.tracking_batch(B, N, seed=1)
    s = T.TinyBatchSolver(prob, B)
    s.set_bounds(*pr.bounds_arrays(prob))
    s.set_xref_window(table, start)
    s.select_kernel(2 if exact else 3)
    s.set_row_kernel(1)
    if mods is not None:
        s.set_models(mods)
    s.enable_timing(True)
    cold = []
    for _ in range(reps):
        s.reset_workspace()
        s.set_x0(x0)
        s.solve()
        cold.append(s.last_solve_ms())
    iters = float(s.get_status()[0].mean())
    s.mpc_run_async(20, 1)
    s.synchronize()
    t0 = time.perf_counter()
    s.mpc_run_async(20, 1)
    s.synchronize()
    warm = (time.perf_counter() - t0) * 1e3 / 20
    name = s.closed_loop_kernel_name()
    s.close()
    return name, float(np.median(cold)), warm, iters


def row(label, r):
    name, cold, warm, iters = r
    print(f"{label:>26}: {name:30s} cold solve {cold:6.3f} ms (mean iters {iters:5.1f}), warm on-chip MPC step {warm:6.3f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--host-sample", type=int, default=256)
    ap.add_argument("--shared-only", action="store_true")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import accelerated_tinympc_amd as T
    pr = T.problems
    B = a.batch
    for N in (10, 30, 50):
        row(f"shared N={N}", run(T, pr.quadrotor(20, N), B, N, None))
    row("shared N=30 fma", run(T, pr.quadrotor(20, 30), B, 30, None, exact=False))
    if a.shared_only:
        return
    N = 30
    prob = pr.quadrotor(20, N)
    rep = {k: np.broadcast_to(np.asarray(prob[k]), (B,) + np.asarray(prob[k]).shape) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")}
    rep["Q"] = np.broadcast_to(np.asarray(prob["Q"]), (B, 12))
    rep["rho"] = np.full(B, prob["rho"])
    row("shared as per-instance", run(T, prob, B, N, rep))
    row("shared as per-inst. fma", run(T, prob, B, N, rep, exact=False))
    for nm in (64, B):
        fam = pr.model_family("quadrotor", nm, B, seed=5)
        A, Bm, Q, R, rho = (fam[k] for k in ("A", "B", "Q", "R", "rho"))
        r = T.riccati_batch(12, 4, A, Bm, Q, R, rho)
        mods = {k: r[k] for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt")}
        mods.update(Adyn=A, Bdyn=Bm, Q=Q + rho[:, None], rho=rho)
        row(f"{nm} models", run(T, prob, B, N, mods))
    fam = pr.model_family("quadrotor", B, B, seed=6)
    A, Bm, Q, R, rho = (fam[k] for k in ("A", "B", "Q", "R", "rho"))
    T.riccati_batch(12, 4, A[:64], Bm[:64], Q[:64], R[:64], rho[:64])  # warm-up
    t0 = time.perf_counter()
    res = T.riccati_batch(12, 4, A, Bm, Q, R, rho)
    gpu = time.perf_counter() - t0
    n = a.host_sample
    t0 = time.perf_counter()
    for i in range(n):
        T.riccati(12, 4, A[i], Bm[i], Q[i], R[i], rho[i])
    host = (time.perf_counter() - t0) / n * B
    print(f"riccati {B} quadrotor-family systems: GPU {gpu * 1e3:.1f} ms incl. transfers (mean iters {res['iters'].mean():.0f}); "
          f"host tiny_riccati {host * 1e3:.0f} ms scaled from {n} systems on one core ({os.cpu_count()} cores visible)")


if __name__ == "__main__":
    main()
