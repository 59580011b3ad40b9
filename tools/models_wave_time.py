"""Per-instance models on the two wave kernels (tiny_batch_set_row_kernel 7 = waveres, 6 = wavestream) at equal and at unequal work, and against the
run-time-dimension kernel that serves the same batch without a forced family.

    python tools/models_wave_time.py [--quick]

Workloads: (32,16,50) at 2 048 and 16 384 instances, (16,8,10) at 2 048; x0[b] = s_b randn with s_b ~ U(0.02, 1), a shared reference of 0.05 randn,
u in +-0.5, x in +-2, default settings.  Per row: ms per cold solve (hipEvents around the solve kernel: median of 7 behind a warm-up, min ... max), its
mean iteration count, and ms per MPC step of a replayed 5-step run (wall time, median of 7 behind the capturing run and the first replay).  Rows:
  * shared                 — one model for the batch (tiny_batch_set_cache / set_dynamics);
  * shared as per-instance — the SAME model replicated through tiny_batch_set_models: equal work, so the difference is the cost of the feature;
  * 64 models              — a model_family("random") batch: different models, different iteration counts;
  * generic                — the 64-model batch on generic<...,pm>, where it runs without a forced family (2 048 instances only).
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

REPS = 7


def inputs(nx, nu, N, B, seed=1):
    rng = np.random.default_rng(seed)
    x0 = (rng.uniform(0.02, 1.0, size=(B, 1)) * rng.standard_normal((B, nx))).astype(np.float32)
    xref = (0.05 * rng.standard_normal((N, nx))).astype(np.float32)
    bnd = (np.full((N, nx), -2.0, np.float32), np.full((N, nx), 2.0, np.float32), np.full((N - 1, nu), -0.5, np.float32), np.full((N - 1, nu), 0.5, np.float32))
    return x0, xref, bnd


def run(T, prob, B, mods, family, variant=0, mpc=True):
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    x0, xref, bnd = inputs(nx, nu, N, B)
    s = T.TinyBatchSolver(prob, B)
    if mods is not None:
        s.set_models(mods)
    s.set_bounds(*bnd)
    s.set_xref(xref)
    s.set_row_kernel(family)  # first: under models the row variants exist through the forced wave family only
    s.select_kernel(variant)
    s.enable_timing(True)
    cold = []
    for _ in range(REPS + 1):
        s.reset_workspace()
        s.set_x0(x0)
        s.solve()
        cold.append(s.last_solve_ms())
    cold = cold[1:]
    iters = float(s.get_status()[0].mean())
    name = s.kernel_name()
    step = []
    if mpc:
        for _ in range(REPS + 2):  # the capturing run and the first replay (which uploads the graph) are the warm-up
            t0 = time.perf_counter()
            s.mpc_run_async(5, 0)
            s.synchronize()
            step.append((time.perf_counter() - t0) * 1e3 / 5)
        step = step[2:]
    s.close()
    return name, cold, iters, step


def row(label, r):
    name, cold, iters, step = r
    f = lambda v: f"{np.median(v):8.3f} ({min(v):.3f} ... {max(v):.3f})" if v else "       -"
    print(f"{label:>24}: {name:28s} cold solve {f(cold)} ms, mean iters {iters:5.1f}, MPC step {f(step)} ms", flush=True)
    return float(np.median(cold)), min(cold), max(cold)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2 048 instances only")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import accelerated_tinympc_amd as T
    pr = T.problems
    for nx, nu, N, B in ((32, 16, 50, 2048), (16, 8, 10, 2048), (32, 16, 50, 16384)):
        if a.quick and B > 2048:
            continue
        print(f"--- ({nx},{nu},{N}) x {B}")
        fam = pr.model_family("random", 64, B, seed=5, dims=(nx, nu))
        mods = pr.family_caches(fam)
        probs = [dict(p, N=N, u_min=-0.5, u_max=0.5, x_min=-2.0, x_max=2.0) for p in mods["probs"]]
        m0 = int(fam["model"][0])
        rep = {k: np.ascontiguousarray(np.broadcast_to(np.asarray(v)[:1], np.asarray(v).shape)) for k, v in mods.items() if k != "probs"}
        new = {}
        for family, what in ((7, "waveres"), (6, "wavestream")):
            row(f"{what} shared", run(T, probs[m0], B, None, family))
            row(f"{what} shared as pm", run(T, probs[m0], B, rep, family))
            new[what] = row(f"{what} 64 models", run(T, probs[m0], B, mods, family))
            if family == 7:
                row(f"{what} fma shared", run(T, probs[m0], B, None, family, 3))
                row(f"{what} fma shared as pm", run(T, probs[m0], B, rep, family, 3))
        if B <= 2048:
            g = row("generic 64 models", run(T, probs[m0], B, mods, 0, mpc=False))
            for what, w in new.items():
                print(f"{'':>24}  generic / {what}: {g[0] / w[0]:.1f}x (slowest {what} run {w[2]:.3f} ms, fastest generic run {g[1]:.3f} ms)", flush=True)


if __name__ == "__main__":
    main()
