"""Per-instance settings on the state-on-chip wave kernel (tiny_batch_set_row_kernel 7) against ANOTHER checkout's shared kernel, the two builds
interleaved on the same box.

    python tools/settings_wave_time.py --parent /path/to/built/parent/checkout [--rounds 5] [--family 7]

Workload: 2 048 instances of (32,16,50) as in tools/models_wave_time.py (x0[b] = s_b randn with s_b ~ U(0.02, 1), a shared reference of 0.05 randn,
u in +-0.5, x in +-2, default settings: tolerances 1e-3, max_iter 100).  Every figure is taken in a child process of its own, one build after the other,
`rounds` times over; a child times 5 launches behind a warm-up (hipEvents around the solve kernel; an MPC step is the wall time of a replayed 5-step run / 5)
and the figure is the median over all its launches of all rounds, min ... max beside it:
  (a) cold solve:   parent waveres<...,exact>   |  this tree's waveres<...,exact,ps> with every instance given the batch's own settings
  (b) MPC step:     the same two handles
  (c) budgets:      half the instances max_iter 10, half 100 — parent: the batch split by budget into two launches of 1 024 (the sum of the two kernel
                    times) | this tree: one launch under per-instance settings
The parent's own run-to-run spread is what a difference has to be read against.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

DIMS, B, REPS = (32, 16, 50), 2048, 5


def inputs(nx, nu, N, B, seed=1):
    rng = np.random.default_rng(seed)
    x0 = (rng.uniform(0.02, 1.0, size=(B, 1)) * rng.standard_normal((B, nx))).astype(np.float32)
    xref = (0.05 * rng.standard_normal((N, nx))).astype(np.float32)
    bnd = (np.full((N, nx), -2.0, np.float32), np.full((N, nx), 2.0, np.float32), np.full((N - 1, nu), -0.5, np.float32), np.full((N - 1, nu), 0.5, np.float32))
    return x0, xref, bnd


def child(root, mode, family):
    """one build, one mode: 'shared' | 'uniform' (cold solve and MPC step), 'split' | 'mixed' (the two budgets); prints one JSON line"""
    sys.path.insert(0, root)
    import accelerated_tinympc_amd as T
    pr = T.problems
    nx, nu, N = DIMS
    fam = pr.model_family("random", 64, B, seed=5, dims=(nx, nu))
    prob = dict(pr.family_caches(fam)["probs"][int(fam["model"][0])], N=N, u_min=-0.5, u_max=0.5, x_min=-2.0, x_max=2.0)
    x0, xref, bnd = inputs(nx, nu, N, B)
    budget = np.where(np.arange(B) < B // 2, 10, 100).astype(np.int32)

    def handle(idx, settings=None):
        s = T.TinyBatchSolver(prob, len(idx), settings=settings)
        s.set_bounds(*bnd); s.set_xref(xref)
        s.set_row_kernel(family)
        s.enable_timing(True)
        return s
    everyone = np.arange(B)
    if mode == "split":
        hs = [(idx, handle(idx, dict(max_iter=int(m)))) for m in (10, 100) for idx in [np.nonzero(budget == m)[0]]]
    else:
        hs = [(everyone, handle(everyone))]
        if mode == "uniform":
            hs[0][1].set_instance_settings(abs_pri_tol=np.full(B, 1e-3, np.float32), abs_dua_tol=np.full(B, 1e-3, np.float32), max_iter=np.full(B, 100, np.int32),
                                           check_termination=np.ones(B, np.int32))
        elif mode == "mixed":
            hs[0][1].set_instance_settings(max_iter=budget)
    cold = []
    for _ in range(REPS + 1):
        ms = 0.0
        for idx, s in hs:
            s.reset_workspace(); s.set_x0(x0[idx])
            s.solve()
            ms += s.last_solve_ms()
        cold.append(ms)
    iters = float(np.concatenate([s.get_status()[0] for _, s in hs]).mean())
    step = []
    if mode in ("shared", "uniform"):
        s = hs[0][1]
        for _ in range(REPS + 2):  # the capturing run and the first replay (which uploads the graph) are the warm-up
            t0 = time.perf_counter()
            s.mpc_run_async(5, 0)
            s.synchronize()
            step.append((time.perf_counter() - t0) * 1e3 / 5)
    print(json.dumps(dict(name=" + ".join(s.kernel_name() for _, s in hs), cold=cold[1:], iters=iters, step=step[2:])), flush=True)
    for _, s in hs:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--family", type=int, default=7)
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.root, a.child, a.family)
    assert a.parent, "--parent: the comparison is against another checkout's build, never against this tree's own shared kernel"
    runs = [("parent shared", a.parent, "shared"), ("ps, the batch's settings", a.root, "uniform"), ("parent split 10 | 100", a.parent, "split"), ("ps 10 | 100", a.root, "mixed")]
    got = {label: dict(cold=[], step=[]) for label, _, _ in runs}
    for _ in range(a.rounds):   # the builds alternate: parent, this tree, parent, this tree
        for label, root, mode in runs:
            out = subprocess.run([sys.executable, __file__, "--root", root, "--child", mode, "--family", str(a.family)], capture_output=True, text=True, timeout=300)
            if out.returncode != 0:   # nothing more is started on the device after a failed child
                sys.exit(f"{label}: the child ended with {out.returncode}\n{out.stderr[-2000:]}")
            r = json.loads(out.stdout.strip().splitlines()[-1])
            got[label]["cold"] += r["cold"]; got[label]["step"] += r["step"]
            got[label].update(name=r["name"], iters=r["iters"])
    f = lambda v: f"{np.median(v):8.3f} ({min(v):.3f} ... {max(v):.3f})" if v else "       -"
    print(f"({DIMS[0]},{DIMS[1]},{DIMS[2]}) x {B}, {a.rounds} rounds x {REPS} launches, ms")
    for label, _, _ in runs:
        g = got[label]
        print(f"{label:>26}: {g['name']:52s} cold solve {f(g['cold'])}, mean iters {g['iters']:5.1f}, MPC step {f(g['step'])}", flush=True)
    med = lambda label, k: float(np.median(got[label][k]))
    p, n = "parent shared", "ps, the batch's settings"
    print(f"(a) cold solve: {100 * (med(n, 'cold') / med(p, 'cold') - 1):+.2f} %; parent's spread {100 * (max(got[p]['cold']) - min(got[p]['cold'])) / med(p, 'cold'):.2f} % of its median")
    print(f"(b) MPC step:   {100 * (med(n, 'step') / med(p, 'step') - 1):+.2f} %; parent's spread {100 * (max(got[p]['step']) - min(got[p]['step'])) / med(p, 'step'):.2f} % of its median")
    print(f"(c) budgets 10 | 100: one launch {med('ps 10 | 100', 'cold'):.3f} against two launches {med('parent split 10 | 100', 'cold'):.3f}: "
          f"{med('parent split 10 | 100', 'cold') / med('ps 10 | 100', 'cold'):.2f}x")


if __name__ == "__main__":
    main()
