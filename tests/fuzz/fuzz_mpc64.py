"""Randomised check (run on an MI355X) of the fp64 library's closed-loop run: tiny_batch64_mpc_run_traj(K) — the on-chip loop or the launch sequence —
must leave exactly the state of K calls of tiny_batch64_mpc_run(1), and both that of the fp64 oracle's closed loop, for random classes, kernels,
horizons, batches, settings, reference modes, window advances and step counts.  Stops at the first HIP error (a TinyBatchError ends the run).
    python tests/fuzz/fuzz_mpc64.py [--seconds S] [--seed N]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import accelerated_tinympc_amd as T  # noqa: E402
from helpers import SCALAR_ORDER, STATE_ORDER, oracle_closed_loop, same_bits  # noqa: E402
from oracle import oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=120.0)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
pr = T.problems
rng = np.random.default_rng(args.seed)
DIMS = [(12, 4), (4, 1), (8, 4), (12, 2), (4, 2), (4, 4), (16, 4)]  # TINY_FOR_EACH_F64DIMS
UNROLLED = [(12, 4, 10), (12, 4, 30), (12, 4, 20), (4, 1, 10), (8, 4, 9)]  # TINY_FOR_EACH_F64ROWS
probs = {}
t_end, rounds, onchip = time.time() + args.seconds, 0, 0
while time.time() < t_end:
    if rng.random() < 0.4:
        nx, nu, N = UNROLLED[rng.integers(len(UNROLLED))]
    else:
        nx, nu = DIMS[rng.integers(len(DIMS))]
        N = int(rng.choice([3, 4, 7, 13, 31, 32, 33, 48, 64]))
    if (nx, nu, N) not in probs:
        probs[(nx, nu, N)] = pr.random_system(nx, nu, N, seed=100 * nx + nu, riccati=O.riccati)
    prob = probs[(nx, nu, N)]
    B = int(rng.choice([1, 3, 4, 5, 63, 64, 65, 130, 200]))
    settings = dict(abs_pri_tol=float(rng.choice([1e-3, 1e-2])), abs_dua_tol=float(rng.choice([1e-3, 1e-1])), max_iter=int(rng.choice([0, 1, 3, 20])),
                    check_termination=int(rng.choice([1, 1, 2, 5])), en_state_bound=int(rng.integers(2)), en_input_bound=int(rng.integers(2)))
    kernel = int(rng.choice([0, 0, 1, 2]))
    K, adv = int(rng.integers(1, 7)), int(rng.choice([0, 1, 2]))
    mode = str(rng.choice(["window", "window", "shared", "inst"]))
    rows = N + int(rng.integers(0, 12))
    table = 0.05 * rng.standard_normal((rows, nx))
    start = rng.integers(0, rows - N + 1, size=B).astype(np.int32)
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx))
    bnds = tuple(np.full(shape, v) for shape, v in (((N, nx), prob["x_min"]), ((N, nx), prob["x_max"]), ((N - 1, nu), 0.2 * prob["u_min"]),
                                                     ((N - 1, nu), 0.2 * prob["u_max"])))
    ref = (table, start) if mode == "window" else (table[:N].copy() if mode == "shared" else table[np.minimum(start[:, None] + np.arange(N), rows - 1)])
    sols = []
    for _ in range(2):
        s = T.TinyBatchSolver64(prob, B, settings=settings)
        try:
            s.select_kernel(kernel)
        except T.TinyBatchError:
            s.select_kernel(0)
        s.set_bounds(*bnds)
        if mode == "window":
            s.set_xref_window(table, start)
        else:
            s.set_xref(ref)
        s.set_x0(x0)
        sols.append(s)
    a, b = sols
    what = f"round {rounds} {a.closed_loop_kernel_name()} N={N} B={B} K={K} adv={adv} {mode} settings {settings}"
    onchip += a.closed_loop_kernel_name().endswith(",mpc>")
    traj = a.mpc_run_traj(K, adv)
    steps = []
    for _ in range(K):
        b.mpc_run(1, adv)
        steps.append(b.first_columns()[1])
    want = oracle_closed_loop(O, prob, np.float64, settings, x0, ref, bnds, K, adv if mode == "window" else 0)
    sa, sb = a.get_state(), b.get_state()
    bad = [n for n in STATE_ORDER + SCALAR_ORDER if not (same_bits(sa[n], sb[n]) and same_bits(sa[n], want["st"][n]))]
    if settings["max_iter"] > 0:  # (with no iteration u.col(0) is the workspace's stale column: only the two device paths are compared)
        bad += ["u0 (oracle)"] * (not same_bits(traj, want["u0"]))
    bad += ["u0 (steps)"] * (not same_bits(traj, np.array(steps))) + ["x.col(0)"] * (not same_bits(a.first_columns()[0], b.first_columns()[0]))
    if mode == "window":
        bad += ["window starts"] * (not (np.array_equal(a.xref_start(), start + K * adv) and np.array_equal(b.xref_start(), start + K * adv)))
    if bad:
        print(f"MISMATCH {what}: {bad}")
        sys.exit(1)
    a.close(); b.close(); rounds += 1
print(f"fuzz ok: {rounds} rounds ({onchip} through the on-chip closed loop), mpc_run_traj(K) == K x mpc_run(1) == the fp64 oracle's loop, bit for bit")
