"""Host cost of the closed-loop calls between two builds of the library: the settled hover loop, (12, 4, 10), where a solve is one iteration and the host's
share of an MPC step shows.  Rows: mpc_run_async and mpc_run_log (20 steps per call), on chip (16-lane kernel) and replayed (streaming row kernel), at 16 and
4 096 instances, and mpc_step_async in a loop; us of wall time per MPC step (calls back to back, one synchronize at the end), mean of the repeats.

    python tools/closed_loop_host_cost.py                               (one process, the library in the tree or the one TINYMPC_HIP_LIB names: JSON lines)
    python tools/closed_loop_host_cost.py --parent LIB [--pairs 4]      (alternating pairs, one library per process: the parent build LIB, then the tree's)

The bar of the second form: for every row the new build's mean over its processes lies inside the band (min .. max) of the parent's processes."""
import argparse, json, os, subprocess, sys, time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
STEPS = 20


def one(calls: int, warmup: int):
    import accelerated_tinympc_amd as T
    pr = T.problems
    prob = pr.quadrotor(50, 10)
    for batch in (16, 4096):
        x0, xref = pr.hover_batch(batch, 10)
        for loop, row in (("on chip", 1), ("replayed", 3)):
            sol = T.TinyBatchSolver(prob, batch)
            sol.set_bounds(*pr.bounds_arrays(prob))
            sol.set_xref(xref)
            sol.set_row_kernel(row)
            sol.set_x0(x0)
            ops = [("mpc_run_async", lambda: sol.mpc_run_async(STEPS), STEPS), ("mpc_run_log", lambda: sol.mpc_run_log(STEPS), STEPS)]
            if loop == "on chip":
                ops.append(("mpc_step_async", lambda: sol.mpc_step_async(0), 1))
            for name, fn, per in ops:
                n = calls * (STEPS if per == 1 else 1)
                for _ in range(warmup):
                    fn()
                sol.synchronize()
                c0, t0 = sol.lib.tiny_batch_debug_graph_captures(sol._h), time.perf_counter()
                for _ in range(n):
                    fn()
                sol.synchronize()
                us = (time.perf_counter() - t0) * 1e6 / (n * per)
                print(json.dumps({"row": f"{name} {loop} B={batch}", "kernel": sol.closed_loop_kernel_name() if per > 1 else sol.kernel_name(),
                                  "captures": sol.lib.tiny_batch_debug_graph_captures(sol._h) - c0, "us_per_step": round(us, 3)}), flush=True)
            sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libtinympc_hip.so of the parent commit")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    if not a.parent:
        return one(a.calls, a.warmup)
    rows = {}
    for pair in range(a.pairs):
        for which, lib in (("parent", a.parent), ("new", None)):
            env = {k: v for k, v in os.environ.items() if k != "TINYMPC_HIP_LIB"}
            if lib:
                env["TINYMPC_HIP_LIB"] = lib
            r = subprocess.run([sys.executable, "-W", "ignore", __file__, "--calls", str(a.calls), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            for line in r.stdout.splitlines():
                d = json.loads(line)
                assert d["captures"] == 0, d
                rows.setdefault((d["row"], d["kernel"]), {"parent": [], "new": []})[which].append(d["us_per_step"])
    print(f"# us per MPC step, {a.pairs} alternating pairs of processes (parent, new), {a.calls} calls of {STEPS} steps per figure; band = the parent's min .. max")
    outside = 0
    for (row, kernel), v in rows.items():
        p, n = v["parent"], v["new"]
        mean = sum(n) / len(n)
        inside = min(p) <= mean <= max(p)
        outside += not inside
        print(f"{row:34s} {kernel:26s} parent {' '.join(f'{x:8.3f}' for x in p)}   new {' '.join(f'{x:8.3f}' for x in n)}   new mean {mean:8.3f}  "
              f"{'inside' if inside else 'BELOW' if mean < min(p) else 'ABOVE'} {min(p):.3f} .. {max(p):.3f}")
    print(f"# {outside} rows outside the parent's band")


if __name__ == "__main__":
    main()
