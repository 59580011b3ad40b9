"""Wall time per MPC step of the step-by-step closed loop (tiny_batch_mpc_step_async: one solve launch and one plant-step launch per step) at a batch
so small that the host's cost per launch is most of the step: hovering quadrotors, (12, 4, 10).  One JSON line per repeat.
    python tools/step_loop_time.py [--batch 16] [--steps 2000] [--warmup 200] [--repeats 5]
TINYMPC_HIP_LIB names another build of the library to time instead (solver.load_library)."""
import argparse, json, sys, time
sys.path.insert(0, '.')
import accelerated_tinympc_amd as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
a = ap.parse_args()
pr = T.problems
prob = pr.quadrotor(50, 10)
x0, xref = pr.hover_batch(a.batch, 10)
sol = T.TinyBatchSolver(prob, a.batch)
sol.set_bounds(*pr.bounds_arrays(prob))
sol.set_xref(xref)
for rep in range(a.repeats):
    sol.reset_workspace(); sol.set_x0(x0)
    for _ in range(a.warmup): sol.mpc_step_async(0)
    sol.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps): sol.mpc_step_async(0)
    sol.synchronize()
    us = (time.perf_counter() - t0) * 1e6 / a.steps
    print(json.dumps({"tool": "step_loop_time", "batch": a.batch, "class": [12, 4, 10], "kernel": sol.kernel_name(), "steps": a.steps, "warmup": a.warmup,
                      "repeat": rep, "us_per_step": round(us, 3)}), flush=True)
sol.close()
