"""Cost of per-instance models in the fp64 library (run on an MI355X): 65 536 quadrotor tracking instances, N = 10 and N = 30, timed with hipEvents
around the calls.  Per horizon, a cold solve (tiny_batch64_solve from the all-zero workspace) and an on-chip MPC step (tiny_batch64_mpc_run(K, 1) / K) on

  shared        one model for the batch (tiny_batch64_set_cache / _set_dynamics)
  replicated    the SAME model for every instance through tiny_batch64_set_models: equal work, so the difference is the cost of the feature
  64 models     a model_family() batch with caches from tiny_batch64_set_systems: different models, different iteration counts

    python tools/models64_time.py [--batch B] [--steps K] [--repeats R] [--horizons 10 30] [--models M]

Every timed window follows a warm-up of the same shape from the same initial state; the median of the repeats is printed with min .. max, and the
device memory of the records.  One JSON line per horizon goes to stdout."""
import argparse
import ctypes as C
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import accelerated_tinympc_amd as T  # noqa: E402

pr = T.problems
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--horizons", type=int, nargs="*", default=[10, 30])
ap.add_argument("--models", type=int, default=64)
args = ap.parse_args()
B, K = args.batch, args.steps

hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]


def _ck(rc):
    assert rc == 0, f"HIP error {rc}"


ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    _ck(hip.hipEventCreate(C.byref(e)))


def timed(fn):
    """device time between two events on the null stream around fn (the library's fp64 calls run there and block)"""
    _ck(hip.hipEventRecord(ev[0], None))
    fn()
    _ck(hip.hipEventRecord(ev[1], None))
    _ck(hip.hipEventSynchronize(ev[1]))
    ms = C.c_float(0)
    _ck(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
    return ms.value


def spread(ms, per=1):
    a = np.array(ms) / per
    return dict(ms=round(float(np.median(a)), 4), min=round(float(a.min()), 4), max=round(float(a.max()), 4))


def measure(run, reset):
    """warm-up from the initial state, then `repeats` timed windows, each from the same initial state"""
    reset(); run()
    out = []
    for _ in range(args.repeats):
        reset()
        out.append(timed(run))
    return out


SETTINGS = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1)
KEYS = ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")
for N in args.horizons:
    prob = pr.quadrotor(20, N)
    x0, table, start = pr.tracking_batch(B, N)
    x0, table = np.asarray(x0, np.float64), np.asarray(table, np.float64)
    bnds = pr.bounds_arrays(prob, np.float64)
    rep = {k: np.broadcast_to(np.asarray(prob[k], np.float64), (B,) + np.asarray(prob[k]).shape) for k in KEYS}
    rep["Q"] = np.broadcast_to(np.asarray(prob["Q"], np.float64), (B, 12))
    rep["rho"] = np.full(B, prob["rho"])
    fam = pr.model_family("quadrotor", args.models, B, seed=21)
    rec = 3 * 144 + 2 * 48 + 16 + 12 + 1  # doubles per instance: the record and rho
    res = dict(config=f"quadrotor<12,4,{N}>", batch=B, steps=K, repeats=args.repeats, record_bytes_per_instance=8 * rec, records_MB=round(8 * rec * B / 1e6, 1))
    for tag in ("shared", "replicated", f"{args.models} models"):
        s = T.TinyBatchSolver64(prob, B, settings=SETTINGS)
        s.set_bounds(*bnds)
        if tag == "replicated":
            s.set_models(rep)
        elif tag != "shared":
            s.set_systems(fam["A"], fam["B"], fam["Q"], fam["R"], fam["rho"])
        zero = s.get_state()  # the freshly created workspace: all zero

        def reset():
            s.set_state(zero); s.set_xref_window(table, start); s.set_x0(x0)
        cold = measure(s.solve, reset)
        it_cold = float(s.get_status()[0].mean())
        loop = measure(lambda: s.mpc_run(K, 1), reset)
        res[tag] = dict(solve_kernel=s.kernel_name(), loop_kernel=s.closed_loop_kernel_name(), mean_iter_cold=round(it_cold, 2), cold_solve=spread(cold),
                        mpc_step=spread(loop, K), mean_iter_last_step=round(float(s.get_status()[0].mean()), 2))
        s.close()
    print(json.dumps(res), flush=True)
