"""ms per MPC step of the fp64 library's closed loop (run on an MI355X): 65 536 quadrotor tracking instances, window advance 1, N = 10 and N = 30,
timed with hipEvents around the calls.  Three paths per horizon:

  on chip    tiny_batch64_mpc_run(K, 1): all solves in one launch (closed_loop_kernel_name() ends in ",mpc>")
  sequence   the same call after select_kernel(1): gather, dual reset, thread-per-instance solve and plant kernel enqueued per step
  mpc_step   K calls of tiny_batch64_mpc_step with one shared reference: the only closed loop the library had before the run existed

    python tools/closed_loop64_time.py [--batch B] [--steps K] [--repeats R] [--horizons 10 30] [--dims nx,nu,N ...] [--lib other/libtinympc_hip.so]

--lib times the mpc_step loop on another build of the library as well (raw C-ABI calls: an older build need not have the new symbols), alternating
with this build's in the same process.  --dims adds seeded random systems of other classes: there the on-chip run is also timed against the launch
sequence over the same sixteen-lane solve kernel (TINYMPC_F64_LOOP=sequence), the comparison that decides whether a class keeps its on-chip
instantiation.  Every timed window follows a warm-up of the same shape from the same initial state; the median of the repeats is printed with
their spread.  One JSON line per configuration goes to stdout."""
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
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--horizons", type=int, nargs="*", default=[10, 30])
ap.add_argument("--dims", nargs="*", default=[])
ap.add_argument("--lib", default=None)
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


class Raw64:
    """tiny_batch64_mpc_step on any build of the library: only the C-ABI calls every build has"""

    def __init__(self, path, prob, batch, settings, bnds, xref_shared):
        lib = self.lib = C.CDLL(str(path))
        D, P = C.POINTER(C.c_double), C.c_void_p
        lib.tiny_batch64_create.argtypes = [C.POINTER(P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.tiny_batch64_set_cache.argtypes = [P, C.c_double, D, D, D, D]
        lib.tiny_batch64_set_dynamics.argtypes = [P, D, D, D]
        lib.tiny_batch64_set_settings.argtypes = [P, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.tiny_batch64_set_x0.argtypes = [P, D]
        for n in ("xref", "xmin", "xmax", "umin", "umax"):
            getattr(lib, "tiny_batch64_set_" + n).argtypes = [P, D, C.c_int]
        lib.tiny_batch64_mpc_step.argtypes = [P]
        lib.tiny_batch64_destroy.argtypes, lib.tiny_batch64_destroy.restype = [P], None
        self.h = P()
        dp = lambda a: a.ctypes.data_as(D)
        cm = lambda m: np.ascontiguousarray(np.asarray(m, np.float64).T).ravel()
        self._ok(lib.tiny_batch64_create(C.byref(self.h), prob["nx"], prob["nu"], prob["N"], batch, 0))
        k, p, qi, am = (cm(prob[n]) for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"))
        self._ok(lib.tiny_batch64_set_cache(self.h, float(prob["rho"]), dp(k), dp(p), dp(qi), dp(am)))
        a, b, q = cm(prob["Adyn"]), cm(prob["Bdyn"]), np.ascontiguousarray(np.asarray(prob["Q"], np.float64).ravel())
        self._ok(lib.tiny_batch64_set_dynamics(self.h, dp(a), dp(b), dp(q)))
        s = settings
        self._ok(lib.tiny_batch64_set_settings(self.h, s["abs_pri_tol"], s["abs_dua_tol"], s["max_iter"], s["check_termination"], s["en_state_bound"],
                                               s["en_input_bound"]))
        for n, arr in zip(("xmin", "xmax", "umin", "umax", "xref"), (*bnds, xref_shared)):
            arr = np.ascontiguousarray(arr, np.float64)
            self._ok(getattr(lib, "tiny_batch64_set_" + n)(self.h, dp(arr), 1))
        self.dp = dp

    @staticmethod
    def _ok(rc):
        assert rc >= 0, f"rc={rc}"

    def set_x0(self, x0):
        self._ok(self.lib.tiny_batch64_set_x0(self.h, self.dp(np.ascontiguousarray(x0, np.float64))))

    def mpc_steps(self, k):
        for _ in range(k):
            self._ok(self.lib.tiny_batch64_mpc_step(self.h))

    def close(self):
        self.lib.tiny_batch64_destroy(self.h)


def spread(ms):
    per = np.array(ms) / K
    return dict(ms_per_step=round(float(np.median(per)), 4), min=round(float(per.min()), 4), max=round(float(per.max()), 4))


def measure(run, reset):
    """warm-up from the initial state, then `repeats` timed windows, each from the same initial state"""
    reset(); run()
    out = []
    for _ in range(args.repeats):
        reset()
        out.append(timed(run))
    return out


SETTINGS = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1)
configs = [("quadrotor", (12, 4, N)) for N in args.horizons] + [("random", tuple(int(v) for v in d.split(","))) for d in args.dims]
for kind, (nx, nu, N) in configs:
    if kind == "quadrotor":
        prob = pr.quadrotor(20, N)
        x0, table, start = pr.tracking_batch(B, N)
    else:
        prob = pr.random_system(nx, nu, N, seed=100 * nx + nu)
        rng = np.random.default_rng(64)
        table = 0.05 * rng.standard_normal((301, nx))
        start = (np.arange(B) % (301 - N)).astype(np.int32)
        x0 = table[start] + rng.uniform(-0.05, 0.05, size=(B, nx))
    x0, table = np.asarray(x0, np.float64), np.asarray(table, np.float64)
    bnds = pr.bounds_arrays(prob, np.float64)
    res = dict(config=f"{kind}<{nx},{nu},{N}>", batch=B, steps=K, repeats=args.repeats)

    def run_path(kernel, force_sequence=False):
        os.environ.pop("TINYMPC_F64_LOOP", None)
        if force_sequence:
            os.environ["TINYMPC_F64_LOOP"] = "sequence"
        s = T.TinyBatchSolver64(prob, B, settings=SETTINGS)
        s.select_kernel(kernel)
        s.set_bounds(*bnds)
        name = s.closed_loop_kernel_name()

        def reset():
            s.set_state(zero); s.set_xref_window(table, start); s.set_x0(x0)
        zero = s.get_state()  # the freshly created workspace: all zero
        ms = measure(lambda: s.mpc_run(K, 1), reset)
        it = float(s.get_status()[0].mean())
        s.close()
        os.environ.pop("TINYMPC_F64_LOOP", None)
        return dict(kernel=name, mean_iter_last_step=round(it, 2), **spread(ms))

    res["run"] = run_path(0)
    if res["run"]["kernel"].endswith(",mpc>"):
        res["sequence_same_kernel"] = run_path(0, force_sequence=True)
    res["sequence_thread64"] = run_path(1)

    libs = [("this", T.build.LIB)] + ([("other", args.lib)] if args.lib else [])
    raws = {tag: Raw64(path, prob, B, SETTINGS, bnds, table[:N]) for tag, path in libs}
    loops = {tag: [] for tag in raws}
    for tag, r in raws.items():  # warm-up
        r.set_x0(x0); r.mpc_steps(K)
    for _ in range(args.repeats):  # alternating
        for tag, r in raws.items():
            r.set_x0(x0)
            loops[tag].append(timed(lambda: r.mpc_steps(K)))
    for tag, r in raws.items():
        res[f"mpc_step_loop_{tag}"] = spread(loops[tag])
        r.close()
    print(json.dumps(res), flush=True)
