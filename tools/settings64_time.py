"""What per-instance settings cost on the fp64 library's sixteen-lane kernel (run on an MI355X): 65 536 quadrotor tracking instances in index order,
N = 10 and N = 30, device time by hipEvents.  Legs, each sample taken in a FRESH process and the legs alternated round by round:

  parent    another build of the library (--parent path/to/libtinympc_hip.so, the parent commit's): rows64<12,4,N>
  shared    this build, no per-instance settings: rows64<12,4,N>
  ps        this build, rows64<12,4,N,ps> with every instance given the batch's own settings
  ps-het    this build, rows64<12,4,N,ps> with the budgets 10 and 100 alternating by instance (two rows of every wave leave after 10 iterations and
            ride along until the other two are done: what a wave's lock step costs)

Two figures per sample: one cold solve (tiny_batch64_solve on a fresh workspace) and one MPC step of a 20-step run (tiny_batch64_mpc_run(20, 1),
one launch where the name ends ",mpc>" / ",mpc,ps>").  Each is preceded by the same call on a small handle of the same class, which loads the kernel.
Only C-ABI calls that every build has are used for the first two legs.  The table printed at the end has the median and min .. max over the rounds.

    python tools/settings64_time.py [--parent LIB] [--rounds R] [--batch B] [--horizons 10 30]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--horizons", type=int, nargs="*", default=[10, 30])
ap.add_argument("--leg", default=None, help="internal: one sample of one leg, as a child process")
ap.add_argument("--N", type=int, default=10)
args = ap.parse_args()
SETTINGS = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=100, check_termination=1, en_state_bound=1, en_input_bound=1)
LEGS = (["parent"] if args.parent else []) + ["shared", "ps", "ps-het"]


class Raw64:
    """a handle through the plain C-ABI of any build"""

    def __init__(self, lib, prob, batch, bnds, table, start, x0):
        self.lib, self.B = lib, batch
        D, I, P = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
        self.dp, self.ip = (lambda a: a.ctypes.data_as(D)), (lambda a: a.ctypes.data_as(I))
        lib.tiny_batch64_create.argtypes = [C.POINTER(P), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.tiny_batch64_set_cache.argtypes = [P, C.c_double, D, D, D, D]
        lib.tiny_batch64_set_dynamics.argtypes = [P, D, D, D]
        lib.tiny_batch64_set_settings.argtypes = [P, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.tiny_batch64_set_x0.argtypes = [P, D]
        lib.tiny_batch64_set_xref_window.argtypes = [P, D, C.c_int, I]
        for n in ("xmin", "xmax", "umin", "umax"):
            getattr(lib, "tiny_batch64_set_" + n).argtypes = [P, D, C.c_int]
        lib.tiny_batch64_solve.argtypes = [P]
        lib.tiny_batch64_mpc_run.argtypes = [P, C.c_int, C.c_int]
        lib.tiny_batch64_get_status.argtypes = [P, I, I, D]
        lib.tiny_batch64_destroy.argtypes, lib.tiny_batch64_destroy.restype = [P], None
        for n in ("tiny_batch64_kernel_name", "tiny_batch64_closed_loop_kernel_name"):
            getattr(lib, n).argtypes, getattr(lib, n).restype = [P], C.c_char_p
        self.h = P()
        cm = lambda m: np.ascontiguousarray(np.asarray(m, np.float64).T).ravel()
        ok = self.ok
        ok(lib.tiny_batch64_create(C.byref(self.h), prob["nx"], prob["nu"], prob["N"], batch, 0))
        k, p, qi, am = (cm(prob[n]) for n in ("Kinf", "Pinf", "Quu_inv", "AmBKt"))
        ok(lib.tiny_batch64_set_cache(self.h, float(prob["rho"]), self.dp(k), self.dp(p), self.dp(qi), self.dp(am)))
        a, b, q = cm(prob["Adyn"]), cm(prob["Bdyn"]), np.ascontiguousarray(np.asarray(prob["Q"], np.float64).ravel())
        ok(lib.tiny_batch64_set_dynamics(self.h, self.dp(a), self.dp(b), self.dp(q)))
        s = SETTINGS
        ok(lib.tiny_batch64_set_settings(self.h, s["abs_pri_tol"], s["abs_dua_tol"], s["max_iter"], s["check_termination"], s["en_state_bound"], s["en_input_bound"]))
        for n, arr in zip(("xmin", "xmax", "umin", "umax"), bnds):
            ok(getattr(lib, "tiny_batch64_set_" + n)(self.h, self.dp(np.ascontiguousarray(arr, np.float64)), 1))
        st = np.ascontiguousarray(start[:batch], np.int32)
        ok(lib.tiny_batch64_set_xref_window(self.h, self.dp(table), table.shape[0], self.ip(st)))
        ok(lib.tiny_batch64_set_x0(self.h, self.dp(np.ascontiguousarray(x0[:batch], np.float64))))

    @staticmethod
    def ok(rc):
        assert rc >= 0, f"rc={rc}"
        return rc

    def instance_settings(self, max_iter=None):
        """every instance the batch's own settings, or its own budget"""
        D, I, P = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
        self.lib.tiny_batch64_set_instance_settings.argtypes = [P, D, D, I, I, I, I]
        B, s = self.B, SETTINGS
        f = [np.full(B, s[k], np.float64) for k in ("abs_pri_tol", "abs_dua_tol")]
        i = [np.full(B, s[k], np.int32) for k in ("max_iter", "check_termination", "en_state_bound", "en_input_bound")]
        if max_iter is not None:
            i[0] = np.ascontiguousarray(max_iter, np.int32)
        self.ok(self.lib.tiny_batch64_set_instance_settings(self.h, *[self.dp(a) for a in f], *[self.ip(a) for a in i]))

    def mean_iter(self):
        it = np.zeros(self.B, np.int32)
        self.ok(self.lib.tiny_batch64_get_status(self.h, self.ip(it), None, None))
        return float(it.mean())

    def close(self):
        self.lib.tiny_batch64_destroy(self.h)


def child():
    import accelerated_tinympc_amd.problems as pr  # (importing the package loads no library: the parent leg never maps this build's)
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    ev = [C.c_void_p(), C.c_void_p()]

    def timed(fn):
        assert hip.hipEventRecord(ev[0], None) == 0
        fn()
        assert hip.hipEventRecord(ev[1], None) == 0 and hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        return ms.value

    leg, N, B, K = args.leg, args.N, args.batch, args.steps
    lib = C.CDLL(args.parent if leg == "parent" else str(ROOT / "accelerated-tinympc_amd" / "lib" / "libtinympc_hip.so"))
    prob = pr.quadrotor(20, N)
    x0, table, start = pr.tracking_batch(B, N)
    x0, table = np.asarray(x0, np.float64), np.ascontiguousarray(table, np.float64)
    bnds = pr.bounds_arrays(prob, np.float64)

    def make(batch):
        h = Raw64(lib, prob, batch, bnds, table, start, x0)
        if leg == "ps":
            h.instance_settings()
        elif leg == "ps-het":
            h.instance_settings(np.where(np.arange(batch) % 2 == 0, 10, 100))
        return h
    small = make(256)
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    out = dict(leg=leg, N=N, batch=B, kernel=lib.tiny_batch64_kernel_name(small.h).decode(), loop_kernel=lib.tiny_batch64_closed_loop_kernel_name(small.h).decode())
    small.ok(lib.tiny_batch64_solve(small.h))
    h = make(B)
    lib.tiny_batch64_forward_pass.argtypes = [C.c_void_p]
    h.ok(lib.tiny_batch64_forward_pass(h.h))  # gathers the window (its first-use allocation stays out of the timed call); the solve recomputes x, u
    out["cold_solve_ms"] = round(timed(lambda: h.ok(lib.tiny_batch64_solve(h.h))), 4)
    out["cold_mean_iter"] = round(h.mean_iter(), 2)
    h.close()
    small.ok(lib.tiny_batch64_mpc_run(small.h, K, 1))
    h = make(B)
    out["mpc_step_ms"] = round(timed(lambda: h.ok(lib.tiny_batch64_mpc_run(h.h, K, 1))) / K, 4)
    h.close(); small.close()
    print(json.dumps(out), flush=True)


def main():
    samples = {}
    for N in args.horizons:
        for rnd in range(args.rounds):
            for leg in LEGS:
                cmd = [sys.executable, __file__, "--leg", leg, "--N", str(N), "--batch", str(args.batch), "--steps", str(args.steps)] + (["--parent", args.parent] if args.parent else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
                if r.returncode != 0:   # a leg that fails ends the measurement: nothing more is started on the device
                    sys.exit(f"leg {leg} N={N} round {rnd} failed (rc={r.returncode}):\n{r.stderr[-2000:]}")
                s = json.loads(r.stdout.strip().splitlines()[-1])
                print(json.dumps(s), flush=True)
                samples.setdefault((N, leg), []).append(s)
    print("\n| N | leg | kernel | cold solve ms, median (min .. max) | mean iter | MPC step ms, median (min .. max) | loop kernel |")
    print("|---|---|---|---|---|---|---|")
    for (N, leg), ss in samples.items():
        cell = lambda k: "{:.3f} ({:.3f} .. {:.3f})".format(*(f([s[k] for s in ss]) for f in (np.median, min, max)))
        print(f"| {N} | {leg} | `{ss[0]['kernel']}` | {cell('cold_solve_ms')} | {ss[0]['cold_mean_iter']} | {cell('mpc_step_ms')} | `{ss[0]['loop_kernel']}` |")


if __name__ == "__main__":
    child() if args.leg else main()
