#!/usr/bin/env python3
"""Where the live-out of the headline kernel goes: per wave and tile phase stamps of admm_tile16_kernel<30, true, true>.

    python tools/t16_epilogue_stamps.py build [name="-DFLAG=..."] ...   (CPU container or GPU box; default: stamp="")
    python tools/t16_epilogue_stamps.py run NAME [--out DIR]            (GPU box: the headline workload on lib/ab/libtinympc_hip_NAME.so)
    python tools/t16_epilogue_stamps.py sweep [--out DIR]               (GPU box: kernel time against a fixed iteration count, tol 0)

`build` compiles admm_tile16.hip with -DTINY_T16_STAMP=1 (plus the extra flags of the variant, e.g. -DTINY_T16_LINES=0 for the row-wise
live-out) into a separate library under accelerated-tinympc_amd/lib/ab/ (git-ignored).  That build records, per wave slot and tile, the
s_memrealtime clock (100 MHz) when the tile is claimed, when its iteration loop is left and when its live-out stores have been issued.  The
next claim of the wave returns only after those stores have drained (stores and the claim's atomic share the wave's in-order vmcnt), so

    epilogue = next claim - loop left  = store issue (+ x,u regeneration) + drain.

`run` prints the distribution of that length per round (the k-th tile a wave takes), how many waves are in an epilogue at the same time, and
the share of the waves' busy time spent in epilogues.  `sweep` fits kernel time = intercept + slope x max_iter on the product library (or
TINYMPC_HIP_LIB), the fixed cost per launch that the epilogue is part of."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "accelerated-tinympc_amd"
sys.path.insert(0, str(ROOT))
CLOCK_HZ = 100e6  # s_memrealtime


def build(variants):
    import importlib.util
    spec = importlib.util.spec_from_file_location("b", PKG / "build.py"); b = importlib.util.module_from_spec(spec); spec.loader.exec_module(b)
    b.build()
    ab = PKG / "lib" / "ab"; ab.mkdir(exist_ok=True)
    src = "admm_tile16.hip"
    procs = []
    for name, flags in variants.items():
        obj = ab / f"admm_tile16_{name}.o"
        cmd = ["/opt/rocm/bin/hipcc", *b.FLAGS, *b.EXTRA_FLAGS[src], "-DTINY_T16_STAMP=1", *flags.split(), "-c", str(PKG / "csrc" / src), "-o", str(obj)]
        procs.append((name, obj, subprocess.Popen(cmd)))
    for name, obj, p in procs:
        assert p.wait() == 0, name
        objs = [str(obj) if o.name == "admm_tile16.o" else str(o) for _, o in b._objs()]
        so = ab / f"libtinympc_hip_{name}.so"
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(so), *objs], check=True)
        print("built", so)


def headline_solver(T, B=65536):
    pr = T.problems
    prob = pr.quadrotor(20, 30)
    x0, table, start = pr.tracking_batch(B, 30)
    sol = T.TinyBatchSolver(prob, B)
    sol.set_row_kernel(5)  # tile16 (what bench.py's automatic choice runs on a GPU of its size)
    sol.set_bounds(*pr.bounds_arrays(prob)); sol.set_xref_window(table, start)
    return sol, x0


def analyse(st, iters, kernel_ms):
    """st: [slots][tiles][4] u64 (claim, loop left, stores issued, tile or ~0)."""
    t0 = st[:, :, 0].astype(np.float64); t1 = st[:, :, 1].astype(np.float64); t2 = st[:, :, 2].astype(np.float64); tile = st[:, :, 3]
    used = t0 != 0
    base = t0[used].min()
    us = lambda t: (t - base) / CLOCK_HZ * 1e6
    recs = []  # (slot, round, tile, claim, loop_end, issued, next_claim)
    for w in range(st.shape[0]):
        ks = np.nonzero(used[w])[0]
        for k in ks:
            if tile[w, k] == np.uint64(~np.uint64(0)) or k + 1 not in ks:
                continue  # the failed claim ends the wave (its time is the next_claim of the tile before)
            recs.append((w, k, int(tile[w, k]), us(t0[w, k]), us(t1[w, k]), us(t2[w, k]), us(t0[w, k + 1])))
    r = np.array(recs)
    if r.size == 0:
        return {"error": "no stamps recorded"}
    rnd, claim, lend, issued, nxt = r[:, 1].astype(int), r[:, 3], r[:, 4], r[:, 5], r[:, 6]
    epi, issue, drain, loop = nxt - lend, issued - lend, nxt - issued, lend - claim
    ends = np.array([us(t0[w, np.nonzero(used[w])[0].max()]) for w in range(st.shape[0]) if used[w].any()])
    span = ends.max()
    busy = ends.sum()  # every wave is busy from the launch's first claim to its failed claim
    q = lambda a: {"p10": round(float(np.percentile(a, 10)), 2), "median": round(float(np.median(a)), 2), "p90": round(float(np.percentile(a, 90)), 2),
                   "max": round(float(a.max()), 2)}
    per_round = {}
    for k in sorted(set(rnd)):
        m = rnd == k
        per_round[str(k)] = {"tiles": int(m.sum()), "epilogue_us": q(epi[m]), "issue_us": q(issue[m]), "drain_us": q(drain[m]),
                             "loop_us": q(loop[m]), "loop_end_spread_us": round(float(lend[m].max() - lend[m].min()), 1)}
    # overlap: waves inside an epilogue at each moment (event sweep over [loop_end, next_claim) intervals)
    ev = np.concatenate([np.stack([lend, np.ones_like(lend)], 1), np.stack([nxt, -np.ones_like(nxt)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    cnt = np.cumsum(ev[:, 1]); dt = np.diff(ev[:, 0], append=ev[-1, 0])
    nslots = int(used.any(axis=1).sum())
    hist = {}
    for lo, hi in ((0, 0.05), (0.05, 0.25), (0.25, 0.5), (0.5, 1.01)):
        m = (cnt / nslots >= lo) & (cnt / nslots < hi) & (cnt > 0)
        hist[f"{int(lo * 100)}-{int(min(hi, 1) * 100)}%"] = round(float(dt[m].sum() / span), 4)
    # the tile's iterations (its slowest column) against its loop time: one iteration's cost, for the epilogue in iterations
    it_tile = iters.reshape(-1, 16).max(axis=1)[r[:, 2].astype(int)]
    slope = float(np.polyfit(it_tile, loop, 1)[0])
    return {"kernel_ms_event": kernel_ms, "stamp_span_ms": round(span / 1e3, 4), "wave_slots": nslots, "tiles": len(recs),
            "epilogue_share_of_busy_time": round(float(epi.sum() / busy), 4), "issue_share": round(float(issue.sum() / busy), 4),
            "drain_share": round(float(drain.sum() / busy), 4), "epilogue_us": q(epi), "issue_us": q(issue), "drain_us": q(drain),
            "us_per_iteration": round(slope, 3), "epilogue_in_iterations": round(float(np.median(epi)) / slope, 2),
            "max_waves_in_epilogue": int(cnt.max()), "share_of_span_by_fraction_of_waves_in_epilogue": hist, "per_round": per_round}


def run(name, out):
    so = PKG / "lib" / "ab" / f"libtinympc_hip_{name}.so"
    os.environ["TINYMPC_HIP_LIB"] = str(so)
    import warnings; warnings.simplefilter("ignore")
    import accelerated_tinympc_amd as T
    lib = T.load_library()
    assert hasattr(lib, "tiny_t16_stamp_begin"), f"{so} is not a stamp build"
    sol, x0 = headline_solver(T)
    sol.set_dispatch(-1)
    sol.enable_timing(True)
    tiles = lib.tiny_t16_stamp_tiles()
    ms = []
    for r in range(6):
        assert lib.tiny_t16_stamp_begin() == 0  # one record set per wave slot of the device (four per CU)
        sol.reset_workspace(); sol.set_x0(x0); sol.solve_async(); sol.synchronize()
        ms.append(sol.last_solve_ms())
    nslots = lib.tiny_t16_stamp_slots()
    st = np.zeros((nslots, tiles, 4), dtype=np.uint64)
    assert lib.tiny_t16_stamp_read(st.ctypes.data_as(C.POINTER(C.c_ulonglong)), nslots) == 0
    iters = sol.get_status()[0]
    res = {"variant": name, "kernel": sol.kernel_name(), "kernel_ms_runs": [round(m, 4) for m in ms], **analyse(st, np.asarray(iters), ms[-1])}
    sol.close()
    print(json.dumps(res))
    if out:
        Path(out).mkdir(parents=True, exist_ok=True)
        (Path(out) / f"t16_stamps_{name}.json").write_text(json.dumps(res, indent=1) + "\n")
        np.save(Path(out) / f"t16_stamps_{name}.npy", st)


def sweep(out, label):
    import warnings; warnings.simplefilter("ignore")
    import accelerated_tinympc_amd as T
    sol, x0 = headline_solver(T)
    sol.set_dispatch(-1)
    sol.enable_timing(True)
    pts = []
    for mi in (4, 8, 12, 16, 20, 24):
        sol.set_settings(0.0, 0.0, mi, 1, 1, 1)
        ms = []
        for r in range(5):
            sol.reset_workspace(); sol.set_x0(x0); sol.solve_async(); sol.synchronize()
            if r >= 1: ms.append(sol.last_solve_ms())
        pts.append((mi, float(np.median(ms))))
    x, y = np.array(pts).T
    slope, icpt = np.polyfit(x, y, 1)
    res = {"label": label, "kernel": sol.kernel_name(), "points_ms": pts, "slope_ms_per_iter": round(float(slope), 5), "intercept_ms": round(float(icpt), 4)}
    sol.close()
    print(json.dumps(res))
    if out:
        Path(out).mkdir(parents=True, exist_ok=True)
        (Path(out) / f"t16_sweep_{label}.json").write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    mode, rest = sys.argv[1], sys.argv[2:]
    out = None
    if "--out" in rest:
        i = rest.index("--out"); out = rest[i + 1]; rest = rest[:i] + rest[i + 2:]
    if mode == "build":
        build(dict(a.split("=", 1) for a in rest) if rest else {"stamp": ""})
    elif mode == "run":
        run(rest[0], out)
    elif mode == "sweep":
        sweep(out, rest[0] if rest else "product")
    else:
        raise SystemExit(__doc__)
