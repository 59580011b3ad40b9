"""The fp64 library's kernel-choice table: what a handle state names, refuses and computes, recorded row by row.

    TINYMPC_HIP_LIB=<the library to record> python tools/kernel_choice64_table.py --write tests/golden/kernel_choice64.json --commit <its commit>
    python tools/kernel_choice64_table.py --check tests/golden/kernel_choice64.json     (replay on the library under test, print the first differences)

tests/test_kernel_choice64_gpu.py replays the committed table on the library under test and compares every field for equality.  The table is a
RECORD of the library before the choice was gathered into resolve_plan64 (csrc/tinympc_batch64.hip): it is never regenerated from the library
under test, --write refuses to run without TINYMPC_HIP_LIB naming the build to record, and the table stores the commit that build was made from.

One handle per (class, batch) through the public Python API (TinyBatchSolver64): a seeded random system, x0 / bounds / references from
tests/helpers.closed_loop_inputs (geometric x0 amplitudes over tightened bounds: some instances sit on a bound and run out of iterations, some
converge at once), the plant and disturbance recipe of tests/test_sim_loop64_gpu.py, "models on" = two distinct models alternating over the batch.

  classes  (12,4,10) unrolled body | (4,1,13) capacity-32 body | (12,4,40) capacity-64 body: rows for a solve, the sequence for a run |
           (12,4,70) beyond the sixteen-lane kernel | (16,4,10) no sixteen-lane instantiation      batches 5 and 67

A row's settings (its key, six numbers): s select_kernel 0..2 | m models 0/1 | p plant 0 none, 1 shared, 2 per instance | i max_iter |
e TINYMPC_F64_LOOP 0 unset, 1 "sequence" | r reference 0 window (advance 1), 1 plain per-instance array.

Name rows: the full product s x m x p x i in (0, 1, 25) x e on the window reference — select_kernel's return (its error text where refused: the
choice of the row before then stays), kernel_name(), closed_loop_kernel_name().  No launch.
Result rows: a thinned set of settings (result_cfgs), each from a zeroed workspace, then the calls of CALLS in order, every call starting from what
the call before left: solve, mpc_step, mpc_step_sim(w), and with steps in (1, 3) mpc_run, mpc_run_traj, mpc_run_sim with w / x_traj absent and
present.  Per call: the return code (the error text where refused) and the sha256 over the raw bytes of the twelve work arrays, status, iter, the
residuals, the window starts, u0_traj and x_traj.  When it writes, the tool asserts that the result rows reach every distinct plan of the product,
every arm of the run driver, every plant-kernel choice of a step, and both kinds of reference (check_coverage)."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for _p in (ROOT, ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

ENV = "TINYMPC_F64_LOOP"
CLASSES = [(12, 4, 10), (4, 1, 13), (12, 4, 40), (12, 4, 70), (16, 4, 10)]
BATCHES = (5, 67)
ROWS_BY_DEFAULT = ((12, 4, 10), (4, 1, 13), (12, 4, 40))  # the classes whose automatic choice is the sixteen-lane kernel
MAX_ITERS = (0, 1, 25)
KEYS = "smpier"
SETTINGS = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=25, check_termination=1, en_state_bound=1, en_input_bound=1)
RUN_STEPS = (1, 3)
# (name, steps, w passed, x_traj asked for); steps = 0: not a run
CALLS = [("solve", 0, 0, 0), ("mpc_step", 0, 0, 0), ("mpc_step_sim", 0, 1, 0)]
for _n in RUN_STEPS:
    CALLS += [("mpc_run", _n, 0, 0), ("mpc_run_traj", _n, 0, 0), ("mpc_run_sim", _n, 0, 0), ("mpc_run_sim", _n, 1, 0), ("mpc_run_sim", _n, 0, 1), ("mpc_run_sim", _n, 1, 1)]


def handle_specs() -> list:
    return [dict(cls=list(c), batch=b) for c in CLASSES for b in BATCHES]


def name_cfgs() -> list:
    """the full product, ordered so that the uploads (models, plant) change least often"""
    return [dict(s=s, m=m, p=p, i=i, e=e, r=0) for m in (0, 1) for p in (0, 1, 2) for s in (0, 1, 2) for i in MAX_ITERS for e in (0, 1)]


def result_cfgs(cls, batch) -> list:
    """The settings whose results are recorded.  Every handle: models x plant under the automatic choice; where that is the sixteen-lane kernel
    also the sequence by request and thread64 by choice, with and without models.  The plan reads neither the batch nor max_iter >= 1, so the small
    batch alone carries the other values of max_iter, the sequence by request against a plant per instance, and the plain reference; and thread64,
    which walks the horizon serially (tens of milliseconds per solve of 25 iterations), stops after one iteration except at N = 10 on the small batch."""
    rows, small = tuple(cls) in ROWS_BY_DEFAULT, batch == BATCHES[0]
    full = 25 if small and cls[2] == 10 else 1  # max_iter of a row that thread64 runs
    base = dict(s=0, m=0, p=0, i=25 if rows else 1, e=0, r=0)
    out = [dict(base, m=m, p=p) for m in (0, 1) for p in (0, 1, 2)]
    if rows:
        out += [dict(base, m=m, e=1) for m in (0, 1)] + [dict(base, m=m, s=1, i=full) for m in (0, 1)]
    if small:
        out += [dict(base, m=m, i=i) for m in (0, 1) for i in ((0, 1) if rows else (0, full)) if i != base["i"]]
        out += [dict(base, m=m, p=2, e=1) for m in (0, 1)] + [dict(base, m=m, r=1) for m in (0, 1)]
    return out


def key_of(cfg: dict) -> list:
    return [cfg[k] for k in KEYS]


def cfg_of(key) -> dict:
    return dict(zip(KEYS, key))


class Inputs:
    """everything the handle of one (class, batch) runs on"""

    def __init__(self, T, cls, batch):
        from helpers import closed_loop_inputs
        nx, nu, N = cls
        pr = T.problems
        self.prob = pr.random_system(nx, nu, N, seed=100 * nx + nu)
        other = pr.random_system(nx, nu, N, seed=100 * nx + nu + 1)
        seed = 6400 + nx + N
        self.x0, self.window, self.bnds = closed_loop_inputs(self.prob, batch, "window", seed, dtype=np.float64)
        self.plain = closed_loop_inputs(self.prob, batch, "inst", seed + 1, dtype=np.float64)[1]
        which = np.arange(batch) % 2
        self.models = {k: np.stack([np.asarray((self.prob, other)[m][k], np.float64) for m in which]) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn", "Q")}
        self.models["rho"] = np.array([(self.prob, other)[m]["rho"] for m in which], np.float64)
        rng = np.random.default_rng(seed + 2)
        A = np.broadcast_to(np.asarray(self.prob["Adyn"], np.float64), (batch, nx, nx))
        Bm = np.broadcast_to(np.asarray(self.prob["Bdyn"], np.float64), (batch, nx, nu))
        Ap, Bp = A * (1 + 0.05 * rng.standard_normal(A.shape)), Bm * (1 + 0.05 * rng.standard_normal(Bm.shape))
        self.plants = (None, (Ap[0], Bp[0]), (Ap, Bp))
        self.w = 0.01 * rng.standard_normal((max(RUN_STEPS), batch, nx))


def _try(fn, *a, **kw):
    """(return value, None) or (None, the error text)"""
    from accelerated_tinympc_amd import TinyBatchError
    try:
        return fn(*a, **kw), None
    except TinyBatchError as e:
        return None, str(e)


def _digest(sol, window, extra) -> str:
    from accelerated_tinympc_amd.solver import ARRAY_IDS
    h = hashlib.sha256()
    for k in ARRAY_IDS:
        h.update(sol.get_array(k).tobytes())
    it, st, res = sol.get_status()
    for a in (st, it, res, sol.xref_start() if window else None, *extra):
        h.update(b"-" if a is None else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _apply(sol, inp, cfg, cur):
    """request a row's settings (models and plant only where they changed; select_kernel always and last); returns select_kernel's outcome"""
    if cfg["m"] != cur.get("m"):
        sol.set_models(inp.models) if cfg["m"] else sol.clear_models()
    if cfg["p"] != cur.get("p"):
        sol.set_plant(*inp.plants[cfg["p"]]) if cfg["p"] else sol.clear_plant()
    if cfg["i"] != cur.get("i"):
        sol.set_settings(**dict(SETTINGS, max_iter=cfg["i"]))
    if cfg["e"]:
        os.environ[ENV] = "sequence"
    else:
        os.environ.pop(ENV, None)
    _, err = _try(sol.select_kernel, cfg["s"])
    cur.update(cfg)
    return 0 if err is None else err


def _call(sol, inp, name, steps, w, x, adv):
    """one entry of CALLS: (rc or error text, the trajectories it returned)"""
    if name == "solve":
        rc, err = _try(sol.solve)
        out = ()
    elif name == "mpc_step":
        rc, err = _try(sol.mpc_step)
        out = ()
    elif name == "mpc_step_sim":
        rc, err = _try(sol.mpc_step_sim, inp.w[0])
        out = ()
    elif name == "mpc_run":
        rc, err = _try(sol.mpc_run, steps, adv)
        out = ()
    elif name == "mpc_run_traj":
        out, err = _try(sol.mpc_run_traj, steps, adv)
        rc, out = 0, (out,)
    else:
        out, err = _try(sol.mpc_run_sim, steps, adv, inp.w[:steps] if w else None, bool(x))
        rc = 0
    return (rc if err is None else err), (() if err is not None else tuple(out))


def run_handle(T, spec: dict, names=None, results=None) -> dict:
    """Build the handle of `spec` and run its name rows, then its result rows (those of name_cfgs() / result_cfgs() when None, the recorded keys
    otherwise).  Returns {"names": [[key, select outcome, kernel_name, closed_loop_kernel_name], ...], "results": [[key, [[rc, sha256], ...]], ...]}"""
    from accelerated_tinympc_amd.solver import ARRAY_IDS
    cls, batch = spec["cls"], spec["batch"]
    inp = Inputs(T, cls, batch)
    keep = os.environ.get(ENV)
    sol = T.TinyBatchSolver64(inp.prob, batch, settings=SETTINGS)
    rec = dict(names=[], results=[])
    try:
        sol.set_bounds(*inp.bnds)
        sol.set_xref_window(*inp.window)
        sol.set_x0(inp.x0)
        cur = dict(i=SETTINGS["max_iter"])
        for key in ([key_of(c) for c in name_cfgs()] if names is None else names):
            sel = _apply(sol, inp, cfg_of(key), cur)
            rec["names"].append([key, sel, sol.kernel_name(), sol.closed_loop_kernel_name()])
        zeros = {k: np.zeros(sol._xshape(k)) for k in ARRAY_IDS}
        zeros.update(iter=np.zeros(batch, np.int32), status=np.zeros(batch, np.int32), residuals=np.zeros((batch, 4)))
        for key in ([key_of(c) for c in result_cfgs(cls, batch)] if results is None else results):
            cfg = cfg_of(key)
            sel = _apply(sol, inp, cfg, cur)
            assert sel == 0, f"a result row's select_kernel is refused: {sel}"
            sol.set_state(zeros)
            sol.set_xref(inp.plain) if cfg["r"] else sol.set_xref_window(*inp.window)
            sol.set_x0(inp.x0)
            outs = []
            for name, steps, w, x in CALLS:
                rc, extra = _call(sol, inp, name, steps, w, x, 0 if cfg["r"] else 1)
                outs.append([rc, _digest(sol, not cfg["r"], extra)])
            rec["results"].append([key, outs])
    finally:
        sol.close()
        if keep is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = keep
    return rec


# ---- coverage the thinning must keep -----------------------------------------------------------------------------------------------
def plan_of(kernel_name: str, loop_name: str, cfg: dict, steps: int, w: int, x: int) -> tuple:
    """(family, body, pm, loop, sim) of one call, read off the two recorded names and the row's settings"""
    family = kernel_name.split("<")[0]
    body = "" if family == "thread64" else "cap32" if "n<=32" in kernel_name else "cap64" if "n<=64" in kernel_name else "unrolled"
    loop = "none" if not steps else "onchip" if (",mpc" in loop_name or ",sim" in loop_name) else "sequence"
    return family, body, bool(cfg["m"]), loop, bool(cfg["p"] or w or x or cfg["m"])


def check_coverage(table: dict):
    arms, steps_plant, refs = set(), set(), set()
    for h in table["handles"]:
        named = {tuple(r[0]): r for r in h["names"]}
        want = {plan_of(r[2], r[3], cfg_of(r[0]), steps, w, x) for r in h["names"] for _, steps, w, x in CALLS}
        got = set()
        for key, outs in h["results"]:
            cfg = cfg_of(key)
            r = named[tuple(key[:5]) + (0,)]  # (the names do not read the reference)
            assert len(outs) == len(CALLS) and all(isinstance(o[0], int) and o[0] >= 0 for o in outs), f"a refused call among the result rows: {key}"
            refs.add(cfg["r"])
            for (name, steps, w, x), _ in zip(CALLS, outs):
                plan = plan_of(r[2], r[3], cfg, steps, w, x)
                got.add(plan)
                family, _, pm, loop, sim = plan
                if loop == "onchip":
                    arms.add("models" if pm else "nominal" if not sim else "sim, steps > 1" if steps > 1 else "sim, one step")
                elif loop == "sequence":
                    arms.add("sequence " + family)
                elif name.startswith("mpc_step"):
                    steps_plant.add("model" if not sim else "own" if pm and not cfg["p"] else ("w", "shared", "inst")[cfg["p"]])
        assert want <= got, f"{h['cls']} B={h['batch']}: plans of the product without a result row: {sorted(want - got)}"
    assert arms == {"sequence rows64", "sequence thread64", "nominal", "sim, steps > 1", "sim, one step", "models"}, f"arms of the run driver: {sorted(arms)}"
    assert steps_plant == {"model", "w", "shared", "inst", "own"}, f"plant kernels of a step: {sorted(steps_plant)}"
    assert refs == {0, 1}, "a window reference and a plain one"
    assert [dict(cls=h["cls"], batch=h["batch"]) for h in table["handles"]] == handle_specs()
    assert all([r[0] for r in h["names"]] == [key_of(c) for c in name_cfgs()] for h in table["handles"]), "the name rows are the full product"
    sels = [r[1] for h in table["handles"] for r in h["names"] if r[0][0] == 2]
    assert any(s == 0 for s in sels) and any(isinstance(s, str) and "no instantiation" in s for s in sels), "select_kernel(2) accepted and refused"
    bodies = {plan_of(r[2], r[3], cfg_of(r[0]), 0, 0, 0)[:2] for h in table["handles"] for r in h["names"]}
    assert bodies == {("rows64", "unrolled"), ("rows64", "cap32"), ("rows64", "cap64"), ("thread64", "")}, sorted(bodies)


# ---- the committed form: one row per line ------------------------------------------------------------------------------------------
def save_table(table: dict, path: Path):
    line = lambda v: json.dumps(v, separators=(",", ":"))
    out = ["{", f' "commit": {json.dumps(table["commit"])},', f' "keys": {json.dumps(KEYS)},', f' "calls": {line(CALLS)},', ' "handles": [']
    for n, h in enumerate(table["handles"]):
        out.append(f'  {{"cls": {line(h["cls"])}, "batch": {h["batch"]},')
        out.append('   "names": [\n    ' + ",\n    ".join(line(r) for r in h["names"]) + "\n   ],")
        out.append('   "results": [\n    ' + ",\n    ".join(line(r) for r in h["results"]) + "\n   ]}" + ("," if n + 1 < len(table["handles"]) else ""))
    out += [" ]", "}"]
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(out) + "\n")


def load_table(path: Path) -> dict:
    table = json.loads(path.read_text())
    assert table["keys"] == KEYS and [tuple(c) for c in table["calls"]] == CALLS, "the table was written for other rows"
    return table


def replay(T, h: dict) -> dict:
    return run_handle(T, dict(cls=h["cls"], batch=h["batch"]), [r[0] for r in h["names"]], [r[0] for r in h["results"]])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="JSON")
    ap.add_argument("--commit", help="with --write: the commit the library under TINYMPC_HIP_LIB was built from")
    ap.add_argument("--check", metavar="JSON")
    a = ap.parse_args()
    t0 = time.time()
    if a.write:
        if not os.environ.get("TINYMPC_HIP_LIB") or not a.commit:
            sys.exit("refusing to write: the table records the library of a named commit (set TINYMPC_HIP_LIB to its build and pass --commit), never the one under test")
    import accelerated_tinympc_amd as T
    if a.write:
        table = dict(commit=a.commit, handles=[])
        for spec in handle_specs():
            t = time.time()
            rec = run_handle(T, spec)
            table["handles"].append({**spec, **rec})
            print(f"{spec['cls']} B={spec['batch']}: {len(rec['names'])} name rows, {len(rec['results'])} result rows of {len(CALLS)} calls, {time.time() - t:.2f} s", flush=True)
        check_coverage(table)
        print("coverage ok")
        save_table(table, Path(a.write))
        print(f"{Path(a.write).stat().st_size} bytes, {time.time() - t0:.1f} s")
    if a.check:
        table = load_table(Path(a.check))
        bad = 0
        for h in table["handles"]:
            got = replay(T, h)
            diffs = [(w, g) for part in ("names", "results") for w, g in zip(h[part], got[part]) if w != g]
            bad += len(diffs)
            print(f"{h['cls']} B={h['batch']}: {len(h['names'])} + {len(h['results'])} rows, {len(diffs)} differ", flush=True)
            for w, g in diffs[:3]:
                print("   recorded", w, "\n   now     ", g)
        print(f"{bad} differences, {time.time() - t0:.1f} s")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
