"""The closed-loop plan table: which kernel a closed-loop run launches, whether its steps stay on chip or are replayed, and what it computes.

    python tools/closed_loop_plan_table.py --write tests/golden/closed_loop_plan.json    (record; on an MI355X, TINYMPC_HIP_LIB naming the reference build)
    python tools/closed_loop_plan_table.py --check tests/golden/closed_loop_plan.json    (replay on the library under test, print the first differences)
    python tools/closed_loop_plan_table.py --plan                                        (no GPU: the row list and the coverage check on a stubbed record)

tests/test_closed_loop_plan_gpu.py replays the committed table on the library under test and compares every field for equality.  The table is a
RECORD of the library of the commit before the loop decision moved into resolve_plan (KernelPlan::loop, csrc/tinympc_batch.hip); it is never
regenerated from the library under test: --write refuses to run unless TINYMPC_HIP_LIB names the build whose behaviour is the reference.
tests/golden/kernel_choice.json drives mpc_run_async on shared models only; this table drives the plant, the disturbance, the state trajectory,
the per-step log and per-instance models through the same decision.

One handle per (class, batch, storage), built through the public Python API with max_iter 6, shared bounds and a window reference.  A row requests
its settings (only what changed since the row before), resets the workspace, x0 and the window starts, and records
  closed_loop_kernel_name() before and after, and for the call and an identical second one: the increase of tiny_batch_debug_graph_captures
  (0 / 0: the steps ran on chip; 1 / 0: captured, then replayed), dispatch_applied(), and the crc32 of u0_traj, x_traj, iter_log, status_log,
  the final x0 and iter[] (0 for an output the call does not have) — or, refused, the call's error text.
The call is mpc_run_log where the row asks for the logs and mpc_run_sim where it does not.

Settings of a row (the ten characters of its key, in this order):
  k set_row_kernel 0, 1, 2, 3, 5, 6, 7 | v select_kernel 0 (automatic: exact) or 3 (fma) | b bounds 0 shared, 1 per instance | p plant 0 none, 1 shared,
  2 per instance | w a disturbance is passed | x the state trajectory is asked for | l the logs are asked for | m per-instance models |
  a window_advance 0 / 1 | n steps 1 / 3

The product is thinned where the factors do not interact in the decision:
  * block A, the call: k x n x six (p, w, x, l) — none, each of plant, w, x_traj and the logs alone, all together with a plant per instance;
    handles under fp16 storage take three of the six (none, plant, logs);
  * block B, the handle: from the plain run of three steps, each of fma arithmetic, per-instance bounds and window_advance 1 alone, then per-instance
    bounds with the logs and fma with a plant, for every k;
  * block C, per-instance models (fp32 storage): the six of block A x n on the 16-lane class for k = 0, 1, three of them on the wave class for
    k = 6, 7 (everything else resolves to the run-time-dimension kernel, at 0.2 - 1 s per solve), and the refused forced tile16;
  * the batch enters no rule at these sizes: B = 5 everywhere, and B = 17 (one full tile and a padding tile) for k = 0, 5 on the tile16 class.
When it writes, the tool asserts (check_coverage) that for each of the six terms of the on-chip decision two rows differ in that term alone and end on
different sides, and that a refused call is recorded with its text."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

KEYS = "kvbpwxlman"
BASE = dict(k=0, v=0, b=0, p=0, w=0, x=0, l=0, m=0, a=0, n=3)
MAX_ITER = 6
ROWS = 64  # of the reference table
QUAD, CART, LOOP, WAVE = (12, 4, 10), (4, 1, 10), (12, 4, 33), (16, 8, 10)
ROW_KERNELS = (0, 1, 2, 3, 5, 6, 7)
HANDLES = [dict(cls=list(c), batch=b, storage=s) for c, b, s in
           ((QUAD, 5, 32), (QUAD, 5, 16), (QUAD, 17, 32), (CART, 5, 32), (CART, 5, 16), (LOOP, 5, 32), (WAVE, 5, 32))]
CALLS = [dict(), dict(p=1), dict(w=1), dict(x=1), dict(l=1), dict(p=2, w=1, x=1, l=1)]  # block A's six


def key_of(cfg: dict) -> str:
    return "".join(str(cfg[c]) for c in KEYS)


def cfg_of(key: str) -> dict:
    return {c: int(ch) for c, ch in zip(KEYS, key)}


def plan(spec: dict, accepted: list) -> list:
    """the rows of one handle (module docstring)"""
    cls, h16 = tuple(spec["cls"]), spec["storage"] == 16
    ks = [k for k in ROW_KERNELS if k in accepted]
    if spec["batch"] == 17:
        ks = [k for k in ks if k in (0, 5)]
    rows = []
    add = lambda **kw: rows.append(key_of({**BASE, **kw}))
    for k in ks:
        for n in (3, 1):
            for c in ([CALLS[0], CALLS[1], CALLS[4]] if h16 else CALLS):
                add(k=k, n=n, **c)
        for kw in (dict(v=3), dict(b=1), dict(a=1), dict(b=1, l=1), dict(v=3, p=1)):
            add(k=k, **kw)
    if not h16 and spec["batch"] == 5:
        if cls == QUAD:
            for k in (0, 1):
                for n in (3, 1):
                    for c in CALLS:
                        add(m=1, k=k, n=n, **c)
            add(m=1, k=5)
        if cls == WAVE:
            for k in (k for k in (6, 7) if k in accepted):
                for c in (CALLS[0], CALLS[4], CALLS[1]):
                    add(m=1, k=k, **c)
    return rows


class Inputs:
    """the arrays one (class, batch) needs, built once and shared by its storages"""

    def __init__(self, T, cls, batch):
        nx, nu, N = cls
        rng = np.random.default_rng(1000 * nx + 10 * nu + N)
        p = self.prob = _kc()._problem(T, cls)
        self.x0 = (0.1 * rng.standard_normal((batch, nx))).astype(np.float32)
        sh = T.problems.bounds_arrays(p)
        scale = rng.uniform(0.5, 1.0, size=(batch, 1, 1)).astype(np.float32)
        self.bounds = (sh, [np.ascontiguousarray(a[None] * scale) for a in sh])
        self.table = (0.05 * rng.standard_normal((ROWS, nx))).astype(np.float32)
        self.start = (np.arange(batch) * 3 % (ROWS - N)).astype(np.int32)
        A, B = np.asarray(p["Adyn"], np.float32), np.asarray(p["Bdyn"], np.float32)
        sA, sB = (1 + 0.02 * rng.standard_normal((batch,) + A.shape)).astype(np.float32), (1 + 0.02 * rng.standard_normal((batch,) + B.shape)).astype(np.float32)
        self.plants = (None, (A * sA[0], B * sB[0]), (A[None] * sA, B[None] * sB))
        self.w = (0.01 * rng.standard_normal((3, batch, nx))).astype(np.float32)
        self.models = {k: np.broadcast_to(np.asarray(p[k], np.float32), (batch,) + np.shape(p[k])) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")}
        self.models["Q"] = np.broadcast_to(np.asarray(p["Q"], np.float32).ravel(), (batch, nx))
        self.models["rho"] = np.full(batch, p["rho"], np.float32)


def _kc():
    """tools/kernel_choice_table.py, for what the two tools share (_problem, _try)"""
    import importlib.util
    name = "tools_kernel_choice_table"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, ROOT / "tools" / "kernel_choice_table.py")
        sys.modules[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[name])
    return sys.modules[name]


def run_handle(T, spec: dict, inp: Inputs, rows=None) -> dict:
    """Build the handle of `spec` and run its rows (those of plan() when `rows` is None, the recorded keys otherwise).  Returns the handle's record:
    {"row_kernels": the accepted ones, "rows": [[key, [name before, name after, setters refused], first call, second call], ...]}"""
    _try = _kc()._try
    crc = lambda a: 0 if a is None else zlib.crc32(np.ascontiguousarray(a).tobytes())
    sol = T.TinyBatchSolver(inp.prob, spec["batch"], settings=dict(max_iter=MAX_ITER))
    rec = dict(row_kernels=[], rows=[])
    try:
        if spec["storage"] != 32:
            sol.set_storage(spec["storage"])
        rec["row_kernels"] = [k for k in ROW_KERNELS if _try([], "set_row_kernel", sol.set_row_kernel, k)]
        sol.set_row_kernel(0)
        sol.set_bounds(*inp.bounds[0])
        cur = dict(BASE)
        captures = lambda: int(sol.lib.tiny_batch_debug_graph_captures(sol._h))
        for key in (plan(spec, rec["row_kernels"]) if rows is None else rows):
            cfg, fails = cfg_of(key), []
            if cfg["k"] != cur["k"]:
                _try(fails, "set_row_kernel", sol.set_row_kernel, cfg["k"])
            if cfg["m"] != cur["m"]:
                _try(fails, "set_models", sol.set_models, inp.models) if cfg["m"] else _try(fails, "clear_models", sol.clear_models)
            if cfg["b"] != cur["b"]:
                _try(fails, "set_bounds", sol.set_bounds, *inp.bounds[cfg["b"]])
            if cfg["p"] != cur["p"]:
                _try(fails, "set_plant", sol.set_plant, *inp.plants[cfg["p"]]) if cfg["p"] else _try(fails, "clear_plant", sol.clear_plant)
            if cfg["v"] != cur["v"]:
                _try(fails, "select_kernel", sol.select_kernel, cfg["v"])
            cur = cfg
            n, w = cfg["n"], (inp.w[:cfg["n"]] if cfg["w"] else None)
            calls, before = [], None
            for _ in range(2):
                sol.reset_workspace()
                if not calls:  # (the second call's window starts are where the first left them: setting them again would drop the captured graph)
                    sol.set_xref_window(inp.table, inp.start)
                sol.set_x0(inp.x0)
                before = before or sol.closed_loop_kernel_name()
                c0, f = captures(), []

                def call():
                    if cfg["l"]:
                        return sol.mpc_run_log(n, cfg["a"], w, record_x=bool(cfg["x"]))
                    u0, xt = sol.mpc_run_sim(n, cfg["a"], w, record_x=bool(cfg["x"]))
                    return {"u0": u0, "x": xt, "iter": None, "status": None}
                out = []
                if _try(f, "run", lambda: out.append(call())):
                    o = out[0]
                    calls.append([captures() - c0, sol.dispatch_applied(), crc(o["u0"]), crc(o["x"]), crc(o["iter"]), crc(o["status"]), crc(sol.get_x0()), crc(sol.get_status()[0])])
                else:
                    calls.append(f[0][1])
            rec["rows"].append([key, [before, sol.closed_loop_kernel_name(), fails]] + calls)
    finally:
        sol.close()
    return rec


class Session:
    def __init__(self):
        import accelerated_tinympc_amd as T
        self.T = T
        T.load_library()
        self._inp = (None, None)

    def run(self, spec, rows=None):
        key = (tuple(spec["cls"]), spec["batch"])
        if self._inp[0] != key:
            self._inp = (key, Inputs(self.T, spec["cls"], spec["batch"]))
        return run_handle(self.T, spec, self._inp[1], rows)


def save_table(handles: list, path: Path):
    path.parent.mkdir(parents=True, exist_ok=True)
    body = []
    for h in handles:
        rows = ",\n   ".join(json.dumps(r, separators=(",", ":")) for r in h["rows"])
        head = ", ".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in h.items() if k != "rows")
        body.append(" {" + head + ', "rows": [\n   ' + rows + "\n  ]}")
    path.write_text('{"keys": ' + json.dumps(KEYS) + ', "max_iter": ' + str(MAX_ITER) + ', "handles": [\n' + ",\n".join(body) + "\n]}\n")


def load_table(path: Path) -> dict:
    return json.loads(path.read_text())


# ---- coverage the thinning must keep -----------------------------------------------------------------------------------------------
# the six terms of the on-chip decision (plan_of, csrc/tinympc_batch.hip): the key characters of which exactly one differs between the two rows
# ("s": the handles' storage), and what both rows' kernel must be for the pair to be about this term
TERMS = {
    "the kernel has an on-chip loop": ("k", lambda fam, c: True),
    "fp32 storage": ("s", lambda fam, c: fam == "rowlane"),
    "more than one step": ("n", lambda fam, c: True),
    "batch-shared bounds": ("b", lambda fam, c: fam == "rowlane"),
    "a simulated run stays on chip on the 16-lane kernel only": ("pwx", lambda fam, c: fam == "quadlane"),
    "no log on the matrix-core kernel or with per-instance models": ("l", lambda fam, c: fam == "tile16" or c["m"] == 1),
}


def check_coverage(table: dict):
    rows, refused = [], []
    for h in table["handles"]:
        for key, (before, after, fails), c1, c2 in h["rows"]:
            if isinstance(c1, str):
                refused.append(c1)
            elif not isinstance(c2, str):
                rows.append((tuple(h["cls"]), h["batch"], key + str(h["storage"] // 16), after.split("<")[0], (c1[0], c2[0])))
    assert any("rc=" in t and len(t) > 20 for t in refused), "no refused call with its text"
    sides = {(0, 0): "on chip", (1, 0): "replayed"}
    assert all(d in sides for *_, d in rows), f"capture counts that are neither on chip nor replayed: {sorted({d for *_, d in rows} - set(sides))}"
    by_key = {r[:3]: r for r in rows}
    missing = []
    for term, (chars, about) in TERMS.items():
        idx = [(KEYS + "s").index(c) for c in chars]
        hit = False
        for cls, batch, key, fam, d in rows:
            if d != (0, 0) or not about(fam, cfg_of(key)):
                continue
            for (c2, b2, k2), (_, _, _, fam2, d2) in by_key.items():
                diff = [i for i in range(len(key)) if key[i] != k2[i]]
                if (c2, b2) == (cls, batch) and len(diff) == 1 and diff[0] in idx and d2 == (1, 0) and (chars == "k" or about(fam2, cfg_of(k2))):
                    hit = True
        if not hit:
            missing.append(term)
    assert not missing, f"no pair of rows that differs in this term alone and ends on different sides: {missing}"


def stub_record() -> dict:
    """no GPU: every handle's rows with the record the decision as DESIGN.md states it would leave (every row kernel accepted that the class could have)"""
    fam_of = {QUAD: {0: "rowlane", 1: "rowlane", 2: "rowloop", 3: "rowstream", 5: "tile16"}, CART: {0: "quadlane", 1: "rowlane", 2: "rowloop", 3: "rowstream"},
              LOOP: {0: "rowloop", 2: "rowloop", 3: "rowstream", 5: "rowloop"}, WAVE: {0: "waveres", 6: "wavestream", 7: "waveres"}}
    handles = []
    for spec in HANDLES:
        fams = fam_of[tuple(spec["cls"])]
        rows = []
        for key in plan(spec, list(fams)):
            c = cfg_of(key)
            sim, h16 = bool(c["p"] or c["w"] or c["x"]), spec["storage"] == 16
            fam = fams[c["k"]]
            if fam == "tile16" and (h16 or c["b"] or (sim and c["n"] > 1)):
                fam = "rowlane"
            if c["m"] and c["k"] == 5:
                rows.append([key, ["unsupported", "unsupported", []], "rc=-3: refused by the stub", "rc=-3: refused by the stub"])
                continue
            on_chip = fam in ("rowlane", "quadlane", "tile16") and not h16 and c["n"] > 1 and not c["b"] and (not sim or fam == "rowlane") and \
                not (c["l"] and (fam == "tile16" or c["m"]))
            rows.append([key, [fam + "<>", fam + "<>", []], [0 if on_chip else 1] + [0] * 7, [0] * 8])
        handles.append({**spec, "row_kernels": list(fams), "rows": rows})
    return dict(keys=KEYS, handles=handles)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    ap.add_argument("--plan", action="store_true", help="no GPU: count the rows and run the coverage check on a stubbed record")
    a = ap.parse_args()
    t0 = time.time()
    if a.plan:
        table = stub_record()
        for h in table["handles"]:
            print(f"{h['cls']} B={h['batch']} storage={h['storage']}: {len(h['rows'])} rows")
        check_coverage(table)
        print(f"{sum(len(h['rows']) for h in table['handles'])} rows; coverage ok on the stub")
    if a.write:
        assert os.environ.get("TINYMPC_HIP_LIB"), "--write records a REFERENCE build: name it in TINYMPC_HIP_LIB (never the library under test)"
        ses, handles = Session(), []
        for spec in HANDLES:
            t = time.time()
            handles.append({**spec, **ses.run(spec)})
            print(f"{spec['cls']} B={spec['batch']} storage={spec['storage']}: {len(handles[-1]['rows'])} rows, {time.time() - t:.1f} s", flush=True)
        save_table(handles, Path(a.write))
        print(f"{sum(len(h['rows']) for h in handles)} rows, {Path(a.write).stat().st_size} bytes, {time.time() - t0:.0f} s", flush=True)
        check_coverage(load_table(Path(a.write)))
        print("coverage ok")
    if a.check:
        table, ses, bad = load_table(Path(a.check)), Session(), 0
        for h in table["handles"]:
            got = ses.run({k: h[k] for k in ("cls", "batch", "storage")}, [r[0] for r in h["rows"]])
            diffs = [(w, g) for w, g in zip(h["rows"], json.loads(json.dumps(got["rows"]))) if w != g] + ([("row kernels", got["row_kernels"])] if got["row_kernels"] != h["row_kernels"] else [])
            bad += len(diffs)
            print(f"{h['cls']} B={h['batch']} storage={h['storage']}: {len(h['rows'])} rows, {len(diffs)} differ", flush=True)
            for w, g in diffs[:3]:
                print("   recorded", w, "\n   now     ", g)
        print(f"{bad} differences, {time.time() - t0:.0f} s")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
