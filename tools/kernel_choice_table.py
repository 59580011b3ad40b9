"""The kernel-choice table: which kernel, arithmetic and dispatch order the library picks for a handle state, recorded row by row.

    python tools/kernel_choice_table.py --write tests/golden/kernel_choice.json     (record; on an MI355X, with the library to be recorded)
    python tools/kernel_choice_table.py --check tests/golden/kernel_choice.json     (replay on the library under test, print the first differences)
    python tools/kernel_choice_table.py --dump tests/golden/kernel_choice.json      (every row in full; the rows are kept gzipped beside the .json)

tests/test_kernel_choice_gpu.py replays the committed table on the library under test and compares every field for equality.  The table is
a RECORD of the library before the selection code was gathered into resolve_plan (csrc/tinympc_batch.hip); it is never regenerated from the
library under test: record it with TINYMPC_HIP_LIB naming a build of the commit whose choice is the reference.

Handles are built through the public Python API only.  One handle per (class, batch, storage) is reused for all its rows; a row requests its
settings (only what changed since the row before, select_kernel always and last), optionally resets the workspace, and records
  kernel_name(), closed_loop_kernel_name(), arithmetic() (or its error text), every setter that was refused (name and error text),
and, on the handles that solve (at least 4 096 groups of four instances, and the small batch of every class): dispatch_applied() and the crc32
of iter[] after a solve, a second (warm) solve, mpc_run_async(3) and — on the large batches' rows that reset — a second mpc_run_async(3)
straight from a reset workspace, then tiny_batch_debug_graph_captures.  A row depends on the rows before it (a refused select_kernel leaves the variant of the
row before; a row that does not reset starts from the state the row before left): the replay runs them in the same order.

Settings of a row (the ten characters of its key, in this order):
  v select_kernel 0..4 | k set_row_kernel 0..8 | o optional terms 0 off, 1 Uref, 2 coeff_d2p | p per-instance models 0/1 |
  b bounds 0 shared, 1 per instance constant along the horizon, 2 per instance varying | x reference 0 never set, 1 shared, 2 per instance,
  3 window of a short table, 4 window of a table long enough that tile16 gives way (its length is found by doubling, header "long_rows") |
  d set_dispatch + 1 (0..3 for -1..2) | c a caller's dispatch order set | w workspace reset before the row | m max_iter 0: 6, 1: 1

The full product has 194 400 rows per handle; it is thinned where factors do not interact in the policy, to stay below the size of the largest
file under tests/golden/ and the run time of the other GPU test files:
  * set_row_kernel values the class refuses (one flag per class, fixed at create) are probed once per handle and recorded there, not per row;
    a storage the class refuses is recorded as the handle's only entry;
  * block A, the selection core: (v, k) x o in {off, Uref} x b in {shared, per instance constant} under the defaults of everything else, where
    (v, k) is k x the three variants that read it (auto, row exact, row fma) and k = 0 for the streaming and the run-time-dimension variant, which
    name one kernel each.  Per-instance models refuse storage 16, the optional terms and every forced row kernel but the 16-lane one, so p = 1
    takes (v, k) once — k only where the class has a 16-lane kernel — then per-instance bounds and Uref on three rows.  coeff_d2p alone
    (block D: (v, k)) — every rule asks "either optional term".  The run-time-dimension kernel takes 0.2 - 1 s per solve of these classes:
    the order of the rows keeps a refused request from leaving it selected;
  * block B, the tables: x x b x (k in auto, rowlane, tile16) x (v in auto, fma) x c x (d in auto, index order) on the tile16 class, the
    only one whose choice reads the reference kind, table length or whether per-instance rows vary; x x b alone elsewhere;
  * block C, dispatch: b in {shared, per instance} x (k in auto, rowlane, rowloop, tile16) x c x d x w on a window reference, then max_iter 1,
    fma arithmetic and a shared reference over k x d x w.  Dispatch orders need 4 096 groups, so they show on the two large quadrotor batches;
  * the batch only enters through the size rules: the classes without one get a small batch; (32, 16, 50) gets block A with shared bounds at
    each side of its three round boundaries; storage 16 / (16, 32) is refused by the classes without a 16-lane kernel.
When it writes, the tool asserts that the rows hit every kernel family, every refusal text of the variant resolution that a caller can reach,
and each of the differences between a lone solve and an on-chip run that the dispatch code keeps (check_coverage)."""
from __future__ import annotations

import argparse
import json
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

KEYS = "vkopbxdcwm"
BASE = dict(v=0, k=0, o=0, p=0, b=0, x=0, d=-1, c=0, w=1, m=0)
MAX_ITER = (6, 1)
SHORT_ROWS = 301
QUAD = (12, 4, 30)
WAVE = (32, 16, 50)
NO_EXACT = (5, 3, 10)  # nx = 5: no compiled class and outside the run-time-dimension kernel's alignment rule
CLASSES = [QUAD, (12, 4, 50), (12, 4, 33), (4, 1, 10), (8, 3, 7), (2, 2, 3), WAVE, (16, 8, 10), (8, 8, 6), NO_EXACT]
SMALL = 50
STORAGES = (32, 16, (16, 32))


def handle_specs(cu: int) -> list:
    """(class, batch, storage, full product?, solves?) of every handle, in table order"""
    out = []
    for cls in CLASSES:
        batches = [SMALL]
        if cls == QUAD:
            batches += [160 * cu - 1, 160 * cu]
        if cls == WAVE:
            batches += [8 * cu, 8 * cu + 1, 16 * cu, 16 * cu + 1, 24 * cu, 24 * cu + 1]
        for batch in batches:
            for sto in STORAGES:
                if sto != 32 and cls == WAVE and batch != SMALL:
                    continue  # refused: recorded once, at the small batch
                full = batch == SMALL or cls == QUAD
                out.append(dict(cls=list(cls), batch=batch, storage=list(sto) if isinstance(sto, tuple) else sto, full=full,
                                solves=batch == SMALL or (batch + 3) // 4 >= 4096))
    return out


def key_of(cfg: dict) -> str:
    return "".join(str(cfg[c] + 1 if c == "d" else cfg[c]) for c in KEYS)


def cfg_of(key: str) -> dict:
    return {c: int(ch) - (1 if c == "d" else 0) for c, ch in zip(KEYS, key)}


def plan(cls, full: bool, accepted: list) -> list:
    """the rows of one handle (module docstring), ordered so that the expensive settings change least often and x = 0 comes first"""
    t16 = tuple(cls) == QUAD
    rows = []
    add = lambda **kw: rows.append(key_of({**BASE, **kw}))
    kv = [(0, 4), (0, 1)] + [(k, v) for k in accepted for v in (0, 2, 3)]  # variants 4 and 1 first: a refused request then leaves a cheap kernel
    for b in ((0, 1) if full else (0,)):
        for o in (0, 1):
            for k, v in kv:
                add(b=b, o=o, k=k, v=v)
    for k, v in (kv if 1 in accepted else kv[:2] + [(0, v) for v in (0, 2, 3)]):
        add(p=1, k=k, v=v)
    if not full:
        return rows
    for kw in (dict(b=1, v=4), dict(b=1, v=0), dict(o=1, v=0)):
        add(p=1, **kw)
    for k, v in kv:
        add(o=2, k=k, v=v)
    for x in range(5):
        for b in range(3):
            if x == 0 and b < 2:
                continue  # block A
            for k in ([k for k in (0, 1, 5) if k in accepted] if t16 else [0]):
                for v in ((0, 3) if t16 else (0,)):
                    for c in ((0, 1) if t16 else (0,)):
                        for d in ((-1, 0) if t16 else (-1,)):
                            add(x=x, b=b, k=k, v=v, c=c, d=d)
    kc = [k for k in (0, 1, 2, 5) if k in accepted]
    dw = [(d, w) for d in (-1, 0, 1, 2) for w in (1, 0)]
    for b in (0, 1):
        for k in kc:
            for c in (0, 1):
                for d, w in dw:
                    add(x=3, b=b, k=k, c=c, d=d, w=w)
    for k in kc:
        for d, w in dw:
            add(x=3, k=k, d=d, w=w, m=1)
    for k in (k for k in (0, 5) if k in accepted):
        for d, w in dw:
            add(x=3, k=k, d=d, w=w, v=3)
    for k in (k for k in (0, 5) if k in accepted):
        for d, w in dw:
            add(x=1, k=k, d=d, w=w)
    return rows


def _problem(T, cls):
    pr = T.problems
    nx, nu, N = cls
    if (nx, nu) == (12, 4):
        return pr.quadrotor(20, N)
    if (nx, nu) == (4, 1):
        return pr.cartpole(N)
    return pr.random_system(nx, nu, N, seed=7)


class Inputs:
    """the arrays one (class, batch) needs, built once and shared by its storages"""

    def __init__(self, T, cls, batch, long_rows):
        nx, nu, N = cls
        rng = np.random.default_rng(1000 * nx + 10 * nu + N)
        self.prob = _problem(T, cls)
        self.x0 = (0.1 * rng.standard_normal((batch, nx))).astype(np.float32)
        sh = T.problems.bounds_arrays(self.prob)
        scale = rng.uniform(0.5, 1.0, size=(batch, 1, 1)).astype(np.float32)
        const = [np.ascontiguousarray(a[None] * scale) for a in sh]
        vary = [np.ascontiguousarray(a * np.linspace(1.0, 0.8, a.shape[1], dtype=np.float32)[None, :, None]) for a in const]
        self.bounds = (sh, const, vary)
        table = (0.05 * rng.standard_normal((long_rows, nx))).astype(np.float32)
        self.tables = (np.ascontiguousarray(table[:SHORT_ROWS]), table)
        self.start = (np.arange(batch) % (SHORT_ROWS - N)).astype(np.int32)
        self.xref_shared = np.ascontiguousarray(table[:N])
        self.xref_inst = np.ascontiguousarray(table[self.start[:, None] + np.arange(N)[None, :]])
        p = self.prob
        self.models = {k: np.broadcast_to(np.asarray(p[k], np.float32), (batch,) + np.shape(p[k])) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")}
        self.models["Q"] = np.broadcast_to(np.asarray(p["Q"], np.float32).ravel(), (batch, nx))
        self.models["rho"] = np.full(batch, p["rho"], np.float32)


def _try(fails, name, fn, *a, **kw):
    from accelerated_tinympc_amd import TinyBatchError
    try:
        fn(*a, **kw)
        return True
    except TinyBatchError as e:
        fails.append([name, str(e)])
        return False


def run_handle(T, spec: dict, inp: Inputs, order_ptr: int, rows=None) -> dict:
    """Build the handle of `spec` and run its rows (those of plan() when `rows` is None, the recorded keys otherwise).  Returns the handle's
    record: {"storage_refused": text or None, "row_kernels_refused": {k: text}, "rows": [[key, [kn, cl, arith, fails], ops or None], ...]}"""
    cls, batch, sto = spec["cls"], spec["batch"], spec["storage"]
    nx, nu, N = cls
    sol = T.TinyBatchSolver(inp.prob, batch, settings=dict(max_iter=MAX_ITER[0]))
    rec = dict(storage_refused=None, row_kernels_refused={}, rows=[])
    try:
        if sto != 32:
            f = []
            _try(f, "set_storage", sol.set_storage, *(sto if isinstance(sto, list) else [sto]))
            if f:
                rec["storage_refused"] = f[0][1]
                return rec
        accepted = []
        for k in range(9):
            f = []
            if _try(f, "set_row_kernel", sol.set_row_kernel, k):
                accepted.append(k)
            else:
                rec["row_kernels_refused"][str(k)] = f[0][1]
        sol.set_row_kernel(0)
        sol.set_bounds(*inp.bounds[0])
        sol.set_input_cost(np.asarray(inp.prob["R"], np.float32).ravel())
        sol.set_coeff_d2p(np.full((nx, nu), 0.01, np.float32))
        sol.set_uref(np.zeros((N - 1, nu), np.float32))
        sol.set_x0(inp.x0)
        cur = dict(BASE)
        for key in (plan(cls, spec["full"], accepted) if rows is None else rows):
            cfg, fails = cfg_of(key), []
            if cfg["k"] != cur["k"]:
                _try(fails, "set_row_kernel", sol.set_row_kernel, cfg["k"])
            if cfg["o"] != cur["o"]:
                _try(fails, "set_optional_terms", sol.set_optional_terms, cfg["o"] == 1, cfg["o"] == 2)
            if cfg["p"] != cur["p"]:
                _try(fails, "set_models", sol.set_models, inp.models) if cfg["p"] else _try(fails, "clear_models", sol.clear_models)
            if cfg["b"] != cur["b"]:
                _try(fails, "set_bounds", sol.set_bounds, *inp.bounds[cfg["b"]])
            if cfg["x"] != cur["x"]:
                assert cfg["x"] != 0, "a reference cannot be withdrawn: x = 0 rows come first"
                if cfg["x"] == 1:
                    _try(fails, "set_xref", sol.set_xref, inp.xref_shared)
                elif cfg["x"] == 2:
                    _try(fails, "set_xref", sol.set_xref, inp.xref_inst)
                else:
                    _try(fails, "set_xref_window", sol.set_xref_window, inp.tables[cfg["x"] - 3], inp.start)
            if cfg["d"] != cur["d"]:
                _try(fails, "set_dispatch", sol.set_dispatch, cfg["d"])
            if cfg["c"] != cur["c"]:
                _try(fails, "set_dispatch_order_device", sol.set_dispatch_order_device, order_ptr if cfg["c"] else None)
            if cfg["m"] != cur["m"]:
                _try(fails, "set_settings", sol.set_settings, **{**sol.settings, "max_iter": MAX_ITER[cfg["m"]]})
            _try(fails, "select_kernel", sol.select_kernel, cfg["v"])
            cur = cfg
            if cfg["w"]:
                sol.reset_workspace()
                sol.set_x0(inp.x0)
            f = []
            arith = sol.arithmetic() if _try(f, "arithmetic", sol.arithmetic) else f[0][1]
            names = [sol.kernel_name(), sol.closed_loop_kernel_name(), arith, fails]
            ops = None
            if spec["solves"]:
                ops = []

                def op(fn, *a):
                    f = []
                    if _try(f, "op", fn, *a):
                        sol.synchronize()
                        ops.append([sol.dispatch_applied(), zlib.crc32(sol.get_status()[0].tobytes())])
                    else:
                        ops.append(f[0][1])
                op(sol.solve)
                op(sol.solve)
                op(sol.mpc_run_async, 3)
                if cfg["w"] and spec["batch"] != SMALL:
                    sol.reset_workspace()
                    sol.set_x0(inp.x0)
                    op(sol.mpc_run_async, 3)
                ops.append(int(sol.lib.tiny_batch_debug_graph_captures(sol._h)))
            rec["rows"].append([key, names, ops])
    finally:
        sol.close()
    return rec


def find_long_rows(T) -> int:
    """the shortest table, doubling from SHORT_ROWS, on which a forced tile16 gives way to another kernel (the limit is internal to the library)"""
    pr = T.problems
    prob = pr.quadrotor(20, 30)
    sol = T.TinyBatchSolver(prob, SMALL)
    sol.set_bounds(*pr.bounds_arrays(prob))
    sol.set_row_kernel(5)
    rows = SHORT_ROWS
    try:
        while True:
            sol.set_xref_window(np.zeros((rows, 12), np.float32), np.zeros(SMALL, np.int32))
            if not sol.kernel_name().startswith("tile16"):
                return rows
            assert rows == SHORT_ROWS or rows < 1 << 16, "tile16 never gives way"
            rows *= 2
    finally:
        sol.close()


class Session:
    """GPU-side state shared by the handles of one recording or replay: the CU count, a caller's dispatch order, inputs per (class, batch).
    The device is reached through the HIP runtime the library itself links (solver._hip), not through a framework that brings its own."""

    def __init__(self, long_rows=None):
        import ctypes
        import accelerated_tinympc_amd as T
        from accelerated_tinympc_amd import solver
        self.T, self._C, self._hip = T, ctypes, solver._hip()
        T.load_library()
        n = ctypes.c_int(0)
        rc = self._hip.hipDeviceGetAttribute(ctypes.byref(n), 63, 0)  # hipDeviceAttributeMultiprocessorCount
        assert rc == 0 and 0 < n.value <= 1024, (rc, n.value)
        self.cu = n.value
        self.long_rows = long_rows or find_long_rows(T)
        self._order = (0, None)
        self._inp = (None, None)

    def run(self, spec, rows=None):
        key = (tuple(spec["cls"]), spec["batch"])
        if self._inp[0] != key:
            self._inp = (key, Inputs(self.T, spec["cls"], spec["batch"], self.long_rows))
        groups = (spec["batch"] + 3) // 4
        if self._order[0] != groups:  # a permutation of the groups: last first
            if self._order[1]:
                self._hip.hipFree(self._order[1])
            host, ptr = np.arange(groups - 1, -1, -1, dtype=np.int32), self._C.c_void_p()
            assert self._hip.hipMalloc(self._C.byref(ptr), host.nbytes) == 0 and self._hip.hipMemcpy(ptr, host.ctypes.data, host.nbytes, 1) == 0
            self._order = (groups, ptr)
        return run_handle(self.T, spec, self._inp[1], self._order[1].value, rows)


# ---- the committed form: names and solve records interned, one short list per row -------------------------------------------------
def pack(cu, long_rows, specs, recs) -> dict:
    names, ops, ni, oi = [], [], {}, {}

    def intern(tab, idx, v):
        s = json.dumps(v)
        if s not in idx:
            idx[s] = len(tab)
            tab.append(v)
        return idx[s]
    handles = []
    for spec, rec in zip(specs, recs):
        rows = [[key, intern(names, ni, nm)] + ([] if op is None else [intern(ops, oi, op)]) for key, nm, op in rec["rows"]]
        handles.append({**spec, "storage_refused": rec["storage_refused"], "row_kernels_refused": rec["row_kernels_refused"], "rows": rows})
    return dict(cu=cu, long_rows=long_rows, keys=KEYS, names=names, ops=ops, handles=handles)


def unpack_rows(table: dict, h: dict) -> list:
    return [[r[0], table["names"][r[1]], table["ops"][r[2]] if len(r) > 2 else None] for r in h["rows"]]


def spec_of(h: dict) -> dict:
    return {k: h[k] for k in ("cls", "batch", "storage", "full", "solves")}


# On disk the table is two fixtures: PATH (.json, readable: the device, the handles with their refusals and row counts, every distinct set of
# names and refusal texts, one per line) and, beside it, PATH's stem + "_rows.json.gz" (the rows and the distinct solve records: nine thousand
# lines of digits nobody reads; --dump prints them).  The readable half carries the other's sha256.
def rows_path(path: Path) -> Path:
    return path.with_name(path.stem + "_rows.json.gz")


def save_table(table: dict, path: Path):
    import gzip
    import hashlib
    body = json.dumps(dict(ops=table["ops"], rows=[h["rows"] for h in table["handles"]]), separators=(",", ":")).encode()
    blob = gzip.compress(body, 9, mtime=0)
    head = {k: v for k, v in table.items() if k not in ("ops", "handles")}
    head["rows_sha256"] = hashlib.sha256(blob).hexdigest()
    head["handles"] = [{**{k: v for k, v in h.items() if k != "rows"}, "n_rows": len(h["rows"])} for h in table["handles"]]
    item = lambda v: "[\n  " + ",\n  ".join(json.dumps(e) for e in v) + "\n ]" if isinstance(v, list) else json.dumps(v)
    path.parent.mkdir(parents=True, exist_ok=True)
    rows_path(path).write_bytes(blob)
    path.write_text("{\n" + ",\n".join(f" {json.dumps(k)}: {item(v)}" for k, v in head.items()) + "\n}\n")


def load_table(path: Path) -> dict:
    import gzip
    import hashlib
    table, blob = json.loads(path.read_text()), rows_path(path).read_bytes()
    assert hashlib.sha256(blob).hexdigest() == table["rows_sha256"], f"{rows_path(path).name} is not the one {path.name} was written with"
    body = json.loads(gzip.decompress(blob))
    table["ops"] = body["ops"]
    for h, rows in zip(table["handles"], body["rows"]):
        assert len(rows) == h.pop("n_rows")
        h["rows"] = rows
    return table


# ---- coverage the thinning must keep -----------------------------------------------------------------------------------------------
# one distinctive piece of every refusal of the variant resolution.  "no streaming kernel instantiation" is left out: tiny_batch_create accepts a
# class only if the streaming kernel's padded instantiations hold it (nx <= 64, nu <= 32) or a row / wave class does, and every one of those fits too
REFUSALS = ["are implemented for fp32 storage only", "terms are not implemented with per-instance models", "holds one gain matrix for the whole launch",
            "per-instance models need the unrolled 16-lane kernel", "with per-instance models the row variants run on the unrolled 16-lane kernel only",
            "keeps one gain table for the whole launch", "(variant 4) needs nx, nu each <= 4 or a multiple of 4 (nx=", "needs the state-on-chip wave kernel",
            "has no exact-arithmetic kernel", "fp32 storage and no optional terms", "are implemented by the row kernels for nx + nu <= 16 only",
            "no row kernel instantiation", "fp16 storage is implemented by the row kernels only (nx + nu <= 16)"]
FAMILIES = ["rowlane", "rowloop", "rowstream", "wavestream", "quadlane", "tile16", "waveres", "tile48", "stream", "generic"]


def check_coverage(table: dict):
    texts, fams, rows = [], set(), []
    for h in table["handles"]:
        for key, (kn, cl, arith, fails), ops in unpack_rows(table, h):
            fams.update((kn.split("<")[0], cl.split("<")[0]))
            texts += [t for _, t in fails] + ([arith] if arith not in ("exact", "fma") else []) + [o for o in (ops or [])[:-1] if isinstance(o, str)]
            if ops and all(isinstance(o, list) for o in ops[:-1]):
                rows.append((cfg_of(key), kn, cl, [o[0] for o in ops[:-1]]))
    missing = [f for f in FAMILIES if f not in fams] + [r for r in REFUSALS if not any(r in t for t in texts)]
    assert not missing, f"not hit by any row: {missing}"
    onchip = lambda cl: cl.split("<")[0] in ("rowlane", "tile16")
    hit = {
        "a: a run from a reset workspace takes the predictor under automatic dispatch": any(c["d"] == -1 and c["w"] and onchip(cl) and len(d) == 4 and d[3] == 1 for c, kn, cl, d in rows),
        "a: a lone cold solve takes it too": any(c["d"] == -1 and c["w"] and d[0] == 1 for c, kn, cl, d in rows),
        "b: a warm run is ordered by history": any(c["d"] == -1 and onchip(cl) and d[2] == 3 for c, kn, cl, d in rows),
        "c: tile16 in a run, history order": any(cl.startswith("tile16") and d[2] == 3 for c, kn, cl, d in rows),
        "c: tile16 in a lone solve, history order": any(kn.startswith("tile16") and d[1] == 3 for c, kn, cl, d in rows),
        "d: rowloop is ordered in a lone solve": any(kn.startswith("rowloop") and d[0] in (1, 3) for c, kn, cl, d in rows),
        "e: max_iter 1 keeps a lone solve in index order, not a run": any(c["m"] == 1 and c["d"] in (-1, 2) and onchip(cl) and d[1] == 0 and d[2] == 3 for c, kn, cl, d in rows),
        "e: max_iter 1 drops the predictor of a run": any(c["m"] == 1 and c["d"] == 1 and onchip(cl) and d[2] == 0 for c, kn, cl, d in rows),
        "f: tile16 drops a caller's order": any(c["c"] and kn.startswith("tile16") and cl.startswith("tile16") and 2 not in d for c, kn, cl, d in rows),
        "f: the 16-lane kernel follows it": any(c["c"] and kn.startswith("rowlane") and 2 in d for c, kn, cl, d in rows),
    }
    assert all(hit.values()), f"dispatch differences not hit: {[k for k, v in hit.items() if not v]}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    ap.add_argument("--dump", metavar="JSON", help="print every row of a table in full, one per line (no GPU)")
    a = ap.parse_args()
    t0 = time.time()
    if a.write:
        ses = Session()
        specs = handle_specs(ses.cu)
        recs = []
        for spec in specs:
            t = time.time()
            recs.append(ses.run(spec))
            print(f"{spec['cls']} B={spec['batch']} storage={spec['storage']}: {len(recs[-1]['rows'])} rows, {time.time() - t:.1f} s", flush=True)
        table = pack(ses.cu, ses.long_rows, specs, recs)
        save_table(table, Path(a.write))
        print(f"{sum(len(h['rows']) for h in table['handles'])} rows, {len(table['names'])} distinct names, {len(table['ops'])} distinct solve records, "
              f"{Path(a.write).stat().st_size} + {rows_path(Path(a.write)).stat().st_size} bytes, {time.time() - t0:.0f} s; long table: {ses.long_rows} rows", flush=True)
        check_coverage(table)
        print("coverage ok")
    if a.dump:
        table = load_table(Path(a.dump))
        for h in table["handles"]:
            for row in unpack_rows(table, h):
                print(json.dumps([h["cls"], h["batch"], h["storage"]] + row))
    if a.check:
        table = load_table(Path(a.check))
        ses = Session(table["long_rows"])
        assert ses.cu == table["cu"], f"the table was recorded on {table['cu']} CUs, this device has {ses.cu}"
        bad = 0
        for h in table["handles"]:
            want = unpack_rows(table, h)
            got = ses.run(spec_of(h), [r[0] for r in want])
            diffs = [(w, g) for w, g in zip(want, got["rows"]) if w != g]
            diffs += [("refusals", k) for k in ("storage_refused", "row_kernels_refused") if got[k] != h[k]]
            bad += len(diffs)
            print(f"{h['cls']} B={h['batch']} storage={h['storage']}: {len(want)} rows, {len(diffs)} differ", flush=True)
            for w, g in diffs[:3]:
                print("   recorded", w, "\n   now     ", g)
        print(f"{bad} differences, {time.time() - t0:.0f} s")
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
