"""The standing record of the library's device code, tests/golden/device_code.json: one row per translation unit of build.UNITS with the hash of
its machine code (build.device_isa_sha), its kernel count, its instruction lines and a fingerprint of its instruction streams.  CPU only: hipcc
cross-compiles, nothing here opens a GPU.

    python tools/device_code.py --write           regenerate the record from this tree (a change that means to move a unit)
    python tools/device_code.py --check           compare the record with this tree, print the rows that differ
    python tools/device_code.py --write --added   the same two for the units of build.ADDED_UNITS, which arrived after the standing record was written
    python tools/device_code.py --check --added   and are recorded beside it in tests/golden/device_code_added.json
    python tools/device_code.py --against LIB     LIB = accelerated-tinympc_amd/lib of another checkout (built): the parent / new table of
                                                  profiles/*_isa.txt, and for every moved unit the kernels that differ
"""
import argparse
import importlib.util
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import accelerated_tinympc_amd as T  # noqa: E402
from isa_tools import device_code, kernels_of, moved_units  # noqa: E402

RECORD = ROOT / "tests" / "golden" / "device_code.json"
ADDED_RECORD = RECORD.with_name("device_code_added.json")   # the units of build.ADDED_UNITS


def registers(listing: str) -> dict:
    """{mangled name: (NumVgprs, NumAgprs, ScratchSize)} of every kernel of a listing"""
    out = {}
    for name in kernels_of(listing):
        tail = listing[re.search(rf"^{name}:", listing, re.M).start():]
        out[name] = tuple(int(re.search(rf"^; {k}: (\d+)", tail, re.M).group(1)) for k in ("NumVgprs", "NumAgprs", "ScratchSize"))
    return out


def against(lib: Path) -> None:
    spec = importlib.util.spec_from_file_location("parent_build", lib.parent / "build.py")   # the other tree's own units, flags and objects
    parent = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = parent
    spec.loader.exec_module(parent)
    assert parent.LIB.parent == lib.resolve(), (parent.LIB.parent, lib)
    T.build.build()

    def sha(build, unit):
        try:
            return build.device_isa_sha(unit)
        except KeyError:
            return None
    linked = lambda b: getattr(b, 'LINKED_SOURCES', b.SOURCES)
    for unit in dict.fromkeys([*linked(parent), *linked(T.build)]):
        old = sha(parent, unit) if unit in linked(parent) else "(new unit)"
        new = sha(T.build, unit) if unit in linked(T.build) else "(removed)"
        if old is None and new is None:
            print(f"{unit:28s} no device code (host only), parent and new")
            continue
        verdict = "" if "(" in f"{old}{new}" else "same" if old == new else "moved"
        print(f"{unit:28s} {old!s:16s} {new!s:16s} {verdict}".rstrip())
        if verdict != "moved":
            continue
        a, b = parent.device_asm(unit).read_text(), T.build.device_asm(unit).read_text()
        ka, kb, ra, rb = kernels_of(a), kernels_of(b), registers(a), registers(b)
        print(f"    kernels {len(ka)} -> {len(kb)}")
        for name in sorted({*ka, *kb}):
            if name not in ka or name not in kb:
                print(f"    {name}: only in the {'new' if name in kb else 'parent'} tree")
                continue
            unnumbered = [[re.sub(r"\.LBB\d+_", ".LBB_", ln) for ln in k[name]] for k in (ka, kb)]
            if ra[name] != rb[name] or unnumbered[0] != unnumbered[1]:
                print(f"    {name}: (VGPRs, AGPRs, scratch) {ra[name]} -> {rb[name]}, instructions {len(ka[name])} -> {len(kb[name])}"
                      f"{'' if unnumbered[0] != unnumbered[1] else ' (the same stream)'}")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--write", action="store_true")
    mode.add_argument("--check", action="store_true")
    mode.add_argument("--against", type=Path, metavar="LIB")
    ap.add_argument("--added", action="store_true", help="the units of build.ADDED_UNITS and their record, tests/golden/device_code_added.json")
    args = ap.parse_args()
    if args.against:
        against(args.against)
        return 0
    T.build.build()
    path, units = (ADDED_RECORD, T.build.ADDED) if args.added else (RECORD, T.build)
    now = device_code(units)
    if args.write:
        rows = ",\n".join(f"  {json.dumps(u)}: {json.dumps(r)}" for u, r in now["units"].items())   # a row a line: a moved unit is one line of the diff
        path.write_text(f'{{\n "hipcc": {json.dumps(now["hipcc"])},\n "units": {{\n{rows}\n }}\n}}\n')
        print(f"wrote {path.relative_to(ROOT)}: {len(now['units'])} units, {sum(r['kernels'] for r in now['units'].values())} kernels")
        return 0
    record = json.loads(path.read_text())
    diff = moved_units(record, now)
    for u in diff:
        print(f"{u}: recorded {record['units'].get(u)}, built {now['units'].get(u)}")
    if diff and record["hipcc"] != now["hipcc"]:
        print(f"(recorded under '{record['hipcc']}', this is '{now['hipcc']}')")
    print(f"{len(diff)} of {len(now['units'])} units differ from {path.relative_to(ROOT)}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
