"""The standing record of the library's device code and the routing of kernel names to translation units.  CPU test: hipcc cross-compiles, no GPU
needed.

tests/golden/device_code.json holds, per unit of build.UNITS, the hash of its machine code, its kernel count, its instruction lines and a
fingerprint of its instruction streams (tools/device_code.py --write).  A change that means to leave the device code alone passes as it is; a
change that means to move a unit regenerates the record and names the moved units in its description.  tests/golden/kernel_units.json holds
kernel name -> unit as build.kernel_isa_sha routed the names before build.UNITS replaced its chain of conditions."""
import json
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import device_code, moved_units

GOLDEN = Path(__file__).resolve().parent / "golden"
RECORD = json.loads((GOLDEN / "device_code.json").read_text())
KERNEL_UNITS = json.loads((GOLDEN / "kernel_units.json").read_text())


def test_the_record_has_a_row_for_every_unit():
    assert list(RECORD["units"]) == T.build.SOURCES == [u.source for u in T.build.UNITS]


def test_every_unit_builds_to_its_recorded_device_code():
    T.build.build()
    built = device_code(T.build)
    moved = moved_units(RECORD, built)
    detail = "\n".join(f"  {u}: recorded {RECORD['units'].get(u)}, built {built['units'].get(u)}" for u in moved)
    version = "" if built["hipcc"] == RECORD["hipcc"] else f"\nthe record was written under '{RECORD['hipcc']}', this build ran under '{built['hipcc']}'"
    assert not moved, (f"the device code of {', '.join(moved)} moved:\n{detail}{version}\na pull request that means to move them runs "
                       f"`python tools/device_code.py --write` and names these units in its description; any other leaves the record alone")


def test_the_units_with_device_code_all_hash_differently():
    shas = [r["isa_sha"] for r in RECORD["units"].values() if r["isa_sha"]]
    assert len(shas) == len(set(shas)) == sum(1 for r in RECORD["units"].values() if r["kernels"])


def test_the_helper_units_hold_the_kernels_their_fingerprints_count():
    """the counts inside F32_FINGERPRINT / F64_FINGERPRINT of tests/test_isa_helpers.py"""
    units = RECORD["units"]
    assert (units["batch_helpers.hip"]["kernels"], units["batch_helpers.hip"]["instructions"]) == (15, 11783)
    assert (units["batch64_helpers.hip"]["kernels"], units["batch64_helpers.hip"]["instructions"]) == (3, 1217)


@pytest.mark.parametrize("name", list(KERNEL_UNITS))
def test_a_kernel_name_is_routed_to_its_unit(name):
    assert T.build.unit_of(name) == KERNEL_UNITS[name]
