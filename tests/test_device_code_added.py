"""The record of the device code of the units that arrived after tests/golden/device_code.json was written (build.ADDED_UNITS: admm_wave_ps.hip and
admm_waveres_ps.hip, the wave kernels under per-instance settings), and the routing of their kernel names.  CPU test: hipcc cross-compiles, no GPU needed.

The standing record has exactly the rows of build.UNITS and tests/test_device_code.py holds it there; these units are built and linked like the others and
are recorded the same way — hash of the machine code, kernel count, instruction lines, fingerprint of the instruction streams, by the same readers
(isa_tools.device_code) — in tests/golden/device_code_added.json (`python tools/device_code.py --write --added`).  tests/golden/kernel_units_added.json
holds kernel name -> unit for the names tiny_batch_kernel_name() gives them."""
import json
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import device_code, moved_units

GOLDEN = Path(__file__).resolve().parent / "golden"
RECORD = json.loads((GOLDEN / "device_code_added.json").read_text())
STANDING = json.loads((GOLDEN / "device_code.json").read_text())
KERNEL_UNITS = json.loads((GOLDEN / "kernel_units_added.json").read_text())
OLD_KERNEL_UNITS = json.loads((GOLDEN / "kernel_units.json").read_text())


def test_the_record_has_a_row_for_every_added_unit_and_the_two_records_cover_the_library():
    b = T.build
    assert list(RECORD["units"]) == b.ADDED_SOURCES == [u.source for u in b.ADDED_UNITS] == ["admm_wave_ps.hip", "admm_waveres_ps.hip"]
    assert not set(RECORD["units"]) & set(STANDING["units"])
    assert b.ALL_UNITS == b.UNITS + b.ADDED_UNITS and b.LINKED_SOURCES == [u.source for u in b.ALL_UNITS]
    # everything that is compiled and linked has a row in one of the two records
    assert [src.name for src, _ in b._objs()] == [*STANDING["units"], *RECORD["units"]]


def test_every_added_unit_builds_to_its_recorded_device_code():
    T.build.build()
    built = device_code(T.build.ADDED)
    moved = moved_units(RECORD, built)
    detail = "\n".join(f"  {u}: recorded {RECORD['units'].get(u)}, built {built['units'].get(u)}" for u in moved)
    version = "" if built["hipcc"] == RECORD["hipcc"] else f"\nthe record was written under '{RECORD['hipcc']}', this build ran under '{built['hipcc']}'"
    assert not moved, (f"the device code of {', '.join(moved)} moved:\n{detail}{version}\na pull request that means to move them runs "
                       f"`python tools/device_code.py --write --added` and names these units in its description; any other leaves the record alone")


def test_the_added_units_hold_device_code_that_no_other_unit_holds():
    shas = [r["isa_sha"] for r in RECORD["units"].values()]
    assert all(shas) and len(set(shas)) == len(shas) and all(r["kernels"] == 10 for r in RECORD["units"].values())
    assert not set(shas) & {r["isa_sha"] for r in STANDING["units"].values()}


def test_an_added_unit_is_a_variant_of_its_pm_sibling_s_parent():
    b = T.build
    for unit, sibling in (("admm_wave_ps.hip", "admm_wave_pm.hip"), ("admm_waveres_ps.hip", "admm_waveres_pm.hip")):
        assert b.INCLUDED_SOURCES[unit] == b.INCLUDED_SOURCES[sibling]
        assert b.EXTRA_FLAGS.get(unit, []) == b.EXTRA_FLAGS.get(sibling, []) == b.EXTRA_FLAGS.get(b.INCLUDED_SOURCES[unit][0], [])


@pytest.mark.parametrize("name", list(KERNEL_UNITS))
def test_a_ps_kernel_name_is_routed_to_its_unit(name):
    assert T.build.unit_of(name) == KERNEL_UNITS[name]
    assert T.build.kernel_isa_sha(name) == RECORD["units"][KERNEL_UNITS[name]]["isa_sha"]


@pytest.mark.parametrize("name", [n for n in OLD_KERNEL_UNITS if n.startswith("wave")])
def test_the_other_wave_names_keep_their_units(name):
    assert T.build.unit_of(name) == OLD_KERNEL_UNITS[name]
