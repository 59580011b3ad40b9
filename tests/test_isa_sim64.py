"""Static figures of the fp64 simulated closed loop's kernels (admm_f64_rowsim.hip: the SIM instantiations of admm_f64_rows_kernel in a
translation unit of their own) beside their MPC twins in admm_f64_rows.hip, read from the `hipcc -S` listings (build.device_asm), and the
instruction streams of every kernel of the fp64 library, pinned across its units.  CPU test: hipcc cross-compiles, no GPU needed."""
import re
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import fingerprint, kernel_key, kernels_of, loop_figures

# the fp64 library's translation units with device code: the four kernel units and the unit of the three helper kernels (the host file has none)
F64_UNITS = ("admm_f64_thread.hip", "admm_f64_rows.hip", "admm_f64_rowsim.hip", "admm_f64_plant.hip", "batch64_helpers.hip")
# fingerprint() of the library when all of it was two units (tinympc_batch64.hip, compiled a second time for the SIM instantiations): (kernels,
# instruction lines, hash).  Moving a kernel between units, or editing host code, leaves it alone; it moves when a kernel's instructions do
F64_FINGERPRINT = (112, 805134, "a42208fda02dcc37")
# (NX, NU, N or capacity, RT): (VGPRs, AGPRs, bytes of scratch per lane) of the SIM instantiation as built, and of its MPC twin
SIM = {(12, 4, 10, 0): (256, 0, 508), (12, 4, 30, 0): (256, 256, 708), (12, 4, 20, 0): (256, 256, 388), (4, 1, 10, 0): (256, 0, 0), (8, 4, 9, 0): (256, 0, 144),
       (12, 4, 32, 1): (256, 256, 160), (4, 1, 32, 1): (256, 210, 0), (8, 4, 32, 1): (256, 248, 0), (12, 2, 32, 1): (256, 256, 76), (4, 2, 32, 1): (256, 214, 0),
       (4, 4, 32, 1): (256, 222, 0)}
MPC = {(12, 4, 10, 0): (256, 0, 440), (12, 4, 30, 0): (256, 256, 644), (12, 4, 20, 0): (256, 256, 332), (4, 1, 10, 0): (256, 0, 24), (8, 4, 9, 0): (256, 0, 136),
       (12, 4, 32, 1): (256, 256, 264), (4, 1, 32, 1): (256, 212, 0), (8, 4, 32, 1): (256, 256, 48), (12, 2, 32, 1): (256, 256, 164), (4, 2, 32, 1): (256, 216, 0),
       (4, 4, 32, 1): (256, 228, 0)}


@pytest.fixture(scope="module")
def sim_listing():
    return T.build.device_asm("admm_f64_rowsim.hip").read_text()


@pytest.fixture(scope="module")
def main_listing():
    return T.build.device_asm("admm_f64_rows.hip").read_text()


def test_the_rowsim_unit_holds_the_sim_instantiations_and_nothing_else(sim_listing):
    names = list(kernels_of(sim_listing))
    assert len(names) == 11 and all("admm_f64_rows_kernel" in n and "Mpc64" in n and "Sim64" in n for n in names), names


def test_the_plant_unit_holds_the_three_plant_kernels_of_every_class():
    names = list(kernels_of(T.build.device_asm("admm_f64_plant.hip").read_text()))
    for kernel in ("plant64_kernel", "plant64_run_kernel", "plant64_sim_kernel"):  # one per class of TINY_FOR_EACH_F64DIMS
        assert sum(kernel_key(n)[0] == kernel for n in names) == 7, (kernel, names)
    assert len(names) == 21, names


def test_every_mpc_instantiation_has_a_sim_twin_at_its_occupancy(sim_listing, main_listing):
    sim, mpc = loop_figures(sim_listing, True), loop_figures(main_listing, False)
    assert set(sim) == set(mpc) == set(SIM) == set(MPC)
    for key in sim:
        assert sim[key][3] == mpc[key][3] == (2 if key[2] <= 12 else 1), (key, sim[key], mpc[key])


def test_register_and_scratch_figures_are_pinned(sim_listing, main_listing):
    sim, mpc = loop_figures(sim_listing, True), loop_figures(main_listing, False)
    for key, pin in SIM.items():
        assert sim[key][:3] == pin, f"SIM {key}: (VGPRs, AGPRs, scratch) = {sim[key][:3]}, pinned at {pin}"
    for key, pin in MPC.items():
        assert mpc[key][:3] == pin, f"MPC {key}: (VGPRs, AGPRs, scratch) = {mpc[key][:3]}, pinned at {pin}"


def test_design_records_the_figures_beside_the_twins():
    text = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    sec = text[text.index("### 5.6"):text.index("### 5.7")]
    for key, (_, ag, sc) in SIM.items():
        _, mag, msc = MPC[key]
        label = f"({key[0]},{key[1]},{'n≤32' if key[3] else key[2]})"
        assert re.search(rf"\| {re.escape(label)} \| {ag} / {sc} \| {mag} / {msc} \|", sec), f"DESIGN §5.6 has no row '{label} | {ag} / {sc} | {mag} / {msc}'"


def test_the_fp64_kernels_keep_their_instruction_streams(sim_listing, main_listing):
    """every kernel the library had as two units is found again in today's units, instruction for instruction: a unit's layout, and so its
    device_isa_sha, may move with what else it holds; a kernel's code may not"""
    got = fingerprint([sim_listing if u == "admm_f64_rowsim.hip" else main_listing if u == "admm_f64_rows.hip" else T.build.device_asm(u).read_text()
                       for u in F64_UNITS])
    print(f"fingerprint of the fp64 units = {got}, pinned at {F64_FINGERPRINT}")
    assert got == F64_FINGERPRINT
