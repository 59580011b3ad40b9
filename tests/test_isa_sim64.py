"""Static figures of the fp64 simulated closed loop's kernels (tinympc_batch64_sim.hip: the SIM instantiations of admm_f64_rows_kernel in a
translation unit of their own) beside their MPC twins in tinympc_batch64.hip, read from the `hipcc -S` listings (build.device_asm), and the machine
code of tinympc_batch64.hip itself, which the feature must not move.  CPU test: hipcc cross-compiles, no GPU needed."""
import re
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from test_isa import kernels_of

# device_isa_sha("tinympc_batch64.hip") of the commit before the simulated loop ("Closed loop against a separate plant, with disturbances")
PARENT_ISA_SHA = "0d7d1b9fbe03a3f9"
# (NX, NU, N or capacity, RT): (VGPRs, AGPRs, bytes of scratch per lane) of the SIM instantiation as built, and of its MPC twin
SIM = {(12, 4, 10, 0): (256, 0, 508), (12, 4, 30, 0): (256, 256, 708), (12, 4, 20, 0): (256, 256, 388), (4, 1, 10, 0): (256, 0, 0), (8, 4, 9, 0): (256, 0, 144),
       (12, 4, 32, 1): (256, 256, 160), (4, 1, 32, 1): (256, 210, 0), (8, 4, 32, 1): (256, 248, 0), (12, 2, 32, 1): (256, 256, 76), (4, 2, 32, 1): (256, 214, 0),
       (4, 4, 32, 1): (256, 222, 0)}
MPC = {(12, 4, 10, 0): (256, 0, 440), (12, 4, 30, 0): (256, 256, 644), (12, 4, 20, 0): (256, 256, 332), (4, 1, 10, 0): (256, 0, 24), (8, 4, 9, 0): (256, 0, 136),
       (12, 4, 32, 1): (256, 256, 264), (4, 1, 32, 1): (256, 212, 0), (8, 4, 32, 1): (256, 256, 48), (12, 2, 32, 1): (256, 256, 164), (4, 2, 32, 1): (256, 216, 0),
       (4, 4, 32, 1): (256, 228, 0)}


def figures(listing, want_sim):
    """{(NX, NU, N, RT): (VGPRs, AGPRs, scratch, waves per SIMD)} of the closed-loop instantiations of admm_f64_rows_kernel in a listing"""
    out = {}
    for m in re.finditer(r"^(_Z\w*admm_f64_rows_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb1E\w*):", listing, re.M):
        if ("Sim64" in m.group(1)) != want_sim:
            continue
        tail = listing[m.start():]
        g = lambda k: int(re.search(rf"^; {k}: (\d+)", tail, re.M).group(1))
        out[tuple(int(v) for v in m.groups()[1:])] = (g("NumVgprs"), g("NumAgprs"), g("ScratchSize"), g("Occupancy"))
    return out


@pytest.fixture(scope="module")
def sim_listing():
    return T.build.device_asm("tinympc_batch64_sim.hip").read_text()


@pytest.fixture(scope="module")
def main_listing():
    return T.build.device_asm("tinympc_batch64.hip").read_text()


def test_the_unit_holds_the_sim_instantiations_and_the_plant_kernel(sim_listing):
    names = list(kernels_of(sim_listing))
    rows = [n for n in names if "admm_f64_rows_kernel" in n]
    plant = [n for n in names if "plant64_sim_kernel" in n]
    assert len(rows) == 11 and all("Mpc64" in n and "Sim64" in n for n in rows), rows
    assert len(plant) == 7 and len(names) == 18, names      # one plant kernel per class of TINY_FOR_EACH_F64DIMS, nothing else


def test_every_mpc_instantiation_has_a_sim_twin_at_its_occupancy(sim_listing, main_listing):
    sim, mpc = figures(sim_listing, True), figures(main_listing, False)
    assert set(sim) == set(mpc) == set(SIM) == set(MPC)
    for key in sim:
        assert sim[key][3] == mpc[key][3] == (2 if key[2] <= 12 else 1), (key, sim[key], mpc[key])


def test_register_and_scratch_figures_are_pinned(sim_listing, main_listing):
    sim, mpc = figures(sim_listing, True), figures(main_listing, False)
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


def test_the_fp64_unit_keeps_its_machine_code():
    """the SIM flag, the second argument struct and the new host calls leave every existing fp64 kernel as it was"""
    T.build.build()
    got = T.build.device_isa_sha("tinympc_batch64.hip")
    print(f"device_isa_sha(tinympc_batch64.hip) = {got}, the parent's = {PARENT_ISA_SHA}")
    assert got == PARENT_ISA_SHA
    assert T.build.device_isa_sha("tinympc_batch64_sim.hip") != got
    assert T.build.kernel_isa_sha("rows64<12,4,10,sim>") == T.build.device_isa_sha("tinympc_batch64_sim.hip")
    assert T.build.kernel_isa_sha("rows64<12,4,10,mpc>") == got
