"""Static figures of the simulated closed loop's kernels (admm_rowsim.hip: the SIM instantiations of the 16-lane kernel's body in a translation unit of
their own, which the scans of tests/test_isa.py do not see).  CPU test: hipcc cross-compiles, no GPU needed."""
import re

import pytest

import accelerated_tinympc_amd as T
from isa_tools import hazards, kernels_of, scratch_sizes

ROWLANE = [(12, 4, 30), (12, 4, 25), (12, 4, 20), (12, 4, 10), (4, 1, 10), (8, 3, 7), (12, 4, 40), (12, 4, 50)]
# admm_rowsim_kernel / admm_rowsim_pm_kernel <NX, NU, N, EXACT>: bytes of scratch per lane as built; every instantiation not listed has none.  The MPC
# twins in admm_rowlane.hip have 80 / 84 (exact, N = 30) and 72 / 68 (fma, N = 50): three of the four carry 12 - 16 bytes more, around the plant step
# between two solves (once per MPC step, outside the iteration loop)
SIM_SCRATCH = {("", 12, 4, 30, 1): 92, ("_pm", 12, 4, 30, 1): 96, ("", 12, 4, 50, 0): 72, ("_pm", 12, 4, 50, 0): 84}


@pytest.fixture(scope="module")
def rowsim():
    return T.build.device_asm("admm_rowsim.hip").read_text()


def test_the_unit_holds_the_sim_instantiations_and_nothing_else(rowsim):
    names = list(kernels_of(rowsim))
    assert len(names) == 32 and all("admm_rowsim_kernel" in n or "admm_rowsim_pm_kernel" in n for n in names), names
    assert not any("admm_rowlane_kernel" in n or "admm_rowlane_pm_kernel" in n for n in names)


def test_every_sim_instantiation_has_its_scratch_pinned(rowsim):
    sizes = scratch_sizes(rowsim)
    seen = 0
    for nx, nu, n in ROWLANE:
        for ex in (1, 0):
            for pm in ("", "_pm"):
                key = f"admm_rowsim{pm}_kernelILi{nx}ELi{nu}ELi{n}ELb{ex}EEEv"
                got = [v for k, v in sizes.items() if key in k]
                assert len(got) == 1, key
                pin = SIM_SCRATCH.get((pm, nx, nu, n, ex), 0)
                assert got[0] <= pin, f"{key}: {got[0]} bytes of scratch per lane, pinned at {pin}"
                seen += 1
    assert seen == len(sizes) == 32


def test_sim_kernels_are_free_of_dpp_hazards_and_packed_adds(rowsim):
    ks = kernels_of(rowsim)
    assert len(ks) == 32
    for n, lines in ks.items():
        assert not hazards(lines), (n, hazards(lines)[:3])
        assert not any(i.startswith("v_pk_add_f32") for i in lines), n


def test_sim_kernels_keep_the_occupancy_of_their_twins(rowsim):
    """two waves per SIMD (256 registers) wherever the MPC twin has them: every instantiation but exact arithmetic with N > 32"""
    for name in kernels_of(rowsim):
        n, ex = (int(v) for v in re.search(r"kernelILi\d+ELi\d+ELi(\d+)ELb([01])E", name).groups())
        vgprs = int(re.search(r"; TotalNumVgprs: (\d+)", rowsim[re.search(rf"^{name}:", rowsim, re.M).start():]).group(1))
        assert vgprs <= (512 if n > 32 and ex else 256), (name, vgprs)
