"""Static figures of the per-instance-settings kernels (admm_rowlane_ps.hip: the PS instantiations of the 16-lane kernel's body; admm_steps_ps.hip: the
streaming row kernel and the step kernel compiled with the settings view on the instance's record), translation units of their own, which the scans of
tests/test_isa.py do not see.  CPU test: hipcc cross-compiles, no GPU needed."""
import re

import pytest

import accelerated_tinympc_amd as T
from isa_tools import hazards, kernels_of, scratch_sizes

ROWLANE = [(12, 4, 30), (12, 4, 25), (12, 4, 20), (12, 4, 10), (4, 1, 10), (8, 3, 7), (12, 4, 40), (12, 4, 50)]
ROWDIMS = [(12, 4), (4, 1), (8, 3), (8, 4), (12, 2), (4, 2), (4, 4), (2, 2)]
# admm_rowlane_ps_kernel <NX, NU, N, EXACT, MPC, BPI>: bytes of scratch per lane as built; every instantiation not listed has none.  Beside each, its twin
# without per-instance settings in admm_rowlane.hip (admm_rowlane_kernel <.., H16 = 0, MPC, BPI, D32 = 0, OPT = 0>): the four settings registers are
# carried across the iteration loop, which the kernels that already spill pay in scratch
# (24 - 28 bytes each: the record's four values and what the per-row modulo and budget compares keep beside them)
#                   one solve                        per-instance bounds              the on-chip closed loop
PS_SCRATCH = {(12, 4, 30, 1, 0, 0): 84, (12, 4, 30, 1, 0, 1): 76, (12, 4, 30, 1, 1, 0): 104,     # exact arithmetic, N = 30
              (12, 4, 50, 0, 0, 0): 68, (12, 4, 50, 0, 0, 1): 212, (12, 4, 50, 0, 1, 0): 108}    # fma arithmetic, N = 50
TWIN_SCRATCH = {(12, 4, 30, 1, 0, 0): 60, (12, 4, 30, 1, 0, 1): 52, (12, 4, 30, 1, 1, 0): 80,
                (12, 4, 50, 0, 0, 0): 40, (12, 4, 50, 0, 0, 1): 192, (12, 4, 50, 0, 1, 0): 80}


@pytest.fixture(scope="module")
def rowlane_ps():
    return T.build.device_asm("admm_rowlane_ps.hip").read_text()


@pytest.fixture(scope="module")
def steps_ps():
    return T.build.device_asm("admm_steps_ps.hip").read_text()


def test_the_units_hold_the_ps_kernels_and_nothing_else(rowlane_ps, steps_ps):
    names = list(kernels_of(rowlane_ps))
    assert len(names) == len(ROWLANE) * 2 * 3 == 48 and all("admm_rowlane_ps_kernel" in n for n in names), names
    names = list(kernels_of(steps_ps))
    stream, step = [n for n in names if "admm_rowstream_ps_kernel" in n], [n for n in names if "admm_step_ps_kernel" in n]
    assert len(stream) == len(step) == len(ROWDIMS) * 4 == 32 and len(names) == 64, names


def test_every_ps_instantiation_has_its_scratch_pinned(rowlane_ps, steps_ps):
    sizes = scratch_sizes(rowlane_ps)
    seen = 0
    for nx, nu, n in ROWLANE:
        for ex in (1, 0):
            for mpc, bpi in ((0, 0), (0, 1), (1, 0)):
                key = f"admm_rowlane_ps_kernelILi{nx}ELi{nu}ELi{n}ELb{ex}ELb{mpc}ELb{bpi}EEEv"
                got = [v for k, v in sizes.items() if key in k]
                assert len(got) == 1, key
                pin = PS_SCRATCH.get((nx, nu, n, ex, mpc, bpi), 0)
                assert got[0] <= pin, f"{key}: {got[0]} bytes of scratch per lane, pinned at {pin}"
                seen += 1
    assert seen == len(sizes) == 48
    assert all(v == 0 for v in scratch_sizes(steps_ps).values()), "the streaming and step kernels spill nothing, like their twins"


def test_the_twins_scratch_is_what_the_pins_are_compared_with():
    sizes = scratch_sizes(T.build.device_asm("admm_rowlane.hip").read_text())
    for (nx, nu, n, ex, mpc, bpi), pin in TWIN_SCRATCH.items():
        key = f"admm_rowlane_kernelILi{nx}ELi{nu}ELi{n}ELb{ex}ELb0ELb{mpc}ELb{bpi}ELb0ELb0EEEv"
        got = [v for k, v in sizes.items() if key in k]
        assert got == [pin], (key, got, pin)


def test_ps_kernels_are_free_of_dpp_hazards_and_packed_adds(rowlane_ps, steps_ps):
    for txt, n_kernels in ((rowlane_ps, 48), (steps_ps, 64)):
        ks = kernels_of(txt)
        assert len(ks) == n_kernels
        for n, lines in ks.items():
            assert not hazards(lines), (n, hazards(lines)[:3])
            assert not any(i.startswith("v_pk_add_f32") for i in lines), n


def test_ps_kernels_keep_the_occupancy_of_their_twins(rowlane_ps):
    """two waves per SIMD (256 registers) wherever the twin has them: every instantiation but exact arithmetic with N > 32"""
    for name in kernels_of(rowlane_ps):
        n, ex = (int(v) for v in re.search(r"kernelILi\d+ELi\d+ELi(\d+)ELb([01])E", name).groups())
        vgprs = int(re.search(r"; TotalNumVgprs: (\d+)", rowlane_ps[re.search(rf"^{name}:", rowlane_ps, re.M).start():]).group(1))
        assert vgprs <= (512 if n > 32 and ex else 256), (name, vgprs)
