"""Static figures of the per-instance-model kernels and the batched Riccati kernel (CPU test: hipcc cross-compiles, no GPU needed).

The DPP-hazard and v_pk_add_f32 scans of tests/test_isa.py cover admm_rowlane.hip as a whole, the per-instance instantiations included; this
file pins their scratch sizes, one by one, and the Riccati kernel's registers (per-instance models)."""
import re

import pytest

import accelerated_tinympc_amd as T
from isa_tools import hazards, kernels_of, scratch_sizes

# admm_rowlane_pm_kernel<NX, NU, N, EXACT, MPC, BPI>: bytes of scratch per lane; every instantiation not listed has none
PM_SCRATCH = {(12, 4, 30, 1, 0, 0): 64, (12, 4, 30, 1, 1, 0): 84, (12, 4, 30, 1, 0, 1): 56,
              (12, 4, 50, 0, 0, 0): 40, (12, 4, 50, 0, 1, 0): 68, (12, 4, 50, 0, 0, 1): 192}
ROWLANE = [(12, 4, 30), (12, 4, 25), (12, 4, 20), (12, 4, 10), (4, 1, 10), (8, 3, 7), (12, 4, 40), (12, 4, 50)]


@pytest.fixture(scope="module")
def rowlane():
    return T.build.device_asm("admm_rowlane.hip").read_text()


def pm_key(nx, nu, n, ex, mpc, bpi):
    b = lambda v: f"Lb{int(v)}E"
    return f"admm_rowlane_pm_kernelILi{nx}ELi{nu}ELi{n}E{b(ex)}{b(mpc)}{b(bpi)}EEv"


def test_every_per_instance_instantiation_has_its_scratch_pinned(rowlane):
    sizes = scratch_sizes(rowlane)
    seen = 0
    for nx, nu, n in ROWLANE:
        for ex in (1, 0):
            for mpc, bpi in ((0, 0), (1, 0), (0, 1)):
                key = pm_key(nx, nu, n, ex, mpc, bpi)
                got = [v for k, v in sizes.items() if key in k]
                assert len(got) == 1, key
                pin = PM_SCRATCH.get((nx, nu, n, ex, mpc, bpi), 0)
                assert got[0] <= pin, f"{key}: {got[0]} bytes of scratch per lane, pinned at {pin}"
                seen += 1
    assert seen == sum(1 for k in sizes if "admm_rowlane_pm_kernel" in k) == 48


def test_per_instance_kernels_are_free_of_dpp_hazards_and_packed_adds(rowlane):
    ks = {n: l for n, l in kernels_of(rowlane).items() if "admm_rowlane_pm_kernel" in n}
    assert len(ks) == 48
    for n, lines in ks.items():
        assert not hazards(lines), n
        assert not any(i.startswith("v_pk_add_f32") for i in lines), n


def test_riccati_kernel_needs_no_scratch():
    txt = T.build.device_asm("riccati_batch.hip").read_text()
    sizes = {k: v for k, v in scratch_sizes(txt).items() if "riccati_batch_kernel" in k}
    assert len(sizes) == 1 and list(sizes.values())[0] == 0, sizes
    i = re.search(r"^_Z\w*riccati_batch_kernel\w*:", txt, re.M).start()
    m = re.search(r"; TotalNumVgprs: (\d+)", txt[i:])
    assert m and int(m.group(1)) <= 96, m and m.group(1)
