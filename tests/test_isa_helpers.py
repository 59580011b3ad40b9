"""The helper kernels of both libraries live in units of their own (batch_helpers.hip, batch64_helpers.hip) and the two host files hold no device
code: kernel sets and instruction streams read from the `hipcc -S` listings (build.device_asm), pinned to what the kernels compiled to while
they were still part of the host files.  CPU test: hipcc cross-compiles, no GPU needed."""
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import fingerprint, kernel_key, kernels_of

CSRC = Path(T.build.CSRC)
HOST_FILES = ("tinympc_batch.hip", "tinympc_batch64.hip")
F32_KERNELS = {"guard_fill_kernel", "guard_count_kernel", "pack_kernel", "unpack_kernel", "zero_kernel", "dual_width_kernel", "plant_step_kernel",
               "plant_step_pm_kernel", "plant_step_sim_kernel", "models_gather_kernel", "models_pack_row_kernel", "systems_to_models_kernel",
               "bounds_table_kernel", "tile16_image_kernel", "rows_vary_kernel"}
F64_KERNELS = {"pack64_kernel", "unpack64_kernel", "gather_window64_kernel"}
# fingerprint() of the host files' own listings at the last commit that held these kernels (2dff9b2): (kernels, instruction lines, hash)
F32_FINGERPRINT = (15, 11783, "13608c3d27b40193")
F64_FINGERPRINT = (3, 1217, "30aa079a897e20ec")


@pytest.mark.parametrize("unit, kernels, pinned", [("batch_helpers.hip", F32_KERNELS, F32_FINGERPRINT), ("batch64_helpers.hip", F64_KERNELS, F64_FINGERPRINT)])
def test_the_helper_unit_holds_its_kernels_instruction_for_instruction(unit, kernels, pinned):
    listing = T.build.device_asm(unit).read_text()
    names = sorted(kernel_key(n)[0] for n in kernels_of(listing))
    assert names == sorted(kernels), names
    got = fingerprint([listing])
    print(f"fingerprint of {unit} = {got}, pinned at {pinned}")
    assert got == pinned


@pytest.mark.parametrize("host", HOST_FILES)
def test_the_host_file_compiles_to_no_kernel(host):
    assert kernels_of(T.build.device_asm(host).read_text()) == {}


@pytest.mark.parametrize("host", HOST_FILES)
def test_the_host_file_defines_and_launches_no_kernel(host):
    text = (CSRC / host).read_text()
    for word in ("__global__", "__device__", "hipLaunchKernelGGL", "<<<"):
        assert word not in text, f"{host} contains {word}"
