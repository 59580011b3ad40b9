"""Per-instance models on the wave kernels: coverage guards that need no GPU."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _wavedims():
    hdr = (ROOT / "accelerated-tinympc_amd" / "csrc" / "tinympc_internal.h").read_text()
    line = re.search(r"#define TINY_FOR_EACH_WAVEDIMS\(X\)(.*)", hdr).group(1)
    return {tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+)\)", line)}


def test_every_wave_pm_class_has_a_gpu_test():
    """Every class of TINY_FOR_EACH_WAVEDIMS (admm_waveres_pm_kernel and admm_wavestream_pm_kernel are instantiated for each) is listed in
    tests/test_models_wave_gpu.py and is a case of its waveres test, so a new class cannot land untested."""
    import test_models_wave_gpu as G
    classes = _wavedims()
    assert len(classes) == 5, classes
    assert set(G.WAVEDIMS) == classes and len(G.WAVEDIMS) == len(classes)
    assert {c[:2] for c, _ in G.WAVERES_CASES} == classes
    assert {B for _, B in G.WAVERES_CASES} == {1, 37}
    # the streaming kernel: a horizon beyond waveres and both launch shapes (<= 2 048 instances, more)
    assert any(c[2] > 50 for c in G.WAVESTREAM_CASES) and any(c[3] > 2048 for c in G.WAVESTREAM_CASES) and any(c[3] <= 2048 for c in G.WAVESTREAM_CASES)


def test_the_new_units_are_built_like_their_parents():
    import accelerated_tinympc_amd as T
    b = T.build
    for unit, parent in (("admm_waveres_pm.hip", "admm_waveres.hip"), ("admm_wave_pm.hip", "admm_wave.hip")):
        assert unit in b.SOURCES and b.INCLUDED_SOURCES[unit] == [parent]
        assert b.EXTRA_FLAGS.get(unit, []) == b.EXTRA_FLAGS.get(parent, [])
        text = (b.CSRC / unit).read_text()
        assert f'#include "{parent}"' in text and "__global__" not in text  # the unit is its parent under a macro, nothing else


def test_the_host_file_launches_nothing_itself():
    """the pack kernel lives in admm_waveres_pm.hip: tinympc_batch.hip reaches it through the typed launcher of tinympc_internal.h"""
    host = (ROOT / "accelerated-tinympc_amd" / "csrc" / "tinympc_batch.hip").read_text()
    assert "launch_models_pack_wave(" in host and "models_pack_wave_kernel" not in host
    hdr = (ROOT / "accelerated-tinympc_amd" / "csrc" / "tinympc_internal.h").read_text()
    for decl in ("launch_models_pack_wave(", "launch_admm_waveres_pm(", "launch_admm_wavestream_pm(", "pm_wave_floats("):
        assert decl in hdr, decl
