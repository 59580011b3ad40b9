"""Static figures of the wave kernels' per-instance-model instantiations (admm_waveres_pm.hip, admm_wave_pm.hip: the kernels of admm_waveres.hip and
admm_wave.hip compiled with a trailing ModelParams, in translation units of their own) beside their shared twins, read from the `hipcc -S` listings
(build.device_asm).  CPU test: hipcc cross-compiles, no GPU needed.  The figures are pinned as built: the gain table's base and rho are wave-uniform
(scalar registers), so the vector register counts stay within one of the twins' ('The wave kernels under models', has the same table)."""
import re
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import figures, kernels_of

# (NX, NU, EXACT): (VGPRs, AGPRs, bytes of scratch per lane) of admm_waveres_pm_kernel | of admm_waveres_kernel
WAVERES_PM = {(16, 4, 0): (186, 0, 0), (16, 4, 1): (196, 0, 0), (16, 8, 0): (198, 0, 0), (16, 8, 1): (200, 0, 0), (20, 8, 0): (206, 0, 0), (20, 8, 1): (212, 0, 0),
              (24, 4, 0): (202, 0, 0), (24, 4, 1): (220, 0, 0), (32, 16, 0): (254, 0, 0), (32, 16, 1): (255, 0, 0)}
WAVERES = {(16, 4, 0): (187, 0, 0), (16, 4, 1): (196, 0, 0), (16, 8, 0): (199, 0, 0), (16, 8, 1): (200, 0, 0), (20, 8, 0): (207, 0, 0), (20, 8, 1): (212, 0, 0),
           (24, 4, 0): (203, 0, 0), (24, 4, 1): (220, 0, 0), (32, 16, 0): (254, 0, 0), (32, 16, 1): (255, 0, 0)}
# (NX, NU, PF, WPS): admm_wavestream_pm_kernel | admm_wavestream_kernel
WAVESTREAM_PM = {(16, 4, 1, 3): (110, 0, 0), (16, 4, 4, 2): (160, 0, 0), (16, 8, 1, 3): (118, 0, 0), (16, 8, 4, 2): (168, 0, 0), (20, 8, 1, 3): (130, 0, 0),
                 (20, 8, 4, 2): (176, 0, 0), (24, 4, 1, 3): (136, 0, 0), (24, 4, 4, 2): (176, 0, 0), (32, 16, 1, 3): (168, 0, 64), (32, 16, 4, 2): (224, 0, 0)}
WAVESTREAM = dict(WAVESTREAM_PM)  # as built, the streaming kernel's figures do not move at all


@pytest.fixture(scope="module")
def listings():
    return {u: T.build.device_asm(u).read_text() for u in ("admm_waveres_pm.hip", "admm_wave_pm.hip", "admm_waveres.hip", "admm_wave.hip")}


def _fig(listings):
    return {"waveres_pm": figures(listings["admm_waveres_pm.hip"], "admm_waveres_pm_kernel", lambda n: "ModelParams" in n),
            "waveres": figures(listings["admm_waveres.hip"], "admm_waveres_kernel", lambda n: True),
            "wavestream_pm": figures(listings["admm_wave_pm.hip"], "admm_wavestream_pm_kernel", lambda n: "ModelParams" in n),
            "wavestream": figures(listings["admm_wave.hip"], "admm_wavestream_kernel", lambda n: True)}


def test_the_new_units_hold_exactly_the_pm_instantiations(listings):
    res, stream = list(kernels_of(listings["admm_waveres_pm.hip"])), list(kernels_of(listings["admm_wave_pm.hip"]))
    pack = [n for n in res if "models_pack_wave_kernel" in n]
    assert len(pack) == 1 and len(res) == 11 and all("admm_waveres_pm_kernel" in n and "ModelParams" in n for n in res if n not in pack), res
    assert len(stream) == 10 and all("admm_wavestream_pm_kernel" in n and "ModelParams" in n for n in stream), stream
    for u in ("admm_waveres.hip", "admm_wave.hip"):  # and none has leaked into a pinned unit
        assert not [n for n in kernels_of(listings[u]) if "ModelParams" in n or "_pm_kernel" in n or "models_pack" in n], u
    assert len(list(kernels_of(listings["admm_waveres.hip"]))) == 10 and len(list(kernels_of(listings["admm_wave.hip"]))) == 10


def test_every_pm_instantiation_has_its_twin_s_waves_per_simd(listings):
    f = _fig(listings)
    assert set(f["waveres_pm"]) == set(f["waveres"]) == set(WAVERES)
    for key, v in f["waveres_pm"].items():
        assert v[3] == f["waveres"][key][3] == 2, (key, v, f["waveres"][key])
    # the streaming kernel's launch bounds ask for WPS = 2 or 3 waves per SIMD; the smaller classes fit more, and the pm form fits what its twin does
    assert set(f["wavestream_pm"]) == set(f["wavestream"]) == set(WAVESTREAM)
    for key, v in f["wavestream_pm"].items():
        assert v[3] == f["wavestream"][key][3] >= key[3], (key, v, f["wavestream"][key])
    assert f["wavestream_pm"][(32, 16, 4, 2)][3] == 2 and f["wavestream_pm"][(32, 16, 1, 3)][3] == 3


def test_waveres_pm_has_no_scratch(listings):
    f = _fig(listings)
    for key in WAVERES:
        assert f["waveres_pm"][key][2] == 0 and f["waveres"][key][2] == 0, key


def test_register_and_scratch_figures_are_pinned(listings):
    f = _fig(listings)
    for what, pins in (("waveres_pm", WAVERES_PM), ("waveres", WAVERES), ("wavestream_pm", WAVESTREAM_PM), ("wavestream", WAVESTREAM)):
        for key, pin in pins.items():
            assert f[what][key][:3] == pin, f"{what} {key}: (VGPRs, AGPRs, scratch) = {f[what][key][:3]}, pinned at {pin}"


def test_the_record_offset_is_formed_in_64_bits(listings):
    """inst * mats_stride is a 64-bit product before it is scaled to bytes (65 536 records of the nx = 32 class pass 2 GiB): every pm kernel has a
    high-half scalar multiply more than its twin, which forms the per-instance bounds offset the same way"""
    def highs(text, kernel):
        out = {}
        for m in re.finditer(rf"^(_Z\w*\d+{kernel}I\w*):", text, re.M):
            body = text[m.end():text.index("s_endpgm", m.end())]
            out[tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))] = body.count("s_mul_hi_u32")
        return out
    for pm_u, pm_k, u, k in (("admm_waveres_pm.hip", "admm_waveres_pm_kernel", "admm_waveres.hip", "admm_waveres_kernel"),
                             ("admm_wave_pm.hip", "admm_wavestream_pm_kernel", "admm_wave.hip", "admm_wavestream_kernel")):
        pm, twin = highs(listings[pm_u], pm_k), highs(listings[u], k)
        assert set(pm) == set(twin) and len(pm) == 10
        for key in pm:
            assert pm[key] > twin[key] >= 1, (pm_k, key, pm[key], twin[key])


def test_design_records_the_figures_beside_the_twins():
    text = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    sec = text[text.index("### The wave kernels under models"):]
    cell = lambda f: f"{f[0]} / {f[1]} / {f[2]}"
    for key in WAVERES_PM:
        row = f"| waveres ({key[0]},{key[1]},{'exact' if key[2] else 'fma'}) | {cell(WAVERES_PM[key])} | {cell(WAVERES[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
    for key in WAVESTREAM_PM:
        row = f"| wavestream ({key[0]},{key[1]},PF={key[2]},WPS={key[3]}) | {cell(WAVESTREAM_PM[key])} | {cell(WAVESTREAM[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
