"""Static figures of the wave kernels' per-instance-settings instantiations (admm_waveres_ps.hip, admm_wave_ps.hip: the kernels of admm_waveres.hip and
admm_wave.hip compiled with a trailing SettingsParams, in translation units of their own) beside their shared twins, read from the `hipcc -S` listings
(build.device_asm).  CPU test: hipcc cross-compiles, no GPU needed.  It reads register counts, scratch sizes, occupancy and kernel names only.  The
figures are pinned as built: the instance's record is wave-uniform (four scalar registers), so no ps kernel needs a vector register more than its twin
and waveres<32,16,exact,ps> stays at its twin's 255 without scratch ('The wave kernels under settings', has the same table)."""
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import figures, kernels_of

# (NX, NU, EXACT): (VGPRs, AGPRs, bytes of scratch per lane) of admm_waveres_ps_kernel | of admm_waveres_kernel
WAVERES_PS = {(16, 4, 0): (186, 0, 0), (16, 4, 1): (196, 0, 0), (16, 8, 0): (198, 0, 0), (16, 8, 1): (200, 0, 0), (20, 8, 0): (206, 0, 0), (20, 8, 1): (212, 0, 0),
              (24, 4, 0): (202, 0, 0), (24, 4, 1): (220, 0, 0), (32, 16, 0): (254, 0, 0), (32, 16, 1): (255, 0, 0)}
WAVERES = {(16, 4, 0): (187, 0, 0), (16, 4, 1): (196, 0, 0), (16, 8, 0): (199, 0, 0), (16, 8, 1): (200, 0, 0), (20, 8, 0): (207, 0, 0), (20, 8, 1): (212, 0, 0),
           (24, 4, 0): (203, 0, 0), (24, 4, 1): (220, 0, 0), (32, 16, 0): (254, 0, 0), (32, 16, 1): (255, 0, 0)}
# (NX, NU, PF, WPS): admm_wavestream_ps_kernel | admm_wavestream_kernel
WAVESTREAM_PS = {(16, 4, 1, 3): (110, 0, 0), (16, 4, 4, 2): (160, 0, 0), (16, 8, 1, 3): (118, 0, 0), (16, 8, 4, 2): (168, 0, 0), (20, 8, 1, 3): (130, 0, 0),
                 (20, 8, 4, 2): (176, 0, 0), (24, 4, 1, 3): (136, 0, 0), (24, 4, 4, 2): (176, 0, 0), (32, 16, 1, 3): (168, 0, 64), (32, 16, 4, 2): (224, 0, 0)}
WAVESTREAM = dict(WAVESTREAM_PS)  # as built, the streaming kernel's figures do not move at all
UNITS = ("admm_waveres_ps.hip", "admm_wave_ps.hip", "admm_waveres.hip", "admm_wave.hip", "admm_waveres_pm.hip", "admm_wave_pm.hip")


@pytest.fixture(scope="module")
def listings():
    assert set(getattr(T.build, "ADDED_SOURCES", [])) >= {"admm_waveres_ps.hip", "admm_wave_ps.hip"}, "the build has no ps units of the wave kernels"
    return {u: T.build.device_asm(u).read_text() for u in UNITS}


def _fig(listings):
    return {"waveres_ps": figures(listings["admm_waveres_ps.hip"], "admm_waveres_ps_kernel", lambda n: "SettingsParams" in n),
            "waveres": figures(listings["admm_waveres.hip"], "admm_waveres_kernel", lambda n: True),
            "wavestream_ps": figures(listings["admm_wave_ps.hip"], "admm_wavestream_ps_kernel", lambda n: "SettingsParams" in n),
            "wavestream": figures(listings["admm_wave.hip"], "admm_wavestream_kernel", lambda n: True)}


def test_the_new_units_hold_exactly_the_ps_instantiations(listings):
    res, stream = list(kernels_of(listings["admm_waveres_ps.hip"])), list(kernels_of(listings["admm_wave_ps.hip"]))
    assert len(res) == 10 and all("admm_waveres_ps_kernel" in n and "SettingsParams" in n for n in res), res
    assert len(stream) == 10 and all("admm_wavestream_ps_kernel" in n and "SettingsParams" in n for n in stream), stream
    for u in ("admm_waveres.hip", "admm_wave.hip", "admm_waveres_pm.hip", "admm_wave_pm.hip"):  # and none has leaked into a parent or pm unit
        assert not [n for n in kernels_of(listings[u]) if "SettingsParams" in n or "_ps_kernel" in n], u
    assert len(list(kernels_of(listings["admm_waveres.hip"]))) == 10 and len(list(kernels_of(listings["admm_wave.hip"]))) == 10
    assert len(list(kernels_of(listings["admm_waveres_pm.hip"]))) == 11 and len(list(kernels_of(listings["admm_wave_pm.hip"]))) == 10


def test_every_ps_instantiation_has_its_twin_s_waves_per_simd(listings):
    f = _fig(listings)
    assert set(f["waveres_ps"]) == set(f["waveres"]) == set(WAVERES)
    for key, v in f["waveres_ps"].items():
        assert v[3] == f["waveres"][key][3] == 2, (key, v, f["waveres"][key])
    # the streaming kernel's launch bounds ask for WPS = 2 or 3 waves per SIMD; the smaller classes fit more, and the ps form fits what its twin does
    assert set(f["wavestream_ps"]) == set(f["wavestream"]) == set(WAVESTREAM)
    for key, v in f["wavestream_ps"].items():
        assert v[3] == f["wavestream"][key][3] >= key[3], (key, v, f["wavestream"][key])
    assert f["wavestream_ps"][(32, 16, 4, 2)][3] == 2 and f["wavestream_ps"][(32, 16, 1, 3)][3] == 3


def test_waveres_ps_has_no_scratch_and_wavestream_ps_no_more_than_its_twin(listings):
    f = _fig(listings)
    for key in WAVERES:
        assert f["waveres_ps"][key][2] == 0 and f["waveres"][key][2] == 0, key
    for key in WAVESTREAM:
        assert f["wavestream_ps"][key][2] <= f["wavestream"][key][2], key


def test_register_and_scratch_figures_are_pinned(listings):
    f = _fig(listings)
    for what, pins in (("waveres_ps", WAVERES_PS), ("waveres", WAVERES), ("wavestream_ps", WAVESTREAM_PS), ("wavestream", WAVESTREAM)):
        for key, pin in pins.items():
            assert f[what][key][:3] == pin, f"{what} {key}: (VGPRs, AGPRs, scratch) = {f[what][key][:3]}, pinned at {pin}"


def test_design_records_the_figures_beside_the_twins():
    text = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    sec = text[text.index("### The wave kernels under settings"):]
    sec = sec[:sec.index("\n### ", 4)] if "\n### " in sec[4:] else sec
    cell = lambda f: f"{f[0]} / {f[1]} / {f[2]}"
    for key in WAVERES_PS:
        row = f"| waveres ({key[0]},{key[1]},{'exact' if key[2] else 'fma'}) | {cell(WAVERES_PS[key])} | {cell(WAVERES[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
    for key in WAVESTREAM_PS:
        row = f"| wavestream ({key[0]},{key[1]},PF={key[2]},WPS={key[3]}) | {cell(WAVESTREAM_PS[key])} | {cell(WAVESTREAM[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
