"""CPU side of tests/test_settings_wave_gpu.py: the draw it compares on the device (settings_cases.inputs / draw / oracle_solve, unchanged) is not
vacuous for the wave classes either.  On the oracle alone, over the cold solve of 37 instances of every class: at least 10 % converge before their own
budget and at least 10 % use it up, some budget is 0, a check_termination > 1 delays some instance's end, and everything is finite.  The table that
build.ADDED_UNITS and tests/golden/kernel_units_added.json give the two new units is checked here too."""
import json
from pathlib import Path

import numpy as np
import pytest

import settings_cases as SC

CLASSES = [(16, 4, 3), (16, 4, 10), (16, 4, 50), (16, 4, 51), (16, 8, 10), (24, 4, 10), (32, 16, 50)]
B = 37


@pytest.fixture(scope="module")
def cold_solves(tinympc, oracle_mod):
    """{dims: (per, state, iter with check_termination = 1 for everyone)} of the cold solve, shared bounds"""
    out = {}
    for dims in CLASSES:
        prob, x0, xref, bnds = SC.inputs(tinympc.problems, oracle_mod, dims, B, "shared")
        per = SC.draw(B)
        res = []
        for p in (per, dict(per, check_termination=np.ones(B, np.int32))):
            st = oracle_mod.new_state(B, *dims)
            st["x"][:, 0] = x0
            SC.oracle_solve(oracle_mod, prob, np.float32, p, st, bnds, xref)
            res.append(st)
        out[dims] = (per, res[0], res[1]["iter"].copy())
    return out


@pytest.mark.parametrize("dims", CLASSES, ids=lambda d: "x".join(map(str, d)))
def test_both_ways_out_of_the_loop_occur(cold_solves, dims):
    per, st, _ = cold_solves[dims]
    it, status = st["iter"], st["status"]
    ran = per["max_iter"] > 0
    early = ran & (status == 1) & (it < per["max_iter"])
    spent = ran & (status == 11) & (it == per["max_iter"])
    print(dims, "converge before their budget:", int(early.sum()), "use it up:", int(spent.sum()), "of", B)
    assert early.sum() >= 0.1 * B, "fewer than 10 % of the instances converge before their budget"
    assert spent.sum() >= 0.1 * B, "fewer than 10 % of the instances use up their budget"
    zero = per["max_iter"] == 0
    assert zero.any() and (status[zero] == 11).all() and (it[zero] == 1).all()
    assert all(np.isfinite(v).all() for v in st.values())


@pytest.mark.parametrize("dims", CLASSES, ids=lambda d: "x".join(map(str, d)))
def test_check_termination_delays_an_end(cold_solves, dims):
    per, st, it_ct1 = cold_solves[dims]
    later = (per["check_termination"] > 1) & (st["iter"] > it_ct1)
    print(dims, "delayed by check_termination:", int(later.sum()))
    assert later.any(), "no instance with check_termination > 1 ends later than it would with check_termination = 1"


def test_the_ps_names_route_to_the_new_units(tinympc):
    """build.ADDED_UNITS: each ps unit a variant of the shared kernel's text; the names tiny_batch_kernel_name() gives them route there"""
    B_ = tinympc.build
    assert B_.ADDED_SOURCES == ["admm_wave_ps.hip", "admm_waveres_ps.hip"]
    assert B_.INCLUDED_SOURCES["admm_wave_ps.hip"] == ["admm_wave.hip"] and B_.INCLUDED_SOURCES["admm_waveres_ps.hip"] == ["admm_waveres.hip"]
    golden = json.loads((Path(__file__).resolve().parent / "golden" / "kernel_units_added.json").read_text())
    for name, unit in (("waveres<32,16,exact,ps>", "admm_waveres_ps.hip"), ("waveres<16,4,fast,ps>", "admm_waveres_ps.hip"),
                       ("wavestream<32,16,exact,ps>", "admm_wave_ps.hip"), ("wavestream<16,4,exact,ps>", "admm_wave_ps.hip")):
        assert B_.unit_of(name) == unit, name
        assert golden.get(name) == unit, f"{name} is not in tests/golden/kernel_units_added.json"
    for name, unit in (("waveres<32,16,exact>", "admm_waveres.hip"), ("waveres<32,16,exact,pm>", "admm_waveres_pm.hip"),
                       ("wavestream<32,16,exact>", "admm_wave.hip"), ("wavestream<32,16,exact,pm>", "admm_wave_pm.hip")):
        assert B_.unit_of(name) == unit, name
