"""CPU side of the per-instance-settings tests: the draw that tests/test_settings_gpu.py compares on the device (settings_cases.draw, the same function) is
not vacuous.  On the oracle alone, over the cold solve of the largest batch of every class: instances converge before their budget and instances use
it up, some budget is 0, a check_termination > 1 delays an instance's end, and the four rows of some wave end on four different iterations."""
import numpy as np
import pytest

import settings_cases as SC


@pytest.fixture(scope="module")
def cold_solves(tinympc, oracle_mod):
    """{dims: (per, iter, status, iter with check_termination = 1 for everyone)} of the cold solve at B = 67, shared bounds"""
    out = {}
    B = SC.BATCHES[-1]
    for dims in SC.CLASSES:
        prob, x0, xref, bnds = SC.inputs(tinympc.problems, oracle_mod, dims, B, "shared")
        per = SC.draw(B)
        res = []
        for p in (per, dict(per, check_termination=np.ones(B, np.int32))):
            st = oracle_mod.new_state(B, *dims)
            st["x"][:, 0] = x0
            SC.oracle_solve(oracle_mod, prob, np.float32, p, st, bnds, xref)
            res.append((st["iter"].copy(), st["status"].copy()))
        out[dims] = (per, res[0][0], res[0][1], res[1][0])
    return out


def test_the_draw_covers_every_budget_and_check_value():
    per = SC.draw(SC.BATCHES[-1])
    assert set(per["max_iter"]) == set(SC.BUDGETS) and set(per["check_termination"]) == set(SC.CHECKS)
    assert per["abs_pri_tol"].dtype == np.float32 and np.log10(per["abs_pri_tol"].max() / per["abs_pri_tol"].min()) > 2.5
    assert (per["max_iter"] == 0).any()
    small = SC.draw(5)
    assert len(set(small["max_iter"])) == 5 and len(set(small["check_termination"])) == 4
    again = SC.draw(SC.BATCHES[-1], SC.SEED + 1)
    assert (again["max_iter"] != per["max_iter"]).any() and (again["abs_pri_tol"] != per["abs_pri_tol"]).all()


@pytest.mark.parametrize("dims", SC.CLASSES, ids=lambda d: "x".join(map(str, d)))
def test_both_ways_out_of_the_loop_occur(cold_solves, dims):
    per, it, st, _ = cold_solves[dims]
    B = len(it)
    ran = per["max_iter"] > 0
    early = ran & (st == 1) & (it < per["max_iter"])
    spent = ran & (st == 11) & (it == per["max_iter"])
    print(dims, "converge before their budget:", int(early.sum()), "use it up:", int(spent.sum()), "of", B)
    assert early.sum() >= 0.1 * B, "fewer than 10 % of the instances converge before their budget"
    assert spent.sum() >= 0.1 * B, "fewer than 10 % of the instances use up their budget"
    zero = per["max_iter"] == 0
    assert zero.any() and (st[zero] == 11).all() and (it[zero] == 1).all()


@pytest.mark.parametrize("dims", SC.CLASSES, ids=lambda d: "x".join(map(str, d)))
def test_check_termination_delays_an_end_and_a_wave_ends_on_four_iterations(cold_solves, dims):
    per, it, st, it_ct1 = cold_solves[dims]
    later = (per["check_termination"] > 1) & (it > it_ct1)
    assert later.any(), "no instance with check_termination > 1 ends later than it would with check_termination = 1"
    waves = [it[w:w + 4] for w in range(0, len(it) - 3, 4)]
    assert any(len(set(w)) == 4 for w in waves), "no wave whose four instances all end on different iterations"
