"""CPU side of the fp64 per-instance-settings tests: the draw that tests/test_settings64_gpu.py compares on the device (settings64_cases.draw, the same
function) is not vacuous.  On the fp64 oracle alone, over the cold solve at B = 67 of every class: instances converge before their own budget and
instances use it up, some budget is 0, a check_termination > 1 delays an instance's end, the four rows of some wave end on four different
iterations, the tolerances are doubles that no float32 holds, and the batch-wide BASE settings would end more than one instance elsewhere."""
import numpy as np
import pytest

import settings64_cases as SC


@pytest.fixture(scope="module")
def cold_solves(tinympc, oracle_mod):
    """{dims: (per, iter, status, iter with check_termination = 1 for everyone, iter under BASE for everyone)} of the cold solve at B = 67, shared bounds"""
    out = {}
    B = SC.BATCHES[-1]
    for dims in SC.CLASSES:
        prob, x0, xref, bnds = SC.inputs(tinympc.problems, oracle_mod, dims, B, "shared")
        per = SC.draw(B)
        res = []
        for p in (per, dict(per, check_termination=np.ones(B, np.int32)), {}):
            st = oracle_mod.new_state(B, *dims, SC.DT)
            st["x"][:, 0] = x0
            SC.oracle_solve(oracle_mod, prob, p, st, bnds, xref)
            res.append((st["iter"].copy(), st["status"].copy()))
        out[dims] = (per, res[0][0], res[0][1], res[1][0], res[2][0])
    return out


def test_the_draw_covers_every_budget_and_check_value_in_double():
    per = SC.draw(SC.BATCHES[-1])
    assert set(per["max_iter"]) == set(SC.BUDGETS) and set(per["check_termination"]) == set(SC.CHECKS)
    assert (per["max_iter"] == 0).any()
    for k in ("abs_pri_tol", "abs_dua_tol"):
        t = per[k]
        assert t.dtype == np.float64 and 1e-3 <= t.min() and t.max() <= 1.0 and np.log10(t.max() / t.min()) > 2.5
        assert (t != t.astype(np.float32).astype(np.float64)).all(), f"{k}: some tolerance is a float32 value: narrowing it on the way would go unseen"
    small = SC.draw(5)
    assert len(set(small["max_iter"])) == 5 and len(set(small["check_termination"])) == 4
    again = SC.draw(SC.BATCHES[-1], SC.SEED + 1)
    assert (again["max_iter"] != per["max_iter"]).any() and (again["abs_pri_tol"] != per["abs_pri_tol"]).all()


@pytest.mark.parametrize("dims", SC.CLASSES, ids=lambda d: "x".join(map(str, d)))
def test_both_ways_out_of_the_loop_occur(cold_solves, dims):
    per, it, st, _, _ = cold_solves[dims]
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
    per, it, st, it_ct1, _ = cold_solves[dims]
    later = (per["check_termination"] > 1) & (it > it_ct1)
    waves = [it[w:w + 4] for w in range(0, len(it) - 3, 4)]
    four = sum(len(set(w)) == 4 for w in waves)
    print(dims, "delayed by check_termination:", int(later.sum()), "waves ending on four iterations:", four)
    assert later.any(), "no instance with check_termination > 1 ends later than it would with check_termination = 1"
    assert four >= 1, "no wave whose four instances all end on different iterations"


@pytest.mark.parametrize("dims", SC.CLASSES, ids=lambda d: "x".join(map(str, d)))
def test_the_batch_wide_settings_would_end_instances_elsewhere(cold_solves, dims):
    """an implementation that ran BASE for everyone is seen: iter moves for more than one instance"""
    _, it, _, _, it_base = cold_solves[dims]
    assert (it != it_base).sum() > 1
