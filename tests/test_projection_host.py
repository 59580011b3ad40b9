"""CPU tests of the box projection at its edges (admm.cpp:51-60, the solver's only non-linear step): the inputs of tests/test_projection_gpu.py do
what they are built for (checked on the oracle alone), the oracle's tie rule is the compiled reference's on those inputs — Eigen's packets and its
scalar tail alike — and the v_med3_f32 of the ISA manual, as a numpy model, differs from that rule in two combinations of zero signs and nowhere else."""
import numpy as np
import pytest

from helpers import (PROJ_CATS, PROJ_EXACT, PROJ_INPUTS, STATE_ORDER, compare_select, med3_model, projection_case, projection_input,
                     projection_problem, same_bits)
from test_oracle import CFGS

IDS = [f"{nx}-{nu}-{N}-{np.dtype(dt).name if not isinstance(dt, str) else dt}-{'shared' if not m else 'inst' if m is True else m}"
       for nx, nu, N, B, dt, m in PROJ_INPUTS]


def full(b, like):
    return np.broadcast_to(b, like.shape)


def iteration_one(O, prob, dtype, case, **over):
    st = O.copy_state(case["st0"])
    O.Oracle(prob, dtype, dict(PROJ_EXACT, max_iter=1, **over)).solve(st, *case["bnds"], case["xref"])
    return st


@pytest.mark.parametrize("key", PROJ_INPUTS, ids=IDS)
def test_projection_inputs_reach_every_edge(oracle_mod, tinympc, key):
    """Non-vacuity of one input set, on the oracle alone."""
    O = oracle_mod
    nx, nu, N, B, dtype, mode = key
    prob, case = projection_input(tinympc.problems, O, key)
    st = iteration_one(O, prob, dtype, case)
    xmn, xmx, umn, umx = case["bnds"]
    for name, new, t, lo, hi, cat, laid, dense in (("vnew", st["vnew"], case["t"][0], xmn, xmx, case["cat"][0], case["laid"][0], case["dense"][0]),
                                                   ("znew", st["znew"], case["t"][1], umn, umx, case["cat"][1], case["laid"][1], case["dense"][1])):
        lo, hi = full(lo, t), full(hi, t)
        # the oracle's iteration 1 is the reference's two compare-selects of the t this case was crafted around
        assert same_bits(new, compare_select(t, lo, hi)), name
        # every category of the draw occurs, as a fact about (t, lo, hi): one entry of a shared table is a tie for one instance, binds for others
        seen = {"slack": (lo < t) & (t < hi) & np.isfinite(lo) & np.isfinite(hi), "binds strictly below": t < lo, "binds strictly above": t > hi,
                "tie low": (t == lo) & (lo < hi), "tie high": (t == hi) & (lo < hi), "pinned": (t == lo) & (lo == hi),
                "lo = +0": (lo == 0) & ~np.signbit(lo), "lo = -0": (lo == 0) & np.signbit(lo), "hi = +0": (hi == 0) & ~np.signbit(hi),
                "hi = -0": (hi == 0) & np.signbit(hi), "infeasible": lo > hi, "lo = -inf": np.isneginf(lo), "hi = +inf": np.isposinf(hi)}
        for what, m in seen.items():
            assert m.any(), f"{name}: {what} does not occur"
        assert dense or set(np.unique(cat)) == set(range(len(PROJ_CATS))), f"{name}: categories {sorted(set(range(len(PROJ_CATS))) - set(np.unique(cat)))} not drawn"
        # the first and the last step and row: every category as far as the line is long, less the entries the zero bounds were laid over
        for what, sel in (("first step", np.s_[:, 0, :]), ("last step", np.s_[:, -1, :]), ("first row", np.s_[:, :, 0]), ("last row", np.s_[:, :, -1])):
            line = cat[sel][~laid[sel]]
            want = min(cat[sel].size, len(PROJ_CATS)) - int(laid[sel].sum())
            if dense:   # nine categories by turns along the line, but for the two corners it shares with lines filled before it
                want = min(line.size - 2, len(PROJ_CATS) - 4)
            assert len(np.unique(line)) >= min(want, len(PROJ_CATS)), (name, what, len(np.unique(line)), want)
        # ties and pinned entries hold bit for bit where the entry's t was the source (per-instance tables: everywhere they were drawn)
        if mode is True:
            c = lambda n: (cat == PROJ_CATS.index(n)) & ~laid
            assert same_bits(lo[c("tie_lo") | c("pinned")], t[c("tie_lo") | c("pinned")]) and same_bits(hi[c("tie_hi") | c("pinned")], t[c("tie_hi") | c("pinned")])
            assert (lo[c("bind_lo")] > t[c("bind_lo")]).all() and (hi[c("bind_hi")] < t[c("bind_hi")]).all()
        assert (t == lo).sum() >= 2 and (t == hi).sum() >= 2, f"{name}: too few exact ties"
        assert ((t == lo) & (t != 0)).any() and ((t == hi) & (t != 0)).any(), f"{name}: no tie away from zero"
        # the eight combinations of a zero t with a zero bound, each at least twice
        for tneg in (False, True):
            tz = (t == 0) & (np.signbit(t) == tneg)
            for bound, bname in ((lo, "lo"), (hi, "hi")):
                for bneg in (False, True):
                    n = int((tz & (bound == 0) & (np.signbit(bound) == bneg)).sum())
                    assert n >= 2, f"{name}: t = {'-' if tneg else '+'}0 with {bname} = {'-' if bneg else '+'}0 occurs {n} times"
        # a bound of each side is active in the result, strictly (the projection moved the value)
        assert ((new == lo) & (t < lo)).any() and ((new == hi) & (t > hi)).any(), f"{name}: no strictly active bound on both sides"
        assert np.isfinite(new).all(), f"{name}: not finite"
    for settings in (dict(max_iter=6), dict(max_iter=6, en_state_bound=0), dict(max_iter=6, en_input_bound=0)):
        s6 = O.copy_state(case["st0"])
        O.Oracle(prob, dtype, dict(PROJ_EXACT, **settings)).solve(s6, *case["bnds"], case["xref"])
        assert all(np.isfinite(s6[k]).all() for k in STATE_ORDER), settings
        assert (s6["iter"] == 6).all() and (s6["status"] == 11).all()


@pytest.mark.parametrize("dt,nx,nu,N", CFGS)
@pytest.mark.parametrize("mode", [False, True], ids=["shared", "inst"])
def test_oracle_projection_ties_bit_exact_vs_compiled_reference(oracle_mod, tinympc, dt, nx, nu, N, mode):
    """The crafted bounds through the compiled reference (oracle/_ref) and the oracle: every bit, zero signs included."""
    O = oracle_mod
    if not O.have_ref(dt, nx, nu, N):
        pytest.skip("oracle/_ref not built here (needs /root/reference)")
    prob = projection_problem(tinympc.problems, O, nx, nu, N)
    case = projection_case(O, prob, 12, dt, nx + nu + N, mode)
    for settings in (dict(PROJ_EXACT, max_iter=1), dict(PROJ_EXACT, max_iter=6), dict(max_iter=12, check_termination=3)):
        a, b = O.copy_state(case["st0"]), O.copy_state(case["st0"])
        ra = O.Oracle(prob, dt, settings).solve(a, *case["bnds"], case["xref"])
        rb = O.Reference(prob, dt, settings).solve(b, *case["bnds"], case["xref"])
        assert ra == rb
        for k in STATE_ORDER + ("residuals", "status", "iter"):
            assert same_bits(a[k], b[k]), (settings, k)


@pytest.mark.parametrize("key", PROJ_INPUTS[:3] + PROJ_INPUTS[8:9], ids=IDS[:3] + IDS[8:9])
def test_med3_model_differs_from_the_reference_in_two_zero_sign_combinations_only(oracle_mod, tinympc, key):
    """What the GPU result is checked for.  v_med3_f32(t, min(lo, hi), hi) as the ISA manual states it (max / min that order -0 below +0) equals the
    reference's projection in value everywhere and in the sign of a zero everywhere but: t = +0 on lo = -0 (reference -0, med3 +0; decided there, i.e.
    hi > 0) and t = -0 on hi = +0 (reference +0, med3 -0; with lo below or at -0).  A model of arithmetic: nothing here looks at a kernel."""
    O = oracle_mod
    prob, case = projection_input(tinympc.problems, O, key)
    st = iteration_one(O, prob, key[4], case)
    for new, t, lo, hi in ((st["vnew"], case["t"][0], *case["bnds"][:2]), (st["znew"], case["t"][1], *case["bnds"][2:])):
        lo, hi = full(lo, t), full(hi, t)
        m = med3_model(t, lo, hi)
        assert np.array_equal(m, new)                                      # no value differs
        differs = np.signbit(m) != np.signbit(new)
        neg0 = lambda a: (a == 0) & np.signbit(a)
        pos0 = lambda a: (a == 0) & ~np.signbit(a)
        low = pos0(t) & neg0(lo) & (hi > 0)
        high = neg0(t) & pos0(hi) & ((lo < 0) | neg0(lo))
        assert low.sum() >= 2 and high.sum() >= 2
        assert np.array_equal(differs, low | high)
        assert np.all(neg0(new[low]) & pos0(m[low])) and np.all(pos0(new[high]) & neg0(m[high]))
