"""GPU tests of the box projection at its edges (admm.cpp:51-60), one case per projection site of the kernels: pre-projection values that equal a
bound, bounds of +0 and -0 under zeros of both signs, lo == hi, lo > hi, infinite bounds (tests/helpers.py: projection_case; what those inputs
reach is asserted on the CPU in tests/test_projection_host.py).  Exact arithmetic: every bit of the oracle's result, zero signs included."""
import numpy as np
import pytest

from helpers import PROJ_EXACT, PROJ_INPUTS, STATE_ORDER, bounds_of, projection_input, same_bits

pytestmark = pytest.mark.gpu

SCALARS = ("residuals", "iter", "status")
SETTINGS = (dict(max_iter=1), dict(max_iter=6), dict(max_iter=6, en_input_bound=0), dict(max_iter=6, en_state_bound=0))
F32, F64 = np.float32, np.float64

# what runs -> (kernel_name() expected, input set of helpers.PROJ_INPUTS, select_kernel, set_row_kernel, storage or None, options)
# options: "ref": one shared reference (tile16's shared-table instantiation needs it; t does not depend on the reference), "defuse": the bounds with every
# lo = -0 turned into +0 and every hi = +0 into -0 — the zeros on which v_med3_f32 and the reference agree — so that the handle stays on the matrix-core
# kernels, which keep the median: as crafted, an exact handle is handed over to the next exact family (tinympc_batch.h), asserted here by name
Q10, Q10I, Q10C = (12, 4, 10, 21, F32, False), (12, 4, 10, 21, F32, True), (12, 4, 10, 21, F32, "const")
W, WI, T48, T48I = (16, 4, 10, 20, F32, False), (16, 4, 10, 20, F32, True), (32, 16, 6, 19, F32, False), (32, 16, 6, 19, F32, True)
CASES = {
    "rowlane-12-4-10/shared": ("rowlane<12,4,10,exact>", Q10, 2, 1, None, ""),             # bounds from the LDS table
    "rowlane-12-4-10/inst": ("rowlane<12,4,10,exact>", Q10I, 2, 1, None, ""),              # ... from the look-ahead queue, its clamp at step N-1 included
    "rowlane-8-3-7/shared": ("rowlane<8,3,7,exact>", (8, 3, 7, 22, F32, False), 2, 1, None, ""),
    "rowloop-4-2/shared": ("rowloop<4,2,exact>", (4, 2, 8, 20, F32, False), 2, 2, None, ""),
    "rowloop-4-2/inst": ("rowloop<4,2,exact>", (4, 2, 8, 20, F32, True), 2, 2, None, ""),
    "rowstream-8-4/shared": ("rowstream<8,4,exact>", (8, 4, 9, 20, F32, False), 2, 3, None, ""),
    "rowstream-8-4/inst": ("rowstream<8,4,exact>", (8, 4, 9, 20, F32, True), 2, 3, None, ""),
    "quadlane-4-1-10/shared": ("quadlane<4,1,10,exact>", (4, 1, 10, 28, F32, False), 2, 4, None, ""),
    "tile16/shared/defused": ("tile16<12,4,10,exact>", Q10, 2, 5, None, "ref defuse"),
    "tile16/const/defused": ("tile16<12,4,10,exact,pi>", Q10C, 2, 5, None, "defuse"),        # one resident row of bounds per instance
    "tile16/inst/defused": ("tile16<12,4,10,exact,pi>", Q10I, 2, 5, None, "defuse"),         # the ring of step slots
    "tile16/shared/handed-over": ("rowlane<12,4,10,exact>", Q10, 2, 5, None, "ref"),
    "tile16/const/handed-over": ("rowlane<12,4,10,exact>", Q10C, 2, 5, None, ""),
    "tile16/inst/handed-over": ("rowlane<12,4,10,exact>", Q10I, 2, 5, None, ""),
    "waveres-16-4/shared": ("waveres<16,4,exact>", W, 2, 7, None, ""),
    "waveres-16-4/inst": ("waveres<16,4,exact>", WI, 2, 7, None, ""),
    "wavestream-16-4/shared": ("wavestream<16,4,exact>", W, 2, 6, None, ""),
    "wavestream-16-4/inst": ("wavestream<16,4,exact>", WI, 2, 6, None, ""),
    "tile48/shared/defused": ("tile48<32,16,6,exact>", T48, 2, 8, None, "defuse"),
    "tile48/inst/defused": ("tile48<32,16,6,exact>", T48I, 2, 8, None, "defuse"),
    "tile48/shared/handed-over": ("waveres<32,16,exact>", T48, 2, 8, None, ""),
    "tile48/inst/handed-over": ("waveres<32,16,exact>", T48I, 2, 8, None, ""),
    "generic-3-2/inst": ("generic<3,2,exact>", (3, 2, 6, 20, F32, True), 0, None, None, ""),
    "generic-8-8/shared": ("generic<8,8,exact>", (8, 8, 6, 20, F32, False), 0, None, None, ""),
    "rows64-12-4-10/shared": ("rows64<12,4,10>", (12, 4, 10, 20, F64, False), 0, None, None, ""),
    "rows64-12-4-10/inst": ("rows64<12,4,10>", (12, 4, 10, 20, F64, True), 0, None, None, ""),
    "rows64-4-2/shared": ("rows64<4,2,n<=32>", (4, 2, 8, 20, F64, False), 0, None, None, ""),
    "rows64-4-2/inst": ("rows64<4,2,n<=32>", (4, 2, 8, 20, F64, True), 0, None, None, ""),
    "thread64-12-4/shared": ("thread64<12,4>", (12, 4, 10, 20, F64, False), 1, None, None, ""),
    "thread64-12-4/inst": ("thread64<12,4>", (12, 4, 10, 20, F64, True), 1, None, None, ""),
    "h16/shared": (",h16>", (12, 4, 10, 20, "h16", False), 2, 0, (16, 16), ""),              # fp16 storage, both dual precisions
    "h16d/shared": (",h16d>", (12, 4, 10, 20, "h16d", False), 2, 0, (16, 32), ""),
}


def defused(lo, hi):
    """the zero bounds on which the median and the compare-selects agree: lo = +0, hi = -0; where both are zero (the table would store min(lo, hi) = -0 for
    lo) the lower bound steps just below"""
    lo, hi = lo.copy(), hi.copy()
    lo[lo == 0] = 0.0
    hi[hi == 0] = -0.0
    lo[(lo == 0) & (hi == 0)] = -2.0 ** -60
    return lo, hi


def assert_bits(got, ref, what):
    for k in STATE_ORDER + SCALARS:
        if not same_bits(got[k], ref[k]):
            bad = (got[k] != ref[k]) | ((np.signbit(got[k]) != np.signbit(ref[k])) if got[k].dtype.kind == "f" else False)
            where = np.argwhere(bad)
            i = tuple(where[0])
            only_signs = bool(np.array_equal(got[k], ref[k]))
            raise AssertionError(f"{what}: {k} differs from the oracle in {len(where)} entries ({'zero signs only' if only_signs else 'values'}), "
                                 f"first at {i}: {got[k][i]!r} for {ref[k][i]!r}")


def make(T, prob, key, sel, fam, storage, settings):
    dtype = key[4]
    if dtype is F64:
        sol = T.TinyBatchSolver64(prob, key[3], settings=settings)
        sol.select_kernel(sel)
    else:
        sol = T.TinyBatchSolver(prob, key[3], settings=settings)
        sol.select_kernel(sel)
        if storage:
            sol.set_storage(*storage)
        if fam is not None:
            sol.set_row_kernel(fam)
    return sol


@pytest.mark.parametrize("name", list(CASES))
def test_projection_edges_bitwise(tinympc, oracle_mod, name):
    """One projection site: iteration 1 alone (the crafted ties), six iterations, and each bound switched off, tolerances 0 — all twelve arrays,
    the residuals, iter, status and the return code against the oracle.  Under fp16 storage one lower bound is -1e-9, which the table stores as -0.
    Measured on an MI355X before the kernels were changed: v_med3_f32 does what the ISA manual says (tests/test_projection_host.py states the model);
    every kernel that projected with it returned +0 for the reference's -0 (t = +0 on lo = -0) and -0 for +0 (t = -0 on hi = +0) and nothing else
    differed; the run-time-dimension kernel and the fp64 library, which restate the compare-selects, agreed with the oracle in every bit."""
    O, T = oracle_mod, tinympc
    want, key, sel, fam, storage, options = CASES[name]
    prob, case = projection_input(T.problems, O, key)
    dtype = key[4]
    bnds = [b.copy() for b in case["bnds"]]
    if "defuse" in options:
        bnds = [*defused(*bnds[:2]), *defused(*bnds[2:])]
    xref = case["xref"][2] if "ref" in options else case["xref"]            # instance 2's: zeros of random sign
    R = (lambda a: a)
    if storage:
        R = O.round_h16
        zero_t = np.argwhere((case["t"][1][:case["Z"]] == 0).all(axis=0))[-1]      # an input entry where the zero instances sit on the bound
        bnds[2][tuple(zero_t)] = -1e-9
        assert R(bnds[2])[tuple(zero_t)] == 0 and np.signbit(R(bnds[2])[tuple(zero_t)])
    sol = make(T, prob, key, sel, fam, storage, dict(PROJ_EXACT, max_iter=1, en_state_bound=1, en_input_bound=1))
    try:
        sol.set_bounds(*bnds)
        sol.set_xref(xref)
        for over in SETTINGS:
            settings = {**PROJ_EXACT, "en_state_bound": 1, "en_input_bound": 1, **over}
            sol.set_settings(**settings)
            kn = sol.kernel_name()
            assert kn == want or (storage and kn.endswith(want)), (kn, want)
            sol.set_state(case["st0"])
            rc = sol.solve()
            got = sol.get_state()
            st = O.copy_state(case["st0"])
            hit = O.Oracle(prob, dtype, settings).solve(st, *[R(b) for b in bnds], xref, nthreads=4)
            assert_bits(got, st, f"{kn} {over}")
            assert rc == (1 if hit else 0), (kn, over, rc, hit)
    finally:
        sol.close()


@pytest.mark.parametrize("dims", [(12, 4, 10), (4, 1, 10)])
def test_update_slack_alone_on_exact_ties(tinympc, oracle_mod, dims):
    """tiny_batch_update_slack as a call of its own (the step kernel's own projection): y = g = 0 with u and x set to the bounds themselves, so that
    every entry ties by construction — instance by instance on the lower bound, on the upper bound, on -0 / +0 under a zero bound of the other sign."""
    O, T = oracle_mod, tinympc
    nx, nu, N = dims
    prob = T.problems.quadrotor(20, N) if nx == 12 else T.problems.cartpole(N, riccati=O.riccati)
    B = 8
    rng = np.random.default_rng(nx)
    xmn, xmx, umn, umx = (np.repeat(b[None], B, axis=0) * rng.uniform(0.1, 1.0, size=(B,) + b.shape).astype(F32) for b in bounds_of(prob, F32))
    st = O.new_state(B, nx, nu, N)
    for k in STATE_ORDER:
        st[k][:] = (rng.standard_normal(st[k].shape) * 0.3).astype(F32)
    st["y"][:] = 0; st["g"][:] = 0
    st["x"][0::4], st["u"][0::4] = xmn[0::4], umn[0::4]                       # on the lower bound
    st["x"][1::4], st["u"][1::4] = xmx[1::4], umx[1::4]                       # on the upper bound
    xmn[2::4], umn[2::4], st["x"][2::4], st["u"][2::4] = -0.0, -0.0, 0.0, 0.0   # +0 on a lower bound of -0
    xmx[3::4], umx[3::4], st["x"][3::4], st["u"][3::4] = 0.0, 0.0, -0.0, -0.0   # -0 on an upper bound of +0
    st["y"][2::4] = 0.0; st["g"][2::4] = 0.0; st["y"][3::4] = -0.0; st["g"][3::4] = -0.0   # t = u + y, x + g keeps the sign
    xref = np.zeros((N, nx), F32)
    sol = T.TinyBatchSolver(prob, B, settings=dict(O.DEFAULT_SETTINGS))
    try:
        sol.select_kernel(2)
        sol.set_bounds(xmn, xmx, umn, umx); sol.set_xref(xref)
        sol.set_state(st)
        sol.update_slack()
        got = sol.get_state()
        O.Oracle(prob, F32).step("update_slack", st, xmn, xmx, umn, umx, xref)
        assert same_bits(st["znew"][0::4], umn[0::4]) and same_bits(st["vnew"][1::4], xmx[1::4])      # the ties are ties
        assert np.signbit(st["znew"][2::4]).all() and not np.signbit(st["vnew"][3::4]).any()          # the reference's rule: the bound wins a tie
        assert_bits(got, st, f"update_slack alone {dims}")
    finally:
        sol.close()


@pytest.mark.parametrize("key", [PROJ_INPUTS[0], PROJ_INPUTS[1]], ids=["shared", "inst"])
def test_projection_edges_fma_kernels(tinympc, oracle_mod, key):
    """Fma arithmetic keeps v_med3_f32 (no bitwise contract with the reference): rowlane and tile16 `fast` stay bitwise equal to each other, every
    enabled entry of znew and vnew lies in [min(lo, hi), hi], and a side whose bound is switched off is untouched: znew == u + y, vnew == x + g of the
    live-in duals after one iteration."""
    O, T = oracle_mod, tinympc
    prob, case = projection_input(T.problems, O, key)
    xmn, xmx, umn, umx = (np.broadcast_to(b, (key[3],) + b.shape[-2:]) for b in case["bnds"])
    for over in SETTINGS + (dict(max_iter=1, en_input_bound=0), dict(max_iter=1, en_state_bound=0)):
        settings = {**PROJ_EXACT, "en_state_bound": 1, "en_input_bound": 1, **over}
        outs = []
        for fam in (1, 5):
            sol = T.TinyBatchSolver(prob, key[3], settings=settings)
            try:
                sol.select_kernel(3); sol.set_row_kernel(fam)
                sol.set_bounds(*case["bnds"]); sol.set_xref(case["xref"] if key[5] else case["xref"][2])   # (a shared table goes with one shared reference)
                kn = sol.kernel_name()
                assert kn == ("rowlane<12,4,10,fast>" if fam == 1 else "tile16<12,4,10,fast,pi>" if key[5] else "tile16<12,4,10,fast>"), kn
                sol.set_state(case["st0"])
                outs.append((sol.solve(), sol.get_state()))
            finally:
                sol.close()
        (ra, a), (rb, b) = outs
        assert ra == rb
        assert_bits(b, a, f"tile16 fast against rowlane fast {over}")
        if settings["en_state_bound"]:
            assert ((a["vnew"] >= np.minimum(xmn, xmx)) & (a["vnew"] <= xmx)).all(), over
        elif over["max_iter"] == 1:
            assert same_bits(a["vnew"], a["x"] + case["st0"]["g"]), over
        if settings["en_input_bound"]:
            assert ((a["znew"] >= np.minimum(umn, umx)) & (a["znew"] <= umx)).all(), over
        elif over["max_iter"] == 1:
            assert same_bits(a["znew"], a["u"] + case["st0"]["y"]), over
