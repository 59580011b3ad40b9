"""The fma-order mode of the CPU oracle (oracle/tinympc_oracle_impl.h, ORACLE_FMA; Oracle(..., arith="fma")), checked WITHOUT a GPU and without
the kernels it restates — the device side of the same statement is tests/test_fma_oracle_gpu.py.

  * inputs on which no operation rounds: the fma oracle must equal the EXACT oracle in value (a fused multiply-add and a multiply followed by an
    add coincide there).  Says nothing about the summation order; catches the indexing, sign and which-matrix-where mistakes of a restatement.
  * ordinary inputs: the fma oracle against the exact fp32 oracle passes the bar the GPU fma kernels are held to (compare_states with the
    reference's own fp64-vs-fp32 spread as the yardstick).  No tolerance of its own.
  * the same bytes whatever the thread count; with fp16 storage every array left behind is representable in binary16.
  * what the inputs of tests/test_fma_values_gpu.py are worth (helpers.FMA_VALUE_CASES, the list that file parametrises over): nothing rounds, in the
    oracle's order or in any other; removing any single term of any matrix changes an output; both projections bind and are slack.
"""
import numpy as np
import pytest

import helpers as H
from helpers import STATE_ORDER, rounding_free_case

ALL = STATE_ORDER + ("residuals", "iter", "status")


def _solve(O, prob, dtype, settings, x0, xref, bnds, uref, arith="exact", nthreads=1):
    dt = np.float64 if dtype == np.float64 else np.float32
    # fp64 serves only as the proof that nothing rounds, where the order of a sum is immaterial: every dimension is accepted
    orc = O.Oracle(prob, dtype, settings, arith=arith, allow_unpinned_dims=dtype == np.float64)
    orc.set_uref(None if uref is None else np.asarray(uref, dt))
    st = O.new_state(len(x0), prob["nx"], prob["nu"], prob["N"], dt)
    st["x"][:, 0] = x0
    rc = orc.solve(st, *[np.asarray(b, dt) for b in bnds], np.asarray(xref, dt), nthreads=nthreads)
    return rc, st


@pytest.mark.parametrize("terms", [False, True])
@pytest.mark.parametrize("max_iter", [1, 2])
@pytest.mark.parametrize("dims", [(12, 4, 10), (8, 3, 7), (4, 1, 10), (2, 2, 3)])
def test_fma_oracle_equals_exact_oracle_where_nothing_rounds(oracle_mod, dims, max_iter, terms):
    """Signed selection matrices and small integers (helpers.rounding_free_case), one and two iterations, with and without the Uref and coeff_d2p
    terms.  Premises asserted here: the fp32 exact oracle equals the fp64 exact oracle (nothing rounded), and over the iterations the projection of
    the inputs binds somewhere and is slack somewhere (y = (u + y) - znew is non-zero exactly where it bound).  Values only: the negated gains of the fma
    mode legitimately flip signs of zeros."""
    O = oracle_mod
    nx, nu, N = dims
    prob, settings, x0, xref, bnds, uref = rounding_free_case(nx, nu, N, 8, seed=0, terms=terms)
    settings = dict(settings, max_iter=max_iter)
    rc32, e32 = _solve(O, prob, np.float32, settings, x0, xref, bnds, uref)
    rc64, e64 = _solve(O, prob, np.float64, settings, x0, xref, bnds, uref)
    for k in ALL:
        assert np.array_equal(e32[k], e64[k]), f"{dims} max_iter={max_iter}: the premise fails, {k} rounds in fp32"
    assert rc32 == rc64
    assert float(max(np.abs(e64[k]).max() for k in STATE_ORDER)) < 2.0 ** 24
    # the projections of iteration m are the last ones of a solve with max_iter = m
    bound = np.stack([_solve(O, prob, np.float32, dict(settings, max_iter=m), x0, xref, bnds, uref)[1]["y"] != 0 for m in range(1, max_iter + 1)])
    assert bound.any() and (~bound).any(), f"{dims} max_iter={max_iter}: binding {int(bound.sum())} of {bound.size} input projections"
    rcf, f = _solve(O, prob, np.float32, settings, x0, xref, bnds, uref, arith="fma")
    assert rcf == rc32
    for k in ALL:
        assert np.array_equal(f[k], e32[k]), f"{dims} max_iter={max_iter} terms={terms}: {k} of the fma oracle differs from the exact oracle"


@pytest.mark.parametrize("case", ["quad10", "cartpole10", "random_8_3_7"])
def test_fma_oracle_lies_inside_the_yardstick(oracle_mod, tinympc, case):
    """A cold solve and two warm solves (duals reset) of 64 instances: the fma oracle against the exact fp32 oracle, from the same live-in, under
    compare_states with the fp64 oracle as the yardstick — the bar of the GPU fma kernels, unchanged."""
    import test_parity_gpu as P
    O, pr = oracle_mod, tinympc.problems
    prob = {"quad10": lambda: pr.quadrotor(20, 10), "cartpole10": lambda: pr.cartpole(10, riccati=O.riccati),
            "random_8_3_7": lambda: pr.random_system(8, 3, 7, seed=99, riccati=O.riccati)}[case]()
    nx, nu, N, B = prob["nx"], prob["nu"], prob["N"], 64
    rng = np.random.default_rng(N + nx)
    x0 = rng.uniform(-0.3, 0.3, size=(B, nx)).astype(np.float32)
    xref = (rng.standard_normal((B, N, nx)) * 0.1).astype(np.float32)
    bnds = pr.bounds_arrays(prob)
    settings = dict(O.DEFAULT_SETTINGS, max_iter=60)
    exact, fma = O.Oracle(prob, np.float32, settings), O.Oracle(prob, np.float32, settings, arith="fma")
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = x0
    for k in range(3):
        st["y"][:] = 0; st["g"][:] = 0
        pre = O.copy_state(st)
        got = O.copy_state(st)
        exact.solve(st, *bnds, xref, nthreads=8)
        fma.solve(got, *bnds, xref, nthreads=8)
        assert any(not np.array_equal(got[a], st[a]) for a in STATE_ORDER), "the fma mode rounds nowhere differently: not an fma mode"
        P.compare_states(got, st, prob, f"{case} solve {k}", ref64=P.yardstick(O, prob, settings, pre, xref, bnds))


@pytest.mark.parametrize("dtype", [np.float32, "h16", "h16d"])
def test_fma_oracle_is_deterministic_and_keeps_the_storage_grid(oracle_mod, tinympc, dtype):
    """One thread and eight threads leave identical bytes; the fp16-storage instantiations leave only binary16 values (the duals of "h16d"
    excepted, which stay fp32), as tests/test_oracle.py asserts of the exact ones."""
    O, pr = oracle_mod, tinympc.problems
    prob = pr.quadrotor(20, 10)
    B = 37
    R = O.round_h16 if isinstance(dtype, str) else (lambda a: np.asarray(a, np.float32))
    rng = np.random.default_rng(3)
    x0 = R(rng.uniform(-0.3, 0.3, size=(B, 12)))
    xref = R(rng.standard_normal((B, 10, 12)) * 0.1)
    bnds = tuple(R(b) for b in pr.bounds_arrays(prob))
    outs = [_solve(O, prob, dtype, dict(O.DEFAULT_SETTINGS, max_iter=30), x0, xref, bnds, None, arith="fma", nthreads=n) for n in (1, 8)]
    (rc1, a), (rc8, b) = outs
    assert rc1 == rc8
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert len(set(a["iter"].tolist())) > 1, "every instance runs the same number of iterations"
    if isinstance(dtype, str):
        for k in STATE_ORDER:
            if not (dtype == "h16d" and k in ("g", "y")):
                assert np.array_equal(a[k], O.round_h16(a[k])), k


# ---- the inputs of tests/test_fma_values_gpu.py ---------------------------------------------------------------------------------------------------

MATRICES = ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn")
# one entry per distinct input set and iteration count of the list the GPU file runs (several kernels share some); the largest batch stands for the
# smaller ones, which are its first instances
VALUE_INPUTS = {}
for _c in H.FMA_VALUE_CASES:
    for _mi in _c["max_iters"]:
        VALUE_INPUTS.setdefault("{}-{}-{}-{}-it{}".format(_c["gen"], "_".join(map(str, _c["dims"])), _c["bounds"], _c["ref"], _mi), (_c, _mi))


def _any_order_bound(prob, st, xref):
    """The largest sum of |terms| of any sum the solve forms from the arrays it left behind ([B] of them, prob one model): while that stays below 2^24
    every partial sum of every order is an exactly representable integer, so a kernel that sums in an order of its own (or splits a sum over lanes or
    MFMA passes) cannot round either.  The sums of an earlier iteration are those of the solve with a smaller max_iter."""
    a = {k: np.abs(np.asarray(prob[k], np.float64)) for k in MATRICES}
    s = {k: np.abs(np.asarray(st[k], np.float64)) for k in STATE_ORDER}
    xr = np.abs(np.asarray(xref, np.float64)) * np.ones_like(s["x"])
    inner = s["p"][:, 1:] @ a["Bdyn"] + s["r"]                                                   # Bdyn' p + r
    sums = [s["x"][:, :-1] @ a["Kinf"].T + s["d"],                                               # u = -Kinf x - d
            s["x"][:, :-1] @ a["Adyn"].T + s["u"] @ a["Bdyn"].T,                                  # x+ = Adyn x + Bdyn u
            inner @ a["Quu_inv"].T,                                                              # d = Quu_inv (Bdyn' p + r)
            s["q"][:, :-1] + s["p"][:, 1:] @ a["AmBKt"].T + s["r"] @ a["Kinf"],                  # p = q + AmBKt p+ - Kinf' r
            xr[:, -1] @ a["Pinf"] + s["vnew"][:, -1] + s["g"][:, -1],                            # p_N = -Pinf' xref_N - rho (vnew_N - g_N)
            xr * np.abs(prob["Q"]) + s["vnew"] + s["g"], s["znew"] + s["y"], s["u"] + s["y"], s["x"] + s["g"]]
    return max(float(v.max()) for v in sums)


@pytest.mark.parametrize("key", list(VALUE_INPUTS))
def test_value_case_inputs_round_nowhere_and_bind_in_part(oracle_mod, key):
    """Premise, structure and both sides of both projections, for one input set of helpers.FMA_VALUE_CASES at its largest batch."""
    O = oracle_mod
    c, mi = VALUE_INPUTS[key]
    probs, settings, x0, xref, bnds = H.value_case_inputs(c)
    settings = dict(settings, max_iter=mi)
    assert settings["abs_pri_tol"] == settings["abs_dua_tol"] == 0.0 and settings["check_termination"] == 1
    assert settings["en_state_bound"] == settings["en_input_bound"] == 1
    models = probs if isinstance(probs, list) else [probs]
    nx, nu, N = c["dims"]
    xr = H.ref_at(xref, 0, 0, N, len(x0))
    for a in (x0, xr) + tuple(bnds) + tuple(np.asarray(p["Q"]) for p in models):
        assert np.array_equal(a, np.round(a)), "an input that is no integer"
    for p in models:
        assert p["rho"] == 1.0
        for k in MATRICES:
            m = np.asarray(p[k])
            assert np.isin(m, (-1.0, 0.0, 1.0)).all()
            if c["gen"].startswith("dense"):   # the structure: two terms in every row that has two columns, no column of zeros
                assert ((m != 0).sum(axis=1) >= min(2, m.shape[1])).all() and (m != 0).any(axis=0).all(), (key, k)
    # the premise: fp32 == fp64, every magnitude and every sum of |terms| below 2^24, in every iteration run
    rc32, e32 = H.value_case_oracle(O, probs, np.float32, settings, x0, xref, bnds)
    rc64, e64 = H.value_case_oracle(O, probs, np.float64, settings, x0, xref, bnds)
    for k in ALL:
        assert np.array_equal(e32[k], e64[k]), f"{key}: the premise fails, {k} rounds in fp32"
    assert rc32 == rc64
    assert (e32["iter"] == mi).all()
    u_share, x_share, largest, any_order = [], [], 0.0, 0.0
    for m in range(1, mi + 1):
        st = e64 if m == mi else H.value_case_oracle(O, probs, np.float64, dict(settings, max_iter=m), x0, xref, bnds)[1]
        largest = max(largest, max(float(np.abs(st[k]).max()) for k in STATE_ORDER))
        for b in range(len(x0) if isinstance(probs, list) else 1):
            sel = slice(b, b + 1) if isinstance(probs, list) else slice(None)
            any_order = max(any_order, _any_order_bound(models[b], {k: st[k][sel] for k in STATE_ORDER}, xr[sel] if xr.ndim == 3 else xr))
        u_share.append(float((st["y"] != 0).mean())); x_share.append(float((st["g"] != 0).mean()))   # y, g = what the projection of iteration m cut off
    assert largest < 2.0 ** 24 and any_order < 2.0 ** 24, (key, largest, any_order)
    assert any(0.05 <= s <= 0.95 for s in u_share), f"{key}: the input projection binds on {u_share} of the entries"
    assert any(0.05 <= s <= 0.95 for s in x_share), f"{key}: the state projection binds on {x_share} of the entries"
    # the fma oracle: the same values
    rcf, f = H.value_case_oracle(O, probs, np.float32, settings, x0, xref, bnds, arith="fma")
    assert rcf == rc32
    for k in ALL:
        assert np.array_equal(f[k], e32[k]), f"{key}: {k} of the fma oracle differs from the exact oracle"


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k]) for k in ALL)


def _instances(sel, x0, xr, bnds):
    """(x0, xr, bnds) of the instances sel (a slice): what is shared stays whole"""
    return x0[sel], xr[sel] if xr.ndim == 3 else xr, tuple(a[sel] if a.ndim == 3 else a for a in bnds)


def _without_entry(model, k, r, col):
    m = np.array(model[k])
    m[r, col] = 0.0
    return dict(model, **{k: m})


def _entries(model):
    """(matrix, row, column) of every non-zero entry of a model"""
    return [(k, int(r), int(col)) for k in MATRICES for r, col in np.argwhere(np.asarray(model[k]) != 0)]


def _hidden_entries_of_a_shared_model(O, prob, settings, inputs, B):
    """the entries whose removal changes no output of any instance; most show in the first six instances already, the whole batch runs for the rest"""
    groups = [slice(0, min(6, B)), slice(0, B)]
    solve = lambda model, sel: H.value_case_oracle(O, model, np.float32, settings, *_instances(sel, *inputs))[1]
    full = [solve(prob, sel) for sel in groups]
    return [e for e in _entries(prob) if not any(_differs(solve(_without_entry(prob, *e), sel), want) for sel, want in zip(groups, full))]


def _hidden_entries_of_instance_models(O, probs, settings, inputs):
    """per instance b, the entries of ITS model whose removal changes no output of instance b, the only one that reads them"""
    hidden = []
    for b, model in enumerate(probs):
        mine = _instances(slice(b, b + 1), *inputs)
        solve = lambda m: H.value_case_oracle(O, [m], np.float32, settings, *mine)[1]
        want = solve(model)
        hidden += [("instance", b) + e for e in _entries(model) if not _differs(solve(_without_entry(model, *e)), want)]
    return hidden


def _unseen_neighbour_matrices(O, probs, settings, inputs):
    """the mix-up that is a record kernel's own: matrix k of instance b taken from the record on either side.  Listed where instance b's outputs do
    not change although the two matrices differ."""
    B, unseen = len(probs), []
    solve = lambda models: H.value_case_oracle(O, models, np.float32, settings, *inputs)[1]
    full = solve(probs)
    for k in MATRICES:
        for shift in (1, -1):
            theirs = [probs[(b + shift) % B][k] for b in range(B)]
            st = solve([dict(p, **{k: m}) for p, m in zip(probs, theirs)])
            for b in range(B):
                unchanged = not _differs({a: st[a][b] for a in ALL}, {a: full[a][b] for a in ALL})
                if unchanged and not np.array_equal(probs[b][k], theirs[b]):
                    unseen.append((k, "of instance", (b + shift) % B, "in instance", b))
    return unseen


@pytest.mark.parametrize("key", list(VALUE_INPUTS))
def test_value_case_inputs_show_every_term(oracle_mod, key):
    """Every non-zero entry of every matrix, set to zero on its own, changes a compared output of an instance that reads it: a kernel that drops or
    misplaces any single term of any product cannot equal the oracle on these inputs.  Per-instance models: every entry of every instance's own model
    changes that instance's outputs; and so, as a further check, does every matrix taken from the neighbouring record."""
    O = oracle_mod
    c, mi = VALUE_INPUTS[key]
    probs, settings, x0, xref, bnds = H.value_case_inputs(c)
    settings = dict(settings, max_iter=mi)
    inputs = (x0, H.ref_at(xref, 0, 0, c["dims"][2], len(x0)), bnds)
    if isinstance(probs, list):
        hidden = _hidden_entries_of_instance_models(O, probs, settings, inputs) + _unseen_neighbour_matrices(O, probs, settings, inputs)
    else:
        hidden = _hidden_entries_of_a_shared_model(O, probs, settings, inputs, len(x0))
    assert not hidden, f"{key}: {len(hidden)} terms change nothing, the first {hidden[:5]}"


def test_value_cases_name_every_kernel_of_the_list():
    """the fma code that had the yardstick bar alone"""
    names = {c["kernel"] for c in H.FMA_VALUE_CASES}
    for want in ("quadlane<4,1,10,fast>", "waveres<32,16,fast>", "waveres<16,8,fast>", "waveres<20,8,fast>", "waveres<16,4,fast>", "waveres<24,4,fast>",
                 "tile48<32,16,4,fast>", "tile48<32,16,5,fast>", "stream<3,1>", "stream<1,1>", "stream<2,1>", "stream<8,4>", "stream<16,8>",
                 "rowlane<12,4,10,fast,pm>", "rowlane<8,3,7,fast,pm>", "waveres<32,16,fast,pm>", "waveres<16,8,fast,pm>"):
        assert want in names, want
    padded = {c["dims"][:2] for c in H.STREAM_VALUE_CASES}
    assert {(12, 4), (4, 1), (8, 4), (32, 16), (64, 32), (5, 5), (33, 17), (10, 3), (6, 2)} <= padded


def test_quadlane_loop_inputs_round_nowhere(oracle_mod):
    """The closed loop of helpers.QUADLANE_LOOP_CASE on the oracle, in fp32 and in fp64: u.col(0), iter and status of every step, the final plant
    state and the final workspace are equal, and nothing comes near 2^24 (through the dense matrices the second step already rounds: the sparse ones)."""
    O = oracle_mod
    c = H.QUADLANE_LOOP_CASE
    prob, settings, x0, xref, bnds = H.value_case_inputs(c)
    settings = dict(settings, max_iter=c["max_iters"][0])
    a = H.oracle_closed_loop(O, prob, np.float32, settings, x0, xref, bnds, c["steps"], 0)
    b = H.oracle_closed_loop(O, prob, np.float64, settings, x0, xref, bnds, c["steps"], 0)
    for k in ("u0", "iter", "status", "x"):
        assert np.array_equal(a[k], b[k]), k
    for k in ALL:
        assert np.array_equal(a["st"][k], b["st"][k]), f"the premise fails, {k} rounds in fp32"
    assert max(float(np.abs(b["st"][k]).max()) for k in STATE_ORDER) < 2.0 ** 20
    assert (b["u0"] != 0).any() and len(np.unique(b["u0"][-1])) > 2
