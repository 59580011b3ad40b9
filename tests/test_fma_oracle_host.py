"""The fma-order mode of the CPU oracle (oracle/tinympc_oracle_impl.h, ORACLE_FMA; Oracle(..., arith="fma")), checked WITHOUT a GPU and without
the kernels it restates — the device side of the same statement is tests/test_fma_oracle_gpu.py.

  * inputs on which no operation rounds: the fma oracle must equal the EXACT oracle in value (a fused multiply-add and a multiply followed by an
    add coincide there).  Says nothing about the summation order; catches the indexing, sign and which-matrix-where mistakes of a restatement.
  * ordinary inputs: the fma oracle against the exact fp32 oracle passes the bar the GPU fma kernels are held to (compare_states with the
    reference's own fp64-vs-fp32 spread as the yardstick).  No tolerance of its own.
  * the same bytes whatever the thread count; with fp16 storage every array left behind is representable in binary16.
"""
import numpy as np
import pytest

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
