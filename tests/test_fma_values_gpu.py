"""The fma kernels that sum in orders of their own — quadlane, waveres, tile48, the MFMA streaming kernel with the padded classes it serves, and the
per-instance-model records — against the EXACT fp32 oracle BY VALUE, on inputs where no operation rounds (helpers.rounding_free_dense_case; where
its values outgrow fp32, helpers.rounding_free_case): every operand is an integer, every matrix entry 0 or +-1 and rho 1, so a fused multiply-add, a
multiply followed by an add, an MFMA accumulation and every summation order give the same number.  One cold solve; all twelve work arrays, the four
residual fields, iter, status and the return code, of every instance, with np.array_equal: no mask, no tolerance, no share of instances left out.
Only the sign of a zero is excepted (the negated gains of the fma mode flip it).

What these inputs are worth is proven without a GPU in tests/test_fma_oracle_host.py, over the same list (helpers.FMA_VALUE_CASES): the fp32 oracle
equals the fp64 one and every sum of |terms| stays below 2^24 (nothing rounds in ANY order), removing any single entry of any matrix changes an output,
and both projections bind on a part of the entries and are slack on another.  A kernel that drops a term, reads a padding column as data, takes a gain
row from the neighbouring record or is off by one at the last horizon step is therefore wrong by an integer somewhere.
Every case asserts the name of the kernel it runs on and that it computes in fma arithmetic."""
import numpy as np
import pytest

import helpers as H
from helpers import STATE_ORDER
from test_fma_oracle_gpu import _handle, _named, same_bits
from test_parity_gpu import SCALARS

pytestmark = pytest.mark.gpu

_expected = {}


def _oracle(O, c, max_iter):
    """(settings, state) of the exact fp32 oracle on the case at its largest batch, computed once: the smaller batches are its first instances"""
    key = (H.value_case_id(c), max_iter)
    if key not in _expected:
        probs, settings, x0, xref, bnds = H.value_case_inputs(c)
        settings = dict(O.DEFAULT_SETTINGS, **settings, max_iter=max_iter)
        rc, st = H.value_case_oracle(O, probs, np.float32, settings, x0, xref, bnds)
        assert rc == len(x0), "an instance that does not run out of iterations at tolerance 0"   # so every batch returns 1
        _expected[key] = (settings, st)
    return _expected[key]


def _assert_values(got, want, B, what):
    for k in STATE_ORDER + SCALARS:
        g, w = np.asarray(got[k]), np.asarray(want[k][:B])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            i = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{what}: {k} differs from the exact oracle in {len(bad)} of {g.size} values, first at {i}: {g[i]} for {w[i]}")


@pytest.mark.parametrize("c", H.FMA_VALUE_CASES, ids=[H.value_case_id(c) for c in H.FMA_VALUE_CASES])
def test_fma_kernel_equals_the_exact_oracle_by_value(tinympc, oracle_mod, c):
    """every batch size and iteration count of one case of helpers.FMA_VALUE_CASES"""
    T, O = tinympc, oracle_mod
    for max_iter in c["max_iters"]:
        settings, want = _oracle(O, c, max_iter)
        for B in c["Bs"]:
            probs, _, x0, xref, bnds = H.value_case_inputs(c, B)
            pm = isinstance(probs, list)   # every instance its own model: the records go in before the routing
            sol = _handle(T, probs[0] if pm else probs, B, settings, c["select"], c["family"], bnds, xref, c["kernel"], models=H.models_of(probs) if pm else None)
            sol.set_x0(x0)
            assert sol.kernel_name() == c["kernel"], f"the case runs on {sol.kernel_name()}"
            _named(sol, c["kernel"])
            rc = sol.solve()
            _named(sol, c["kernel"])
            _assert_values(sol.get_state(), want, B, f"{c['kernel']} {c['dims']} B={B} max_iter={max_iter} bounds {c['bounds']} reference {c['ref']}")
            assert rc == 1, rc
            sol.close()


@pytest.mark.parametrize("B", H.QUADLANE_LOOP_CASE["Bs"])
def test_quadlane_closed_loop_equals_the_exact_oracle_loop_by_value(tinympc, oracle_mod, B):
    """quadlane's closed loop on chip (mpc_run_traj), two MPC steps of one iteration each, against helpers.oracle_closed_loop in exact fp32: u.col(0)
    of every step, the final plant state and the final workspace.  The premise — the fp32 loop equals the fp64 loop — is
    test_quadlane_loop_inputs_round_nowhere in tests/test_fma_oracle_host.py."""
    T, O = tinympc, oracle_mod
    c = H.QUADLANE_LOOP_CASE
    prob, settings, x0, xref, bnds = H.value_case_inputs(c, B)
    settings = dict(O.DEFAULT_SETTINGS, **settings, max_iter=c["max_iters"][0])
    want = H.oracle_closed_loop(O, prob, np.float32, settings, x0, xref, bnds, c["steps"], 0)
    sol = _handle(T, prob, B, settings, c["select"], c["family"], bnds, xref, c["kernel"])
    sol.set_x0(x0)
    _named(sol, c["kernel"])
    assert sol.closed_loop_kernel_name() == c["kernel"], sol.closed_loop_kernel_name()
    u = sol.mpc_run_traj(c["steps"], 0)
    assert u.shape == want["u0"].shape and np.array_equal(u, want["u0"]), f"B={B}: u.col(0) differs from step {int(np.argmax((u != want['u0']).any(axis=(1, 2))))} on"
    assert np.array_equal(sol.get_x0(), want["x"]), f"B={B}: the final plant state differs"
    got = sol.get_state()
    _assert_values(got, want["st"], B, f"{c['kernel']} closed loop B={B}: final workspace")
    assert same_bits(got["iter"], want["iter"][-1]) and same_bits(got["status"], want["status"][-1])
    sol.close()
