"""Inputs of the per-instance-settings tests (tests/test_settings_gpu.py on the device, tests/test_settings_host.py on the CPU): ONE draw of the settings,
one recipe for the problem data, and the oracle run per distinct settings tuple.  The oracle takes one settings dict per Oracle, so a batch whose
instances differ in their TinySettings is solved group by group and scattered back."""
import numpy as np

from helpers import closed_loop_inputs

# the classes of the heterogeneous batch: three with an unrolled 16-lane instantiation (rowlane<..,ps>), one horizon without (rowstream<..,ps>)
CLASSES = [(12, 4, 10), (4, 1, 10), (8, 3, 7), (12, 4, 13)]
BATCHES = (1, 5, 67)   # ragged last waves; the four rows of a wave get different settings
BUDGETS = (0, 1, 2, 3, 7, 40)
CHECKS = (1, 2, 3, 7)
TOL_DECADES = (-3.0, 0.0)   # tolerances drawn log-uniformly over three decades, 1e-3 .. 1: with budgets this short the loose end is what converges early
SEED = 20260
BASE = dict(abs_pri_tol=1e-3, abs_dua_tol=1e-3, max_iter=40, check_termination=1, en_state_bound=1, en_input_bound=1)
FIELDS = ("abs_pri_tol", "abs_dua_tol", "max_iter", "check_termination", "en_state_bound", "en_input_bound")


def draw(B, seed=SEED, flags=False):
    """the per-instance settings of one solve: a dict of arrays [B].  Every budget and every check_termination value occurs where B allows it (the
    first len(BUDGETS) instances take them in turn, the rest are drawn), so that a small batch is heterogeneous too."""
    rng = np.random.default_rng(seed)
    mi = np.array([BUDGETS[(b + seed) % len(BUDGETS)] if b < len(BUDGETS) else rng.choice(BUDGETS) for b in range(B)], np.int32)
    ct = np.array([CHECKS[(b + seed) % len(CHECKS)] if b < len(CHECKS) else rng.choice(CHECKS) for b in range(B)], np.int32)
    per = dict(abs_pri_tol=(10.0 ** rng.uniform(*TOL_DECADES, size=B)).astype(np.float32),
               abs_dua_tol=(10.0 ** rng.uniform(*TOL_DECADES, size=B)).astype(np.float32),
               max_iter=rng.permutation(mi), check_termination=rng.permutation(ct))
    if flags:
        per["en_state_bound"] = rng.integers(0, 2, size=B).astype(np.int32)
        per["en_input_bound"] = rng.integers(0, 2, size=B).astype(np.int32)
    return per


def problem(pr, O, dims):
    nx, nu, N = dims
    return pr.quadrotor(20, N) if (nx, nu) == (12, 4) else pr.random_system(nx, nu, N, seed=100 * nx + nu, riccati=O.riccati)


def inputs(pr, O, dims, B, bounds):
    """(prob, x0, xref [B][N][nx], bnds): helpers.closed_loop_inputs' spread of x0 amplitudes — small ones converge at once, large ones sit on the
    tightened bounds and use up their budget; bounds "shared": one box for the batch, "inst": every instance's own, scaled 0.5 .. 1.5"""
    prob = problem(pr, O, dims)
    x0, xref, bnds = closed_loop_inputs(prob, B, "inst", SEED + dims[0] + dims[2], amp=(0.002, 0.6))
    if bounds == "inst":
        sc = np.random.default_rng(SEED + 1).uniform(0.5, 1.5, size=B).astype(np.float32)
        bnds = tuple(np.ascontiguousarray(sc[:, None, None] * b[None]) for b in bnds)
    return prob, x0, xref, bnds


def settings_of(per, b, base=BASE):
    """instance b's TinySettings as the oracle's dict (python scalars; the tolerances are the fp32 values the device gets)"""
    s = dict(base)
    for k in FIELDS:
        if k in per:
            s[k] = float(np.float32(per[k][b])) if k.startswith("abs_") else int(per[k][b])
    return s


def per_group(O, prob, dtype, per, st, bnds, xref, fn, base=BASE, arith="exact"):
    """fn(oracle, sub-state, inputs, indices) once per distinct settings tuple, on that group's slice of the state and of the inputs (a [steps][dim]
    input is shared and passed whole); the slices are scattered back into `st`"""
    B = st["x"].shape[0]
    groups = {}
    for b in range(B):
        groups.setdefault(tuple(settings_of(per, b, base).items()), []).append(b)
    for key, idx in groups.items():
        idx = np.array(idx)
        sub = {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}
        ins = [a if a.ndim == 2 else np.ascontiguousarray(a[idx]) for a in (*bnds, xref)]
        fn(O.Oracle(prob, dtype, dict(key), arith=arith), sub, ins, idx)
        for k in st:
            st[k][idx] = sub[k]


def oracle_solve(O, prob, dtype, per, st, bnds, xref, base=BASE, arith="exact"):
    """tiny_solve of every instance under its own settings, in place on `st`.  Returns the number of instances that did not converge."""
    per_group(O, prob, dtype, per, st, bnds, xref, lambda orc, sub, ins, idx: orc.solve(sub, *ins), base, arith)
    return int((st["status"] != 1).sum())


def oracle_step(O, prob, dtype, per, st, bnds, xref, name, base=BASE):
    """one of the six step functions of every instance under its own settings, in place on `st`; returns what it returns per instance"""
    out = np.zeros(st["x"].shape[0], bool)

    def fn(orc, sub, ins, idx):
        out[idx] = orc.step(name, sub, *ins)
    per_group(O, prob, dtype, per, st, bnds, xref, fn, base)
    return out
