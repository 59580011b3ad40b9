"""Inputs of the fp64 per-instance-settings tests (tests/test_settings64_gpu.py on the device, tests/test_settings64_host.py on the CPU): settings_cases'
budgets, check_termination values, problem recipe and input spread, with everything in float64 and the tolerances drawn as doubles that no float32
holds, so that a device which narrowed a tolerance would flip a compare.  The oracle takes one settings dict per Oracle: a heterogeneous batch is
solved group by group and scattered back (per_group: settings_cases.per_group with the tolerances kept as doubles)."""
import numpy as np

import settings_cases as SC
from settings_cases import BASE, BATCHES, BUDGETS, CHECKS, FIELDS, SEED, TOL_DECADES  # noqa: F401  (the tests read them from here)

# (nx, nu, N): the kernel path of the sixteen-lane kernel it exercises
CLASSES = [(12, 4, 10),   # unrolled, slack in registers
           (4, 1, 10),    # unrolled, the NU == 1 summation path
           (8, 4, 9),     # unrolled
           (12, 4, 30),   # unrolled, slack in LDS
           (12, 2, 11),   # capacity 32
           (4, 2, 40),    # capacity 64: [p ; d] written through
           (16, 4, 10)]   # no sixteen-lane form: thread64
DT = np.float64


def kernel_name(dims, ps=True, mpc=False, thread=False):
    """what tiny_batch64_kernel_name / _closed_loop_kernel_name report for a class"""
    nx, nu, N = dims
    tail = (",mpc" if mpc else "") + (",ps" if ps else "")
    if thread or nx + nu > 16:
        return f"thread64<{nx},{nu}{tail}>"
    body = str(N) if dims in ((12, 4, 10), (12, 4, 30), (12, 4, 20), (4, 1, 10), (8, 4, 9)) else "n<=32" if N <= 32 else "n<=64"
    return f"rows64<{nx},{nu},{body}{tail}>"


def draw(B, seed=SEED, flags=False):
    """settings_cases.draw from the same random stream, the tolerances left as the doubles they were drawn as (log-uniform over 1e-3 .. 1)"""
    rng = np.random.default_rng(seed)
    mi = np.array([BUDGETS[(b + seed) % len(BUDGETS)] if b < len(BUDGETS) else rng.choice(BUDGETS) for b in range(B)], np.int32)
    ct = np.array([CHECKS[(b + seed) % len(CHECKS)] if b < len(CHECKS) else rng.choice(CHECKS) for b in range(B)], np.int32)
    per = dict(abs_pri_tol=10.0 ** rng.uniform(*TOL_DECADES, size=B), abs_dua_tol=10.0 ** rng.uniform(*TOL_DECADES, size=B),
               max_iter=rng.permutation(mi), check_termination=rng.permutation(ct))
    if flags:
        per["en_state_bound"] = rng.integers(0, 2, size=B).astype(np.int32)
        per["en_input_bound"] = rng.integers(0, 2, size=B).astype(np.int32)
    assert per["abs_pri_tol"].dtype == np.float64 and per["abs_dua_tol"].dtype == np.float64
    return per


def problem(pr, O, dims):
    return SC.problem(pr, O, dims)


def inputs(pr, O, dims, B, bounds):
    """settings_cases.inputs (the same x0 spread, reference and boxes) as float64 arrays"""
    prob, x0, xref, bnds = SC.inputs(pr, O, dims, B, bounds)
    return prob, x0.astype(DT), xref.astype(DT), tuple(b.astype(DT) for b in bnds)


def settings_of(per, b, base=BASE):
    """instance b's TinySettings as the oracle's dict: python scalars, the tolerances the very doubles the device gets"""
    s = dict(base)
    for k in FIELDS:
        if k in per:
            s[k] = float(per[k][b]) if k.startswith("abs_") else int(per[k][b])
    return s


def groups_of(per, B, base=BASE):
    """{settings tuple: indices}"""
    groups = {}
    for b in range(B):
        groups.setdefault(tuple(settings_of(per, b, base).items()), []).append(b)
    return {k: np.array(v) for k, v in groups.items()}


def per_group(O, prob, per, st, bnds, xref, fn, base=BASE):
    """fn(oracle, sub-state, inputs, indices) once per distinct settings tuple, on that group's slice of the state and of the inputs (a [steps][dim]
    input is shared and passed whole); the slices are scattered back into `st`"""
    for key, idx in groups_of(per, st["x"].shape[0], base).items():
        sub = {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}
        ins = [a if a.ndim == 2 else np.ascontiguousarray(a[idx]) for a in (*bnds, xref)]
        fn(O.Oracle(prob, DT, dict(key)), sub, ins, idx)
        for k in st:
            st[k][idx] = sub[k]


def oracle_solve(O, prob, per, st, bnds, xref, base=BASE):
    """tiny_solve of every instance under its own settings, in place on `st`.  Returns the number of instances that did not converge."""
    per_group(O, prob, per, st, bnds, xref, lambda orc, sub, ins, idx: orc.solve(sub, *ins), base)
    return int((st["status"] != 1).sum())


def oracle_step(O, prob, per, st, bnds, xref, name, base=BASE):
    """one of the six step functions of every instance under its own settings, in place on `st`; returns what it returns per instance"""
    out = np.zeros(st["x"].shape[0], bool)

    def fn(orc, sub, ins, idx):
        out[idx] = orc.step(name, sub, *ins)
    per_group(O, prob, per, st, bnds, xref, fn, base)
    return out


def oracle_loop(O, prob, per, x0, ref, bnds, steps, adv, plant=None, w=None, base=BASE):
    """The reference's closed loop with every instance under its own settings: per step y = g = 0, tiny_solve per settings group, the plant step
    (`plant`: x, u0 -> x, default the model's) and x = x + w[k] where a disturbance is given.  ref: a [B][N][nx] or [N][nx] array or a (table, start)
    window.  Returns u.col(0), iter, status and x after the plant step of every step, and the final workspace."""
    from helpers import ref_at
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    B = len(x0)
    step = plant or O.Oracle(prob, DT).plant_step
    st = O.new_state(B, nx, nu, N, DT)
    x = np.array(x0, DT)
    out = dict(u0=[], iter=[], status=[], xs=[])
    for k in range(steps):
        st["x"][:, 0] = x; st["y"][:] = 0; st["g"][:] = 0
        oracle_solve(O, prob, per, st, bnds, ref_at(ref, k, adv, N, B), base)
        u0 = st["u"][:, 0].copy()
        x = step(x, u0)
        if w is not None:
            x = x + w[k]
        out["u0"].append(u0); out["iter"].append(st["iter"].copy()); out["status"].append(st["status"].copy()); out["xs"].append(x.copy())
    st["x"][:, 0] = x  # the plant step after the last solve writes x.col(0)
    return dict({k: np.array(v) for k, v in out.items()}, x=x, st=st)
