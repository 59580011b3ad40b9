"""The closed-loop runs, row by row, against the record of the library before the loop decision moved into resolve_plan (KernelPlan::loop).

tests/golden/closed_loop_plan.json was written by tools/closed_loop_plan_table.py (its header says what a row is and how the product was thinned) on an
MI355X with the library of the commit before that refactor; it is never regenerated from the library under test.  Every row of every handle is
replayed in the recorded order and every stored field — the closed-loop kernel's name before and after the call, refusal texts, the count of
graph captures after the call and after an identical second one (0 / 0 on chip, 1 / 0 replayed), dispatch_applied(), the checksums of u0_traj, x_traj,
the two logs, the final x0 and iter[] — must be equal.  No size rule enters at these batches (5 and 17 instances), so the CU count is not asked.

Measured on an MI355X: 0.6 s for the seven handles together (419 rows, two runs each), the slowest handle 0.13 s."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("closed_loop_plan_table", ROOT / "tools" / "closed_loop_plan_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TABLE = _tool().load_table(ROOT / "tests" / "golden" / "closed_loop_plan.json")


def test_table_separates_every_term_of_the_decision():
    """the thinning kept what the tool asserts when it writes: for each of the six terms of the on-chip decision two rows that differ in that term alone
    and end on different sides, and a refused call with its text; the handles and their rows are those the tool plans today"""
    K = _tool()
    K.check_coverage(TABLE)
    assert TABLE["keys"] == K.KEYS and TABLE["max_iter"] == K.MAX_ITER
    assert [{k: h[k] for k in ("cls", "batch", "storage")} for h in TABLE["handles"]] == K.HANDLES
    for h in TABLE["handles"]:
        assert [r[0] for r in h["rows"]] == K.plan(h, h["row_kernels"]), h["cls"]
    assert sum(len(h["rows"]) for h in TABLE["handles"]) > 300


@pytest.fixture(scope="module")
def session():
    return _tool().Session()


@pytest.mark.gpu
@pytest.mark.parametrize("hi", range(len(TABLE["handles"])), ids=lambda i: "{cls[0]}_{cls[1]}_{cls[2]}-B{batch}-s{storage}".format(**TABLE["handles"][i]))
def test_closed_loop_runs_match_the_record(session, hi):
    K, h = _tool(), TABLE["handles"][hi]
    got = session.run({k: h[k] for k in ("cls", "batch", "storage")}, [r[0] for r in h["rows"]])
    assert got["row_kernels"] == h["row_kernels"]
    assert len(got["rows"]) == len(h["rows"])
    for n, (w, g) in enumerate(zip(h["rows"], got["rows"])):
        assert list(g) == w, f"row {n} {K.cfg_of(w[0])}: recorded {w[1:]}, now {g[1:]}"
