"""CPU companion of tests/test_run_log_gpu.py (the per-step solver log of the closed-loop runs: tiny_batch_mpc_run_log_async, tiny_batch_mpc_run_log,
tiny_batch64_mpc_run_log).  The GPU tests compare every entry of a log with the reference's own closed-loop traces for equality; here the fixtures
are shown to be able to carry that: every scenario they are used on holds both status values, the rows of the two scenarios whose iteration counts
move most are pairwise distinct (a log shifted or repeated by one row cannot pass), and the oracle's loop reproduces the recorded iter and status of
all four scenarios.  Header, library and solver.py agree on the three new names."""
import re
from pathlib import Path

import numpy as np
import pytest

from helpers import GOLDEN, closed_loop_case, load_fixture, oracle_closed_loop

ROOT = Path(__file__).resolve().parents[1]
SCENARIOS = ("hover", "track", "cartpole", "dims837")
SYMBOLS32 = ("tiny_batch_mpc_run_log_async", "tiny_batch_mpc_run_log")
SYMBOL64 = "tiny_batch64_mpc_run_log"


@pytest.fixture(scope="module")
def traces():
    return np.load(GOLDEN / "closed_loop_traces.npz")


def test_header_library_and_solver_agree_on_the_names(tinympc):
    lib = tinympc.load_library()
    for n in SYMBOLS32:
        assert n in tinympc.exported_symbols() and hasattr(lib, n), n
    hdr = (ROOT / "include" / "tinympc_batch.h").read_text()
    assert re.search(r"int tiny_batch_mpc_run_log_async\(TinyBatch \*\w+, int steps, int window_advance, const float \*d_w, float \*d_u0_traj, float \*d_x_traj,\s*"
                     r"int \*d_iter_log, int \*d_status_log\);", hdr)
    assert re.search(r"int tiny_batch_mpc_run_log\(TinyBatch \*\w+, int steps, int window_advance, const float \*w, float \*u0_traj, float \*x_traj,\s*"
                     r"int \*iter_log, int \*status_log\);", hdr)
    hdr64 = (ROOT / "include" / "tinympc_batch64.h").read_text()
    assert re.search(r"int tiny_batch64_mpc_run_log\(TinyBatch64 \*\w+, int steps, int window_advance, const double \*w, double \*u0_traj, double \*x_traj,\s*"
                     r"int \*iter_log[^,]*, int \*status_log[^)]*\);", hdr64)
    assert hasattr(lib, SYMBOL64)
    # the bindings take what the header declares: five (fp64: three) array arguments and two int arrays behind steps and window_advance
    assert len(lib.tiny_batch_mpc_run_log_async.argtypes) == len(lib.tiny_batch_mpc_run_log.argtypes) == len(lib.tiny_batch64_mpc_run_log.argtypes) == 8
    for cls in (tinympc.TinyBatchSolver, tinympc.TinyBatchSolver64):
        assert callable(getattr(cls, "mpc_run_log")), cls
        import inspect
        assert list(inspect.signature(cls.mpc_run_log).parameters) == ["self", "steps", "window_advance", "w", "record_x"]
        assert inspect.signature(cls.mpc_run_log).parameters["record_x"].default is False


def test_the_log_pointers_close_the_kernel_arguments(tinympc):
    """RowParams gains the two pointers at its end: no other kernel argument moves"""
    src = (ROOT / "accelerated-tinympc_amd" / "csrc" / "tinympc_internal.h").read_text()
    body = src[src.index("struct RowParams"):]
    body = body[:body.index("\n};")]
    members = [ln.split("//")[0].strip() for ln in body.splitlines()]
    members = [m for m in members if m.endswith(";")]
    assert members[-1] == "int *iter_log, *status_log;" and members[-2] == "int exact_ties;", members[-3:]


def test_the_traces_can_carry_the_test(traces):
    """both status values in every scenario the GPU tests read a status log on; pairwise distinct rows where they read an iter log over many steps"""
    z = traces
    for name, n11 in (("hover", 548), ("cartpole", 3), ("dims837", 7)):
        st = z[f"{name}_status"]
        assert set(np.unique(st)) == {1, 11}, name
        assert int((st == 11).sum()) == n11, (name, int((st == 11).sum()))
        assert z[f"{name}_iter"].shape == st.shape and st.ndim == 2
    assert z["hover_status"].size == 4480
    for name in ("track", "dims837"):
        it = z[f"{name}_iter"]
        assert len({r.tobytes() for r in it}) == len(it), f"{name}: two steps with the same iteration counts"
    assert z["track_iter"].shape[0] == 110
    # ... also on the instances the GPU tests cut out of the batch
    assert len({r.tobytes() for r in z["track_iter"][:, :37]}) == 110 and len({r.tobytes() for r in z["track_iter"][:, :17]}) >= 100
    for B in (1, 3, 37):
        assert (z["hover_status"][:, :B] == 11).any() and (z["hover_status"][:, :B] == 1).any(), B
    assert (z["cartpole_status"][:, 60:62] == 11).sum() == 3, "cartpole reaches max_iter on instances 60 and 61: the batch of 64 carries them, the batch of 5 does not"
    meta, _, _, z64 = load_fixture("quad_hover_f64_N10")
    assert z64["trace_iter"].shape[0] == 70 and set(np.unique(z64["trace_status"])) <= {1, 11} and z64["trace_iter"][0] == 100


@pytest.mark.parametrize("name", SCENARIOS)
def test_the_oracle_loop_reproduces_iter_and_status_of_every_step(tinympc, oracle_mod, traces, name):
    O, pr = oracle_mod, tinympc.problems
    prob, x0, xref_fn, steps, settings, table, start = closed_loop_case(pr, O, traces, name)
    ref = (table, start) if table is not None else xref_fn(0)
    out = oracle_closed_loop(O, prob, np.float32, settings, x0, ref, pr.bounds_arrays(prob), steps, 1 if table is not None else 0)
    assert np.array_equal(out["iter"], traces[f"{name}_iter"]), name
    assert np.array_equal(out["status"], traces[f"{name}_status"]), name
    assert np.array_equal(out["u0"], traces[f"{name}_u0"]), name
