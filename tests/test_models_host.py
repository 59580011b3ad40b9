"""Per-instance models and the batched Riccati: argument checks of the new C-ABI calls (no GPU touched) and the model-family generator."""
import ctypes as C

import numpy as np
import pytest

EINVAL = -1


def test_new_entry_points_are_declared(tinympc):
    names = set(tinympc.exported_symbols())
    for n in ("tiny_batch_set_models", "tiny_batch_set_models_device", "tiny_batch_clear_models", "tiny_batch_models_per_instance",
              "tiny_batch_riccati_device", "tiny_batch_set_systems"):
        assert n in names, n


def test_null_handles_and_pointers_are_rejected(tinympc):
    lib = tinympc.load_library()
    f = (C.c_float * 16)()
    d = (C.c_double * 16)()
    F = C.cast(f, C.POINTER(C.c_float))
    D = C.cast(d, C.POINTER(C.c_double))
    assert lib.tiny_batch_set_models(None, *([F] * 8)) == EINVAL
    assert lib.tiny_batch_set_models_device(None, *([None] * 8)) == EINVAL
    assert lib.tiny_batch_clear_models(None) == EINVAL
    assert lib.tiny_batch_models_per_instance(None) == EINVAL
    assert lib.tiny_batch_set_systems(None, D, D, D, D, D, None) == EINVAL
    assert b"NULL" in lib.tiny_batch_last_error()


@pytest.mark.parametrize("nx,nu,count", [(0, 1, 4), (65, 1, 4), (4, 0, 4), (4, 33, 4), (4, 1, 0), (4, 1, -2)])
def test_riccati_device_rejects_bad_sizes_before_touching_hip(tinympc, nx, nu, count):
    lib = tinympc.load_library()
    p = C.c_void_p(16)  # never dereferenced: the sizes are checked first
    assert lib.tiny_batch_riccati_device(nx, nu, count, *([p] * 12), None) == EINVAL
    assert b"tiny_batch_riccati_device" in lib.tiny_batch_last_error()


def test_riccati_device_rejects_null_pointers(tinympc):
    lib = tinympc.load_library()
    p = C.c_void_p(16)
    args = [p] * 12
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10):  # every pointer but coeff_d2p (9), which may be NULL
        a = list(args)
        a[k] = None
        assert lib.tiny_batch_riccati_device(12, 4, 8, *a, None) == EINVAL, k
        assert b"NULL" in lib.tiny_batch_last_error()


@pytest.mark.parametrize("kind,n", [("quadrotor", 32), ("cartpole", 32), ("random83", 32)])
def test_model_family_is_deterministic_and_converges(tinympc, kind, n):
    pr = tinympc.problems
    a = pr.model_family(kind, n, 4 * n, seed=4)
    b = pr.model_family(kind, n, 4 * n, seed=4)
    for k in ("A", "B", "Q", "R", "rho", "model"):
        assert np.array_equal(a[k], b[k]), k
    assert sorted(set(a["model"].tolist())) == list(range(n))
    assert not np.array_equal(a["model"], np.arange(4 * n) % n)  # shuffled: the four instances of a group differ
    ms = a["models"]
    for i in range(n):
        r = tinympc.riccati(ms["A"].shape[1], ms["B"].shape[2], ms["A"][i], ms["B"][i], ms["Q"][i], ms["R"][i], ms["rho"][i])
        assert 1 <= r["iters"] < 1000, (kind, i, r["iters"])
    # the models differ from each other
    assert len({ms["A"][i].tobytes() + ms["B"][i].tobytes() + ms["rho"][i].tobytes() for i in range(n)}) == n


def test_family_caches_follow_with_cache(tinympc):
    pr = tinympc.problems
    fam = pr.model_family("cartpole", 4, 12, seed=1)
    m = pr.family_caches(fam)
    for b in range(12):
        p = m["probs"][fam["model"][b]]
        assert np.array_equal(m["Kinf"][b], p["Kinf"]) and np.array_equal(m["Q"][b], fam["Q"][b] + fam["rho"][b])
        assert m["rho"][b] == fam["rho"][b]


def test_default_families_are_unchanged(tinympc):
    """vary="some" (the default) draws exactly what it drew before vary="all" and the "random" kind existed (tools/models_time.py and the GPU tests
    depend on it): a fingerprint of the quadrotor and cartpole families (no eigenvalue routine in them, so no LAPACK build in the hash)."""
    import hashlib
    pr = tinympc.problems
    for kind, want in (("quadrotor", "825bd11276045965"), ("cartpole", "5d6938f00f23a851")):
        f = pr.model_family(kind, 8, 32, seed=4)
        h = hashlib.sha256()
        for k in ("A", "B", "Q", "R", "rho", "model"):
            h.update(np.ascontiguousarray(f[k]).tobytes())
        assert h.hexdigest()[:16] == want, kind
        g = pr.model_family(kind, 8, 32, seed=4, vary="all")  # the extra draws come from a stream of their own
        assert np.array_equal(g["model"], f["model"]) and np.array_equal(g["rho"], f["rho"])


VARY_ALL = [("quadrotor", None), ("cartpole", None), ("random83", None)] + [("random", d) for d in ((12, 4), (4, 1), (8, 3), (20, 12), (3, 2), (8, 8), (4, 3),
                                                                                                  (36, 4), (28, 16), (1, 1), (2, 5), (3, 8))]


@pytest.mark.parametrize("kind,dims", VARY_ALL, ids=[k if d is None else f"{k}_{d[0]}_{d[1]}" for k, d in VARY_ALL])
def test_model_family_vary_all(tinympc, kind, dims):
    """The families the per-instance-model GPU tests use: deterministic, every pair of models differs in each of A, B, Q, R and rho, and the host
    Riccati converges for every model."""
    pr = tinympc.problems
    n = 12
    a = pr.model_family(kind, n, 3 * n, seed=6, vary="all", dims=dims)
    b = pr.model_family(kind, n, 3 * n, seed=6, vary="all", dims=dims)
    for k in ("A", "B", "Q", "R", "rho", "model"):
        assert np.array_equal(a[k], b[k]), k
    ms = a["models"]
    for k in ("A", "B", "Q", "R", "rho"):
        for i in range(n):
            for j in range(i):
                assert not np.array_equal(ms[k][i], ms[k][j]), (k, i, j)
    if dims is not None:
        assert ms["A"].shape[1:] == (dims[0], dims[0]) and ms["B"].shape[1:] == dims
    for i in range(n):
        r = tinympc.riccati(ms["A"].shape[1], ms["B"].shape[2], ms["A"][i], ms["B"][i], ms["Q"][i], ms["R"][i], ms["rho"][i])
        assert 1 <= r["iters"] < 1000, (kind, dims, i, r["iters"])


def test_every_rowlane_pm_instantiation_has_a_gpu_test():
    """Coverage guard: every class of TINY_FOR_EACH_ROWLANE x {exact, fma} x {one solve, per-instance bounds, on-chip closed loop} (the 48
    admm_rowlane_pm_kernel instantiations) is a case of tests/test_models_paths_gpu.py, so a new class cannot land untested."""
    import re
    from pathlib import Path
    import test_models_paths_gpu as G
    hdr = (Path(__file__).resolve().parents[1] / "accelerated-tinympc_amd" / "csrc" / "tinympc_internal.h").read_text()
    line = re.search(r"#define TINY_FOR_EACH_ROWLANE\(X\)(.*)", hdr).group(1)
    classes = {tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", line)}
    assert len(classes) == 8, classes
    want = {(c, a, w) for c in classes for a in ("exact", "fast") for w in ("solve", "bpi", "mpc")}
    have = {(c, a, "bpi" if bpi else "solve") for c, a, bpi in G.SOLVE_CASES} | {(c, a, "mpc") for c, a in G.MPC_CASES}
    assert have == want, sorted(want ^ have)
