"""Problem classes and synthetic batch generators for the batched TinyMPC solver.

Host-side product code (numpy only).  It mirrors the *inputs* of the reference's example
programs so that the batched solver can be driven on the same problems:

* quadrotor(rate, N)     — Crazyflie model + precomputed cache, numbers of
                           /root/reference/examples/problem_data/quadrotor_{20,50,100}hz_params.hpp
                           (re-encoded by tools/import_problem_data.py into data/*.json).
* cartpole(N)            — model of examples/codegen_cartpole.cpp:22-28 (A, B column-major there),
                           cache from the Riccati recursion of src/tinympc/codegen.cpp:254-292.
* random_system(...)     — seeded marginally-stable synthetic system.
* y_axis_line()          — the 301-point reference trajectory of
                           examples/trajectory_data/quadrotor_20hz_y_axis_line.hpp (it is analytic).
* hover_batch / tracking_batch — the synthetic batches of BASELINE.json configs 2 and 3.

Matrices are numpy arrays in logical (row, col) indexing, float64; the solver casts to fp32.
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

DATA = Path(__file__).resolve().parent / "data"

NTOTAL = 301  # src/tinympc/glob_opts.hpp:9


def _mat(entry):
    vals = np.array([float(v) for v in entry["values"]], dtype=np.float64)
    return vals.reshape(entry["shape"])  # row-major literals (quadrotor_20hz_params.hpp, Eigen::RowMajor maps)


def quadrotor(rate: int = 20, N: int = 30) -> dict:
    """Quadrotor problem of examples/quadrotor_hovering.cpp:33-47 (nx=12, nu=4)."""
    d = json.loads((DATA / f"quadrotor_{rate}hz.json").read_text())
    prob = dict(name=f"quadrotor_{rate}hz", nx=d["nx"], nu=d["nu"], N=N, rho=float(d["rho"]))
    for k in ("Adyn", "Bdyn", "Kinf", "Pinf", "Quu_inv", "AmBKt", "Q", "R"):
        prob[k] = _mat(d[k])
    # constant box bounds of quadrotor_hovering.cpp:44-47
    prob["u_min"], prob["u_max"], prob["x_min"], prob["x_max"] = -0.5, 0.5, -5.0, 5.0
    return prob


def cartpole(N: int = 10, riccati=None) -> dict:
    """Cartpole of examples/codegen_cartpole.cpp:17-28,51-60 (nx=4, nu=1, rho=0.1, bounds +-5).

    `riccati(nx, nu, A, B, Q, R, rho) -> dict` supplies the cache; default is the product's own
    host routine (accelerated-tinympc_amd/csrc/riccati.cpp through the C-ABI).
    """
    nx, nu = 4, 1
    a_cm = [1.0, 0.0, 0.0, 0.0, 0.01, 1.0, 0.0, 0.0, 2.2330083403300767e-5, 0.004466210576510177,
            1.0002605176397052, 0.05210579005928538, 7.443037974683548e-8, 2.2330083403300767e-5,
            0.01000086835443038, 1.0002605176397052]
    b_cm = [7.468368562730335e-5, 0.014936765390161838, 3.79763323185387e-5, 0.007595596218554721]
    A = np.array(a_cm).reshape(nx, nx).T  # literals are column-major
    B = np.array(b_cm).reshape(nu, nx).T
    prob = dict(name="cartpole", nx=nx, nu=nu, N=N, rho=0.1, Adyn=A, Bdyn=B,
                Q=np.array([10.0, 1.0, 10.0, 1.0]), R=np.array([1.0]),
                u_min=-5.0, u_max=5.0, x_min=-5.0, x_max=5.0)
    return with_cache(prob, riccati)


def random_system(nx: int = 32, nu: int = 16, N: int = 50, seed: int = 1234, riccati=None) -> dict:
    """Seeded marginally-stable random LTI system.

    A = I + 0.05*G/sqrt(nx) rescaled to spectral radius 1 (avoids denormal-dominated decay),
    B = 0.1*G', Q_i = 10, R_i = 1, rho = 1, bounds u in [-0.5,0.5], x in [-5,5].
    """
    rng = np.random.default_rng(seed)
    A = np.eye(nx) + 0.05 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
    A = A / np.max(np.abs(np.linalg.eigvals(A)))
    B = 0.1 * rng.standard_normal((nx, nu))
    prob = dict(name=f"random_{nx}_{nu}", nx=nx, nu=nu, N=N, rho=1.0, Adyn=A, Bdyn=B,
                Q=np.full(nx, 10.0), R=np.full(nu, 1.0), u_min=-0.5, u_max=0.5, x_min=-5.0, x_max=5.0)
    return with_cache(prob, riccati)


def with_cache(prob: dict, riccati=None) -> dict:
    """Attach Kinf/Pinf/Quu_inv/AmBKt computed by the Riccati recursion (codegen.cpp:254-292).

    NOTE the reference's codegen stores Q+rho in work.Q (codegen.cpp:255,:433) whereas the
    shipped quadrotor headers store the raw Q; `tiny_solve` just uses whatever is in work.Q
    (admm.cpp:81).  We follow the codegen convention here: prob["Q"] becomes Q+rho.
    """
    if riccati is None:
        from . import riccati as _r
        riccati = _r
    cache = riccati(prob["nx"], prob["nu"], prob["Adyn"], prob["Bdyn"], prob["Q"], prob["R"], prob["rho"])
    if isinstance(cache, tuple):
        cache = cache[0]
    out = dict(prob)
    out.update({k: np.asarray(cache[k], np.float64) for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt")})
    out["Q_raw"] = np.asarray(prob["Q"], np.float64)
    out["Q"] = out["Q_raw"] + prob["rho"]
    return out


def model_family(kind: str, n_models: int, batch: int, seed: int = 7, vary: str = "some", dims: tuple | None = None) -> dict:
    """Seeded family of `n_models` distinct models of one class, assigned to `batch` instances by a shuffled index.

    kind = "quadrotor": the 20 Hz quadrotor with per-model scaled Bdyn columns (mass / inertia, 0.8 ... 1.25) and rho (4 ... 6.5, around the shipped 5);
    "cartpole": the cartpole with A perturbed by 1 % relative noise on its non-zero entries and rho (1 ... 4); "random83": seeded random (8, 3) systems;
    "random": seeded random systems of any dims = (nx, nu) (each <= 4 or a multiple of 4 for the run-time-dimension kernel), spectral radius 0.9 ... 0.97,
    every matrix their own.
    vary = "all" gives every model its own A, B, Q and R as well: the quadrotor's non-zero Adyn entries get 1 ... 2 % relative noise, the cartpole's
    Bdyn a per-model scale (0.8 ... 1.25), and every kind per-entry Q and R scales (0.5 ... 2).  Those extra draws come from a second stream seeded by `seed`, so
    vary = "some" (the default) gives the same models for the same seed with or without it.
    Returns per-instance A [B][nx][nx], B [B][nx][nu], Q [B][nx], R [B][nu] (without rho), rho [B] (float64), the per-instance model index
    `model` [B] and the distinct models' own arrays under "models" (the same keys, leading axis n_models)."""
    if vary not in ("some", "all"):
        raise ValueError(vary)
    rng = np.random.default_rng(seed)
    if kind == "quadrotor":
        base = quadrotor(20, 30)
        A0, B0, Q0, R0 = base["Adyn"], base["Bdyn"], np.asarray(base["Q"], np.float64), np.asarray(base["R"], np.float64).ravel()
        As, Bs, rhos = [], [], []
        for _ in range(n_models):
            As.append(A0.copy())
            Bs.append(B0 * rng.uniform(0.8, 1.25, size=B0.shape[1])[None, :])
            rhos.append(rng.uniform(4.0, 6.5))
        Qs, Rs = [Q0.copy() for _ in range(n_models)], [R0.copy() for _ in range(n_models)]
    elif kind == "cartpole":
        base = cartpole()
        A0, B0 = base["Adyn"], base["Bdyn"]
        As = [A0 * (1.0 + 0.01 * rng.standard_normal(A0.shape) * (A0 != 0)) for _ in range(n_models)]
        Bs = [B0.copy() for _ in range(n_models)]
        Qs, Rs = [np.array([10.0, 1.0, 10.0, 1.0]) for _ in range(n_models)], [np.array([1.0]) for _ in range(n_models)]
        rhos = [float(rng.uniform(5.0, 20.0)) for _ in range(n_models)]
    elif kind == "random83":
        As, Bs, Qs, Rs, rhos = [], [], [], [], []
        for _ in range(n_models):
            A = np.eye(8) + 0.05 * rng.standard_normal((8, 8)) / np.sqrt(8)
            As.append(A / np.max(np.abs(np.linalg.eigvals(A))))
            Bs.append(0.1 * rng.standard_normal((8, 3)))
            Qs.append(np.full(8, 10.0)); Rs.append(np.full(3, 1.0)); rhos.append(float(rng.uniform(0.5, 2.0)))
    elif kind == "random":
        nx, nu = dims
        As, Bs, Qs, Rs, rhos = [], [], [], [], []
        for _ in range(n_models):
            A = np.eye(nx) + 0.05 * rng.standard_normal((nx, nx)) / np.sqrt(nx)
            As.append(rng.uniform(0.9, 0.97) * A / np.max(np.abs(np.linalg.eigvals(A))))  # strictly stable: the Riccati recursion converges in ~100 iterations
            Bs.append(0.1 * rng.standard_normal((nx, nu)))
            Qs.append(10.0 * rng.uniform(0.5, 2.0, size=nx)); Rs.append(rng.uniform(0.5, 2.0, size=nu)); rhos.append(float(rng.uniform(0.5, 2.0)))
    else:
        raise ValueError(kind)
    if vary == "all" and kind != "random":
        r2 = np.random.default_rng([seed, 1])
        for i in range(n_models):
            if kind == "quadrotor":
                nz = As[i] != 0
                As[i] = As[i] * (1.0 + r2.uniform(0.01, 0.02, size=nz.shape) * r2.choice([-1.0, 1.0], size=nz.shape) * nz)
            elif kind == "cartpole":
                Bs[i] = Bs[i] * r2.uniform(0.8, 1.25, size=Bs[i].shape[1])[None, :]
            Qs[i] = Qs[i] * r2.uniform(0.5, 2.0, size=Qs[i].shape)
            Rs[i] = Rs[i] * r2.uniform(0.5, 2.0, size=Rs[i].shape)
    model = rng.permutation(np.arange(batch) % n_models)
    models = dict(A=np.array(As), B=np.array(Bs), Q=np.array(Qs), R=np.array(Rs), rho=np.array(rhos, np.float64))
    out = {k: v[model] for k, v in models.items()}
    out["model"] = model
    out["models"] = models
    return out


def family_caches(fam: dict, riccati=None) -> dict:
    """The per-instance models of a model_family() batch with host Riccati caches (one tiny_riccati per distinct model), in the keys and
    conventions of with_cache / TinyBatchSolver.set_models (Q = Q + rho).  Also returns the distinct models' prob-style dicts under "probs"."""
    if riccati is None:
        from . import riccati as _r
        riccati = _r
    ms = fam["models"]
    nx, nu = ms["A"].shape[1], ms["B"].shape[2]
    probs = []
    for i in range(len(ms["rho"])):
        p = dict(nx=nx, nu=nu, rho=float(ms["rho"][i]), Adyn=ms["A"][i], Bdyn=ms["B"][i], Q=ms["Q"][i], R=ms["R"][i])
        probs.append(with_cache(p, riccati))
    idx = fam["model"]
    out = {k: np.array([probs[m][k] for m in range(len(probs))])[idx] for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt", "Adyn", "Bdyn", "Q")}
    out["rho"] = ms["rho"][idx]
    out["probs"] = probs
    return out


def y_axis_line() -> np.ndarray:
    """(301, 12) reference trajectory: z = 1 m, y from 0 to 4 m, dy = 0.2666667 m/s (0 in the last row).

    The reference stores it as 7-decimal literals (quadrotor_20hz_y_axis_line.hpp:6-306); we
    regenerate the same decimals analytically (tests/test_problems.py checks equality against the
    header when the reference tree is present).
    """
    X = np.zeros((NTOTAL, 12))
    for k in range(NTOTAL):
        X[k, 1] = float(f"{k * 4.0 / 300.0:.7f}")
        X[k, 2] = 1.0
        X[k, 7] = 0.2666667 if k < NTOTAL - 1 else 0.0
    return X


HOVER_X0 = np.array([0, 1, 0, 0.2, 0, 0, 0.1, 0, 0, 0, 0, 0], dtype=np.float64)   # quadrotor_hovering.cpp:88
HOVER_XREF = np.array([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.float64)    # quadrotor_hovering.cpp:83-85


def hover_batch(B: int, N: int = 30, seed: int = 20241024, spread: float = 0.2):
    """BASELINE.json config 2: x0_b = x0_nom + U(-spread, spread)^12; Xref = hover set-point, shared.

    Returns (x0 (B,12) float32, Xref (N,12) float32).
    """
    rng = np.random.default_rng(seed)
    x0 = HOVER_X0[None, :] + rng.uniform(-spread, spread, size=(B, 12))
    xref = np.tile(HOVER_XREF, (N, 1))
    return x0.astype(np.float32), xref.astype(np.float32)


def tracking_batch(B: int, N: int = 30, seed: int = 20241024, spread: float = 0.05):
    """BASELINE.json config 3: instance b tracks the window of y_axis_line starting at
    k_b = b mod (301 - N) (quadrotor_tracking.cpp:84-85,101), x0_b = Xref_b[0] + U(-spread, spread)^12.

    Returns (x0 (B,12) float32, table (301,12) float32, start (B,) int32).  The per-instance
    reference is Xref_b = table[start[b] : start[b]+N].
    """
    rng = np.random.default_rng(seed)
    table = y_axis_line()
    start = (np.arange(B) % (NTOTAL - N)).astype(np.int32)
    x0 = table[start] + rng.uniform(-spread, spread, size=(B, 12))
    return x0.astype(np.float32), table.astype(np.float32), start


def random_batch(B: int, nx: int = 32, N: int = 50, seed: int = 20241024):
    """BASELINE.json config 4: x0_b ~ U(-1, 1)^nx, reference = the origin, shared by the batch.

    Returns (x0 (B,nx) float32, Xref (N,nx) float32).  Row b is the same whatever B is (the generator fills row-major).
    """
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1.0, 1.0, size=(B, nx))
    return x0.astype(np.float32), np.zeros((N, nx), np.float32)


def expand_windows(table: np.ndarray, start: np.ndarray, N: int) -> np.ndarray:
    """Materialise per-instance references (B, N, nx) from a trajectory table and window starts."""
    idx = start[:, None].astype(np.int64) + np.arange(N)[None, :]
    return np.ascontiguousarray(table[idx])


def bounds_arrays(prob: dict, dtype=np.float32):
    """Constant box bounds as shared (N, nx) / (N-1, nu) arrays (quadrotor_hovering.cpp:44-47)."""
    N, nx, nu = prob["N"], prob["nx"], prob["nu"]
    return (np.full((N, nx), prob["x_min"], dtype), np.full((N, nx), prob["x_max"], dtype),
            np.full((N - 1, nu), prob["u_min"], dtype), np.full((N - 1, nu), prob["u_max"], dtype))
