"""Per-instance models (tiny_batch_set_models) on the two wave kernels: admm_waveres_pm_kernel and admm_wavestream_pm_kernel, reached with
tiny_batch_set_row_kernel(tb, 7) / (tb, 6), and models_pack_wave_kernel, which packs their gain tables.

Exact arithmetic is pinned bit for bit against the CPU oracle, run once per distinct model over that model's instances.  fma arithmetic (waveres
only) has no bitwise oracle: its reference is the batch-shared waveres<...,fast> kernel, run once per model on that model's instances with the same
inputs.  tests/test_models_wave_host.py checks that WAVEDIMS below lists every class of TINY_FOR_EACH_WAVEDIMS.

The inputs are not those of tests/test_models_paths_gpu.py: with x0 = 0.3 randn and bounds of +-5 these classes converge in their first iteration
and never run a backward sweep.  Here x0[b] = s_b randn with s_b ~ U(0.02, 1), the reference is 0.05 randn, u in +-0.5, x in +-2 and max_iter = 40:
the oracle alone then sees early exits, one-iteration warm solves and instances that exhaust max_iter on every class (test_the_inputs_exercise_...)."""
import numpy as np
import pytest

from test_models_paths_gpu import _SharedFma, _check, _dev_models, _family, _oracle_loop, _oracle_solve, _probs, _same, _set_inputs

pytestmark = pytest.mark.gpu

# TINY_FOR_EACH_WAVEDIMS: both pm kernels are instantiated for each class (waveres: exact and fma; wavestream: the (4, 2) and (1, 3) shapes)
WAVEDIMS = [(32, 16), (16, 8), (16, 4), (20, 8), (24, 4)]
# (nx, nu, N): the (16, 4) horizons are the edges of StepRegs (the 32-register vector, the 16-register vector, the two scalars, in both sweeps);
# (16, 8), (20, 8): the GEMV orders; (24, 4), (32, 16): the other WavePlans
WAVERES = [(16, 4, 3), (16, 4, 10), (16, 4, 33), (16, 4, 34), (16, 4, 49), (16, 4, 50), (16, 8, 10), (20, 8, 10), (24, 4, 10), (32, 16, 50)]
WAVERES_CASES = [(c, B) for c in WAVERES for B in (1, 37)]
# (nx, nu, N, B): N = 51 is a horizon beyond waveres, 2 051 instances reach the (1, 3) shape and a batch beyond one round of the chip
WAVESTREAM_CASES = [(16, 4, 10, 37), (16, 4, 51, 37), (32, 16, 50, 37), (16, 4, 10, 2051)]
REFMODES = ("shared", "per_instance", "window")
SETTINGS = {3: dict(max_iter=1), 8: dict(check_termination=3), 13: dict(en_state_bound=0)}  # by case index; {} elsewhere
N_MODELS, SEED = 5, 500


def _settings(O, extra=None):
    return dict(dict(O.DEFAULT_SETTINGS, max_iter=40), **(extra or {}))


def _winputs(nx, nu, N, B, pib, refmode, seed):
    """x0, reference (shared [N][nx], per instance, or a (table, start) window pair) and bounds (shared or per instance)"""
    rng = np.random.default_rng(seed)
    x0 = (rng.uniform(0.02, 1.0, size=(B, 1)) * rng.standard_normal((B, nx))).astype(np.float32)
    xmn, xmx = np.full((N, nx), -2.0, np.float32), np.full((N, nx), 2.0, np.float32)
    umn, umx = np.full((N - 1, nu), -0.5, np.float32), np.full((N - 1, nu), 0.5, np.float32)
    if pib:
        s = rng.uniform(0.3, 1.0, size=(B, 1, 1)).astype(np.float32)
        xmn, xmx, umn, umx = (np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape) * s, np.float32) for a in (xmn, xmx, umn, umx))
    if refmode == "window":
        ref = ((0.05 * rng.standard_normal((N + 20, nx))).astype(np.float32), rng.integers(0, 20, size=B).astype(np.int32))
    else:
        ref = (0.05 * rng.standard_normal(((N, nx) if refmode == "shared" else (B, N, nx)))).astype(np.float32)
    return x0, ref, (xmn, xmx, umn, umx)


_families = {}


def _models(T, nx, nu, N, B):
    """(fam, mods, probs) of a class and batch: built once, shared by the tests"""
    key = (nx, nu, N, B)
    if key not in _families:
        fam, mods = _family(T, nx, nu, N_MODELS, B, seed=SEED)
        _families[key] = (fam, mods, _probs(mods, N, nx))
    return _families[key]


def _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, family, variant=0):
    s = T.TinyBatchSolver(probs[0], B, settings=settings)
    if mods is not None:
        s.set_models(mods)
    _set_inputs(s, x0, ref, bnd)
    s.set_row_kernel(family)  # first: under models the row variants exist through the forced wave family only
    s.select_kernel(variant)
    return s


def _three_solves(s, step_ref, what):
    """a cold solve, a warm solve from the live-in state, a solve after reset_dual_variables; step_ref(step) returns the state to compare with"""
    for step in ("cold", "warm", "duals reset"):
        if step == "duals reset":
            s.reset_dual_variables()
        s.solve()
        _check(s.get_state(), step_ref(step), f"{what} {step}")


def _oracle_steps(O, probs, model, x0, ref, bnd, settings):
    B, (nx, nu, N) = len(x0), (probs[0]["nx"], probs[0]["nu"], probs[0]["N"])
    st = O.new_state(B, nx, nu, N)
    st["x"][:, 0] = x0
    stats = {}

    def step_ref(step):
        if step == "duals reset":
            st["y"][:] = 0
            st["g"][:] = 0
        _oracle_solve(O, probs, model, st, ref, bnd, settings)
        stats[step] = (st["iter"].copy(), st["status"].copy())
        return st
    return step_ref, stats


# ---- 1: routing --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(16, 4, 10), (32, 16, 50)], ids=["16_4_10", "32_16_50"])
def test_routing(tinympc, oracle_mod, dims):
    T = tinympc
    nx, nu, N = dims
    B = 5
    fam, mods, probs = _models(T, nx, nu, N, B)
    s = T.TinyBatchSolver(probs[0], B, settings=_settings(oracle_mod))
    assert s.kernel_name() == f"waveres<{nx},{nu},exact>"
    s.set_models(mods)
    for family, name in ((7, "waveres"), (6, "wavestream")):
        s.set_row_kernel(family)
        for v in (0, 2):
            s.select_kernel(v)
            assert s.kernel_name() == s.closed_loop_kernel_name() == f"{name}<{nx},{nu},exact,pm>", (family, v, s.kernel_name())
            assert s.arithmetic() == "exact"
        if family == 7:
            s.select_kernel(3)
            assert s.kernel_name() == s.closed_loop_kernel_name() == f"waveres<{nx},{nu},fast,pm>", s.kernel_name()
            assert s.arithmetic() == "fma"
        else:  # fma on the streaming wave kernel keeps its refusal
            with pytest.raises(T.TinyBatchError, match="fma arithmetic for 16 < nx \\+ nu <= 64 needs the state-on-chip wave kernel"):
                s.select_kernel(3)
        s.select_kernel(4)  # the run-time-dimension kernel by name, whatever family is forced
        assert s.kernel_name() == f"generic<{nx},{nu},exact,pm>", s.kernel_name()
    # without a forced family nothing has moved: auto is generic<...,pm>, the row variants are refused with the present text
    s.set_row_kernel(0)
    s.select_kernel(0)
    assert s.kernel_name() == s.closed_loop_kernel_name() == f"generic<{nx},{nu},exact,pm>", s.kernel_name()
    for v in (2, 3):
        with pytest.raises(T.TinyBatchError, match="with per-instance models the row variants run on the unrolled 16-lane kernel only"):
            s.select_kernel(v)
    if (nx, nu) == (32, 16):  # tile48 (8) under models keeps what it does today
        s.set_row_kernel(8)
        assert s.kernel_name() == "generic<32,16,exact,pm>"
        with pytest.raises(T.TinyBatchError, match="with per-instance models the row variants run on the unrolled 16-lane kernel only"):
            s.select_kernel(2)
    # a family switched under a selected fma variant: the name says so and the solve is refused
    s.set_row_kernel(7)
    s.select_kernel(3)
    s.set_row_kernel(6)
    assert s.kernel_name() == "unsupported"
    with pytest.raises(T.TinyBatchError, match="fma arithmetic for 16 < nx \\+ nu <= 64 needs the state-on-chip wave kernel"):
        s.solve()
    s.set_row_kernel(7)
    # the shared names return with clear_models
    s.clear_models()
    s.select_kernel(0)
    for family, name in ((7, f"waveres<{nx},{nu},exact>"), (6, f"wavestream<{nx},{nu},exact>"), (0, f"waveres<{nx},{nu},exact>")):
        s.set_row_kernel(family)
        assert s.kernel_name() == name, (family, s.kernel_name())
    s.close()


def test_waveres_family_is_refused_beyond_its_horizon(tinympc, oracle_mod):
    T = tinympc
    fam, mods, probs = _models(T, 16, 4, 51, 5)
    s = T.TinyBatchSolver(probs[0], 5, settings=_settings(oracle_mod))
    s.set_models(mods)
    with pytest.raises(T.TinyBatchError, match="row kernel 7 has no instantiation"):
        s.set_row_kernel(7)
    s.set_row_kernel(6)
    assert s.kernel_name() == "wavestream<16,4,exact,pm>"
    s.close()


def test_refusals_under_models_stay(tinympc, oracle_mod):
    """fp16 storage and the six step functions keep their refusals with a wave family forced"""
    T = tinympc
    fam, mods, probs = _models(T, 16, 4, 10, 5)
    s = T.TinyBatchSolver(probs[0], 5, settings=_settings(oracle_mod))
    s.set_models(mods)
    s.set_row_kernel(7)
    assert s.lib.tiny_batch_forward_pass(s._h) < 0 and "per-instance models" in s.lib.tiny_batch_last_error().decode()
    s.close()


# ---- 2: waveres pm, exact --------------------------------------------------------------------------------------------------------------------

def test_the_inputs_exercise_every_exit(tinympc, oracle_mod):
    """What the module docstring says about the inputs, on the oracle alone (37 instances, default settings + max_iter = 40): a cold solve has early
    exits and instances that exhaust max_iter, a warm solve has one-iteration exits, everything is finite."""
    T, O = tinympc, oracle_mod
    for nx, nu, N in WAVERES[1:]:
        fam, mods, probs = _models(T, nx, nu, N, 37)
        x0, ref, bnd = _winputs(nx, nu, N, 37, False, "shared", seed=SEED + 1)
        step_ref, stats = _oracle_steps(O, probs, fam["model"], x0, ref, bnd, _settings(O))
        st = step_ref("cold")
        it, status = stats["cold"]
        assert 1 < it.min() < 40 and it.max() == 40 and (status == 1).any() and (status != 1).any(), ((nx, nu, N), it.min(), it.max())
        step_ref("warm")
        assert stats["warm"][0].min() == 1, (nx, nu, N)
        assert all(np.isfinite(v).all() for v in st.values())


@pytest.mark.parametrize("case", WAVERES_CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}-B{B}" for c, B in WAVERES_CASES])
def test_waveres_pm_exact(tinympc, oracle_mod, case):
    """admm_waveres_pm_kernel<NX, NU, true>: all twelve arrays, residuals, status, iter and the signs of zeros, bitwise the oracle per model."""
    T, O = tinympc, oracle_mod
    (nx, nu, N), B = case
    i = WAVERES_CASES.index(case)
    settings = _settings(O, SETTINGS.get(i))
    fam, mods, probs = _models(T, nx, nu, N, B)
    x0, ref, bnd = _winputs(nx, nu, N, B, i % 2 == 1, REFMODES[i % 3], seed=SEED + 10 + i)
    s = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, 7, variant=(0, 2)[i % 2])
    assert s.kernel_name() == f"waveres<{nx},{nu},exact,pm>", s.kernel_name()
    step_ref, _ = _oracle_steps(O, probs, fam["model"], x0, ref, bnd, settings)
    _three_solves(s, step_ref, str(case))
    s.close()


# ---- 3: wavestream pm ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", WAVESTREAM_CASES, ids=[f"{c[0]}_{c[1]}_{c[2]}-B{c[3]}" for c in WAVESTREAM_CASES])
def test_wavestream_pm_exact(tinympc, oracle_mod, case):
    """admm_wavestream_pm_kernel, the (4, 2) shape up to 2 048 instances and the (1, 3) shape beyond: bitwise the oracle per model."""
    T, O = tinympc, oracle_mod
    nx, nu, N, B = case
    i = WAVESTREAM_CASES.index(case)
    settings = _settings(O)
    fam, mods, probs = _models(T, nx, nu, N, B)
    x0, ref, bnd = _winputs(nx, nu, N, B, i % 2 == 0, REFMODES[(i + 1) % 3], seed=SEED + 40 + i)
    s = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, 6, variant=(2, 0)[i % 2])
    assert s.kernel_name() == f"wavestream<{nx},{nu},exact,pm>", s.kernel_name()
    step_ref, _ = _oracle_steps(O, probs, fam["model"], x0, ref, bnd, settings)
    _three_solves(s, step_ref, str(case))
    s.close()


# ---- 4: waveres pm, fma ----------------------------------------------------------------------------------------------------------------------

class _SharedWaveFma(_SharedFma):
    """The fma reference: the batch-shared waveres<...,fast> kernel, one handle per model on that model's instances."""

    def __init__(self, T, probs, model, x0, ref, bnd, settings):
        from test_models_paths_gpu import _sub_ref
        self.B, self.parts = len(model), []
        for m, p in enumerate(probs):
            idx = np.nonzero(model == m)[0]
            if idx.size == 0:
                continue
            s = _wave_solver(T, [p], None, idx.size, x0[idx], _sub_ref(ref, idx), tuple(a[idx] if a.ndim == 3 else a for a in bnd), settings, 7, variant=3)
            assert s.kernel_name() == f"waveres<{p['nx']},{p['nu']},fast>", s.kernel_name()
            self.parts.append((idx, s))


@pytest.mark.parametrize("dims", [(16, 4, 34), (32, 16, 50)], ids=["16_4_34", "32_16_50"])
def test_waveres_pm_fma(tinympc, oracle_mod, dims):
    T, O = tinympc, oracle_mod
    nx, nu, N = dims
    B = 37
    settings = _settings(O)
    fam, mods, probs = _models(T, nx, nu, N, B)
    x0, ref, bnd = _winputs(nx, nu, N, B, nx == 16, "per_instance" if nx == 16 else "window", seed=SEED + 60 + nx)
    s = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, 7, variant=3)
    assert s.kernel_name() == f"waveres<{nx},{nu},fast,pm>", s.kernel_name()
    r = _SharedWaveFma(T, probs, fam["model"], x0, ref, bnd, settings)

    def step_ref(step):
        if step == "duals reset":
            r.call("reset_dual_variables")
        r.call("solve")
        return r.state()
    _three_solves(s, step_ref, f"{dims} fma")
    s.close()
    r.close()


# ---- 5: the same model everywhere is the shared path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(16, 8, 10), (32, 16, 50)], ids=["16_8_10", "32_16_50"])
def test_one_model_replicated_is_the_shared_kernel(tinympc, oracle_mod, dims):
    T, O = tinympc, oracle_mod
    nx, nu, N = dims
    B = 37
    settings = _settings(O)
    fam, mods, probs = _models(T, nx, nu, N, B)
    m0 = int(fam["model"][0])
    rep = {k: np.ascontiguousarray(np.broadcast_to(np.asarray(v)[:1], np.asarray(v).shape)) for k, v in mods.items() if k != "probs"}
    x0, ref, bnd = _winputs(nx, nu, N, B, True, "per_instance", seed=SEED + 70 + nx)
    for family, variant, name in ((7, 2, "waveres<{},{},exact{}>"), (7, 3, "waveres<{},{},fast{}>"), (6, 2, "wavestream<{},{},exact{}>")):
        a = _wave_solver(T, [probs[m0]], rep, B, x0, ref, bnd, settings, family, variant)
        b = _wave_solver(T, [probs[m0]], None, B, x0, ref, bnd, settings, family, variant)
        assert a.kernel_name() == name.format(nx, nu, ",pm") and b.kernel_name() == name.format(nx, nu, ""), (a.kernel_name(), b.kernel_name())

        def step_ref(step):
            if step == "duals reset":
                b.reset_dual_variables()
            b.solve()
            return b.get_state()
        _three_solves(a, step_ref, f"{dims} {name}")
        a.close()
        b.close()


# ---- 6: closed loop --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(16, 4, 10, 7), (24, 4, 10, 6), (24, 4, 10, 7)], ids=["16_4_10-waveres", "24_4_10-wavestream", "24_4_10-waveres"])
def test_closed_loop(tinympc, oracle_mod, case):
    """(solve, plant_step_pm_kernel on the ROW layout at row width 64) x steps: step by step and from the captured graph, against the oracle's loop with
    each instance's own model; a second run continues from the graph."""
    T, O = tinympc, oracle_mod
    nx, nu, N, family = case
    B, steps = 37, 3
    settings = _settings(O)
    fam, mods, probs = _models(T, nx, nu, N, B)
    x0, ref, bnd = _winputs(nx, nu, N, B, False, "window", seed=SEED + 80 + nx + family)
    u0s, x, st = _oracle_loop(O, probs, fam["model"], x0, ref, bnd, steps, 1, settings)
    a = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, family)
    name = ("wavestream" if family == 6 else "waveres") + f"<{nx},{nu},exact,pm>"
    assert a.closed_loop_kernel_name() == name, a.closed_loop_kernel_name()
    for k in range(steps):
        a.mpc_step_async(1)
        assert _same(a.get_u()[:, 0], u0s[k]), f"step by step: u0 of step {k}"
    assert _same(a.get_x0(), x), "step by step: final x0"
    _check(a.get_state(), st, "step by step")
    a.close()
    b = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, family)
    b.mpc_run_async(steps, 1)
    assert _same(b.get_x0(), x), "mpc_run_async: final x0"
    _check(b.get_state(), st, "mpc_run_async")
    assert b.lib.tiny_batch_debug_graph_captures(b._h) == 1
    u0s2, x2, st2 = _oracle_loop(O, probs, fam["model"], x, (ref[0], ref[1] + steps), bnd, 2, 1, settings, st=st)
    b.mpc_run_async(2, 1)
    assert _same(b.get_x0(), x2), "second mpc_run_async: final x0"
    _check(b.get_state(), st2, "second mpc_run_async")
    b.close()
    c = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, family)
    assert _same(c.mpc_run_traj(steps, 1), u0s), "mpc_run_traj: u0 trajectory"
    assert _same(c.get_x0(), x)
    c.close()


def test_closed_loop_against_per_instance_plants(tinympc, oracle_mod):
    """mpc_run_sim with a plant per instance, a disturbance and the state trajectory: the replayed graph's plant step is
    Oracle(dict(prob, Adyn = A_p, Bdyn = B_p)).plant_step plus one fp32 add."""
    T, O = tinympc, oracle_mod
    nx, nu, N, B, steps = 16, 4, 10, 37, 3
    settings = _settings(O)
    fam, mods, probs = _models(T, nx, nu, N, B)
    x0, ref, bnd = _winputs(nx, nu, N, B, False, "window", seed=SEED + 90)
    rng = np.random.default_rng(SEED + 91)
    A = np.stack([np.asarray(probs[m]["Adyn"], np.float64) for m in fam["model"]])
    Bm = np.stack([np.asarray(probs[m]["Bdyn"], np.float64) for m in fam["model"]])
    Ap = (A * (1 + 0.05 * rng.standard_normal(A.shape))).astype(np.float32)
    Bp = (Bm * (1 + 0.05 * rng.standard_normal(Bm.shape))).astype(np.float32)
    w = (0.01 * rng.standard_normal((steps, B, nx))).astype(np.float32)
    plants = [O.Oracle(dict(probs[0], Adyn=a, Bdyn=b), np.float32) for a, b in zip(Ap, Bp)]
    st = O.new_state(B, nx, nu, N)
    x, u0s, xs = x0.copy(), [], []
    for k in range(steps):
        st["x"][:, 0] = x
        st["y"][:] = 0
        st["g"][:] = 0
        _oracle_solve(O, probs, fam["model"], st, (ref[0], ref[1] + k), bnd, settings)
        u0 = st["u"][:, 0].copy()
        x = np.concatenate([o.plant_step(x[b:b + 1], u0[b:b + 1]) for b, o in enumerate(plants)])
        x = (x + w[k]).astype(np.float32)
        u0s.append(u0)
        xs.append(x.copy())
    st["x"][:, 0] = x
    s = _wave_solver(T, probs, mods, B, x0, ref, bnd, settings, 7)
    s.set_plant(Ap, Bp)
    assert s.closed_loop_kernel_name() == "waveres<16,4,exact,pm>"
    u, xt = s.mpc_run_sim(steps, 1, w)
    assert _same(u, np.array(u0s)) and _same(xt, np.array(xs))
    assert _same(s.get_x0(), x)
    _check(s.get_state(), st, "mpc_run_sim")
    s.close()


# ---- 7: lifecycle ----------------------------------------------------------------------------------------------------------------------------

def test_lifecycle(tinympc, oracle_mod):
    import ctypes as C
    T, O = tinympc, oracle_mod
    nx, nu, N, B = 16, 4, 10, 37
    settings = _settings(O)
    fam, mods, probs = _models(T, nx, nu, N, B)
    x0, ref, bnd = _winputs(nx, nu, N, B, True, "per_instance", seed=SEED + 100)
    step_ref, _ = _oracle_steps(O, probs, fam["model"], x0, ref, bnd, settings)
    cold = {k: v.copy() for k, v in step_ref("cold").items()}
    # set_systems (GPU Riccati) and set_models_device install the records set_models does
    a = T.TinyBatchSolver(probs[0], B, settings=settings)
    a.set_systems(fam["A"], fam["B"], fam["Q"], fam["R"], fam["rho"])
    _set_inputs(a, x0, ref, bnd)
    a.set_row_kernel(7)
    assert a.kernel_name() == "waveres<16,4,exact,pm>"
    a.solve()
    _check(a.get_state(), cold, "set_systems")
    a.close()
    s = T.TinyBatchSolver(probs[0], B, settings=settings)
    bufs = _dev_models(mods, B, nx)
    try:
        s._check(s.lib.tiny_batch_set_models_device(s._h, *[C.c_void_p(b.ptr) for b in bufs]))
        s.synchronize()
    finally:
        for b in bufs:
            b.free()
    _set_inputs(s, x0, ref, bnd)
    s.set_row_kernel(7)
    assert s.kernel_name() == "waveres<16,4,exact,pm>"
    s.solve()
    _check(s.get_state(), cold, "set_models_device")
    # 7 -> 6 -> 0 on one handle: the workspace is kept (ROW -> ROW -> TILE under models), a warm solve after each switch continues the oracle's chain
    for family, name in ((6, "wavestream<16,4,exact,pm>"), (0, "generic<16,4,exact,pm>"), (7, "waveres<16,4,exact,pm>")):
        s.set_row_kernel(family)
        assert s.kernel_name() == name, s.kernel_name()
        s.solve()
        _check(s.get_state(), step_ref("warm"), f"warm solve after the switch to {name}")
    # new models at the same record address: both packed tables follow
    fam2, mods2 = _family(T, nx, nu, N_MODELS, B, seed=SEED + 1)
    probs2 = _probs(mods2, N, nx)
    s.set_models(mods2)
    for v, ref_of in ((2, None), (3, _SharedWaveFma)):
        s.select_kernel(v)
        s.reset_workspace()
        s.set_x0(x0)
        s.solve()
        if ref_of is None:
            st2 = O.new_state(B, nx, nu, N)
            st2["x"][:, 0] = x0
            _oracle_solve(O, probs2, fam2["model"], st2, ref, bnd, settings)
        else:
            r = ref_of(T, probs2, fam2["model"], x0, ref, bnd, settings)
            r.call("solve")
            st2 = r.state()
            r.close()
        _check(s.get_state(), st2, f"models replaced, variant {v}")
    # clear_models: the shared model of the handle's construction again
    s.clear_models()
    s.select_kernel(0)
    assert s.kernel_name() == "waveres<16,4,exact>"
    s.reset_workspace()
    s.set_x0(x0)
    s.solve()
    st0 = O.new_state(B, nx, nu, N)
    st0["x"][:, 0] = x0
    _oracle_solve(O, probs[:1], np.zeros(B, np.int64), st0, ref, bnd, settings)
    _check(s.get_state(), st0, "shared solve after clear_models")
    s.close()


# ---- 8: guard zones --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 37])
def test_guard_zones_stay_intact(tinympc, oracle_mod, B):
    """both pm kernels (waveres in both arithmetic forms: both tables) and models_pack_wave_kernel under tiny_batch_debug_guards(1)"""
    T, O = tinympc, oracle_mod
    T.solver.debug_guards(True)
    try:
        for nx, nu, N in ((16, 4, 50), (32, 16, 50)):
            fam, mods, probs = _models(T, nx, nu, N, B)
            x0, ref, bnd = _winputs(nx, nu, N, B, True, "window", seed=SEED + 110)
            for family, variant in ((7, 2), (7, 3), (6, 2)):
                s = _wave_solver(T, probs, mods, B, x0, ref, bnd, _settings(O), family, variant)
                s.solve()
                s.mpc_run_async(2, 1)
                st = s.get_state()
                assert T.solver.debug_check() == 0, (nx, nu, N, family, variant)
                assert all(np.isfinite(v).all() for v in st.values()), (nx, nu, N, family, variant)
                s.close()
    finally:
        T.solver.debug_guards(False)
