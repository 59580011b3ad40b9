"""Static figures of the fp64 per-instance-settings kernels (admm_f64_rows_ps.hip, admm_f64_rowloop_ps.hip, admm_f64_thread_ps.hip: the ",ps"
instantiations of admm_f64_rows_kernel and admm_f64_kernel and the ps forms of two step functions, in translation units of their own) beside their
shared twins, read from the `hipcc -S` listings (build.device_asm).  CPU test: hipcc cross-compiles, no GPU needed.  Kernel names, register and
scratch figures and occupancy only (tests/test_device_code.py has the unit hashes and the routing of the names).  The figures are pinned as built, with no threshold on the growth: the record's lane index and, for
the span of an iteration, its eight words are per-lane values where the twin has scalars ('Per-instance settings: the fp64 library', has
the same table and what it shows)."""
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import figures, kernels_of

# (NX, NU, N or capacity, RT): (VGPRs, AGPRs, bytes of scratch per lane) of the one-solve ps instantiation | of its shared twin in admm_f64_rows.hip
SOLVE_PS = {(12, 4, 10, 0): (256, 0, 176), (12, 4, 30, 0): (256, 232, 0), (12, 4, 20, 0): (256, 208, 0), (4, 1, 10, 0): (255, 0, 0), (8, 4, 9, 0): (256, 0, 100),
            (12, 4, 32, 1): (256, 166, 0), (4, 1, 32, 1): (256, 118, 0), (8, 4, 32, 1): (256, 146, 0), (12, 2, 32, 1): (256, 158, 0), (4, 2, 32, 1): (256, 122, 0),
            (4, 4, 32, 1): (256, 124, 0), (12, 4, 64, 1): (256, 32, 1040), (4, 1, 64, 1): (256, 118, 1040), (8, 4, 64, 1): (256, 138, 1040),
            (12, 2, 64, 1): (256, 26, 1040), (4, 2, 64, 1): (256, 122, 1040), (4, 4, 64, 1): (256, 126, 1040)}
SOLVE = {(12, 4, 10, 0): (256, 0, 160), (12, 4, 30, 0): (256, 224, 0), (12, 4, 20, 0): (256, 206, 0), (4, 1, 10, 0): (249, 0, 0), (8, 4, 9, 0): (256, 0, 96),
         (12, 4, 32, 1): (256, 152, 0), (4, 1, 32, 1): (256, 110, 0), (8, 4, 32, 1): (256, 136, 0), (12, 2, 32, 1): (256, 148, 0), (4, 2, 32, 1): (256, 114, 0),
         (4, 4, 32, 1): (256, 109, 0), (12, 4, 64, 1): (256, 26, 1040), (4, 1, 64, 1): (256, 112, 1040), (8, 4, 64, 1): (256, 134, 1040),
         (12, 2, 64, 1): (256, 18, 1040), (4, 2, 64, 1): (256, 118, 1040), (4, 4, 64, 1): (256, 128, 1040)}
# the on-chip closed loop (Mpc64, Settings64) | its MPC twin in admm_f64_rows.hip
LOOP_PS = {(12, 4, 10, 0): (256, 0, 460), (12, 4, 30, 0): (256, 256, 676), (12, 4, 20, 0): (256, 256, 332), (4, 1, 10, 0): (256, 0, 48), (8, 4, 9, 0): (256, 0, 144),
           (12, 4, 32, 1): (256, 256, 264), (4, 1, 32, 1): (256, 212, 0), (8, 4, 32, 1): (256, 256, 48), (12, 2, 32, 1): (256, 256, 160), (4, 2, 32, 1): (256, 216, 0),
           (4, 4, 32, 1): (256, 228, 0)}
LOOP = {(12, 4, 10, 0): (256, 0, 440), (12, 4, 30, 0): (256, 256, 644), (12, 4, 20, 0): (256, 256, 332), (4, 1, 10, 0): (256, 0, 24), (8, 4, 9, 0): (256, 0, 136),
        (12, 4, 32, 1): (256, 256, 264), (4, 1, 32, 1): (256, 212, 0), (8, 4, 32, 1): (256, 256, 48), (12, 2, 32, 1): (256, 256, 164), (4, 2, 32, 1): (256, 216, 0),
        (4, 4, 32, 1): (256, 228, 0)}
# (NX, NU): the thread-per-instance kernel with per-instance settings | its twin in admm_f64_thread.hip
THREAD_PS = {(12, 4): (256, 256, 1568), (4, 1): (255, 30, 0), (8, 4): (256, 256, 1492), (12, 2): (256, 256, 1228), (4, 2): (256, 78, 0), (4, 4): (256, 120, 0), (16, 4): (256, 256, 2728)}
THREAD = {(12, 4): (256, 256, 1528), (4, 1): (256, 22, 0), (8, 4): (256, 256, 1412), (12, 2): (256, 256, 1184), (4, 2): (256, 72, 0), (4, 4): (256, 112, 0), (16, 4): (256, 256, 2696)}
# (NX, NU, FN): update_slack (FN = 1) and termination_condition (FN = 4) with per-instance settings | admm_f64_step_kernel<NX, NU, FN> in admm_f64_thread.hip
STEP_PS = {(12, 4, 1): (16, 0, 0), (12, 4, 4): (67, 0, 0), (4, 1, 1): (18, 0, 0), (4, 1, 4): (62, 0, 0), (8, 4, 1): (16, 0, 0), (8, 4, 4): (68, 0, 0), (12, 2, 1): (18, 0, 0),
           (12, 2, 4): (67, 0, 0), (4, 2, 1): (16, 0, 0), (4, 2, 4): (62, 0, 0), (4, 4, 1): (14, 0, 0), (4, 4, 4): (64, 0, 0), (16, 4, 1): (16, 0, 0), (16, 4, 4): (67, 0, 0)}
STEP = {(12, 4, 1): (18, 0, 0), (12, 4, 4): (60, 0, 0), (4, 1, 1): (14, 0, 0), (4, 1, 4): (58, 0, 0), (8, 4, 1): (18, 0, 0), (8, 4, 4): (64, 0, 0), (12, 2, 1): (18, 0, 0),
        (12, 2, 4): (36, 0, 0), (4, 2, 1): (14, 0, 0), (4, 2, 4): (58, 0, 0), (4, 4, 1): (14, 0, 0), (4, 4, 4): (60, 0, 0), (16, 4, 1): (18, 0, 0), (16, 4, 4): (60, 0, 0)}
PS_KERNELS = len(SOLVE_PS) + len(LOOP_PS) + len(THREAD_PS) + len(STEP_PS)  # 17 + 11 + 7 + 14 = 49
NEW = ("admm_f64_rows_ps.hip", "admm_f64_rowloop_ps.hip", "admm_f64_thread_ps.hip")
EXISTING = ("admm_f64_rows.hip", "admm_f64_rowsim.hip", "admm_f64_thread.hip", "admm_f64_rows_pm.hip", "admm_f64_rowsim_pm.hip", "admm_f64_thread_pm.hip",
            "admm_f64_plant.hip", "batch64_helpers.hip")


@pytest.fixture(scope="module")
def listings():
    return {u: T.build.device_asm(u).read_text() for u in NEW + EXISTING}


def _rows(listing, loop, ps):
    """keyed (NX, NU, N, RT)"""
    f = figures(listing, "admm_f64_rows_kernel", lambda n: ("Settings64" in n) == ps and ("Mpc64" in n) == loop and "Sim64" not in n and "Models64" not in n)
    return {k[:4]: v for k, v in f.items() if k[4] == int(loop)}


def test_the_new_units_hold_exactly_the_ps_instantiations(listings):
    rows, loop, thread = (list(kernels_of(listings[u])) for u in NEW)
    assert len(rows) == 17 and all("admm_f64_rows_kernel" in n and "Settings64" in n and "Mpc64" not in n and "Sim64" not in n and "Models64" not in n for n in rows), rows
    assert len(loop) == 11 and all("admm_f64_rows_kernel" in n and "Mpc64" in n and "Settings64" in n and "Sim64" not in n and "Models64" not in n for n in loop), loop
    solve = [n for n in thread if "admm_f64_kernel" in n]
    step = [n for n in thread if "admm_f64_step_ps_kernel" in n]
    assert len(solve) == 7 and len(step) == 14 and len(thread) == 21 and all("Settings64" in n and "Models64" not in n for n in thread), thread
    assert len(rows) + len(loop) + len(thread) == PS_KERNELS == 49
    assert set(_rows(listings[NEW[0]], False, True)) == set(SOLVE) and set(_rows(listings[NEW[1]], True, True)) == set(LOOP)
    assert set(figures(listings[NEW[2]], "admm_f64_kernel", lambda n: True)) == set(THREAD)
    assert set(figures(listings[NEW[2]], "admm_f64_step_ps_kernel", lambda n: True)) == {(nx, nu, fn) for nx, nu in THREAD for fn in (1, 4)}


def test_no_settings64_kernel_sits_in_an_existing_unit(listings):
    for u in EXISTING:
        assert not [n for n in kernels_of(listings[u]) if "Settings64" in n or "step_ps" in n], u


def test_every_rows_ps_instantiation_has_its_twin_s_occupancy(listings):
    for ps, twin in ((_rows(listings[NEW[0]], False, True), _rows(listings["admm_f64_rows.hip"], False, False)),
                     (_rows(listings[NEW[1]], True, True), _rows(listings["admm_f64_rows.hip"], True, False))):
        assert set(ps) == set(twin)
        for key in ps:
            assert ps[key][3] == twin[key][3] == (2 if key[2] <= 12 else 1), (key, ps[key], twin[key])
    # the thread-per-instance kernel states no occupancy (launch bounds of one wave per block)
    ps = figures(listings[NEW[2]], "admm_f64_kernel", lambda n: True)
    twin = figures(listings["admm_f64_thread.hip"], "admm_f64_kernel", lambda n: True)
    for key in ps:
        assert ps[key][3] == twin[key][3] >= 1, (key, ps[key], twin[key])


def test_register_and_scratch_figures_are_pinned(listings):
    step_twin = {k: v for k, v in figures(listings["admm_f64_thread.hip"], "admm_f64_step_kernel", lambda n: True).items() if k[2] in (1, 4)}
    got = [(_rows(listings[NEW[0]], False, True), SOLVE_PS, "one solve, ps"), (_rows(listings["admm_f64_rows.hip"], False, False), SOLVE, "one solve"),
           (_rows(listings[NEW[1]], True, True), LOOP_PS, "closed loop, ps"), (_rows(listings["admm_f64_rows.hip"], True, False), LOOP, "closed loop"),
           (figures(listings[NEW[2]], "admm_f64_kernel", lambda n: True), THREAD_PS, "thread, ps"),
           (figures(listings["admm_f64_thread.hip"], "admm_f64_kernel", lambda n: True), THREAD, "thread"),
           (figures(listings[NEW[2]], "admm_f64_step_ps_kernel", lambda n: True), STEP_PS, "step, ps"), (step_twin, STEP, "step")]
    for have, pins, what in got:
        assert set(have) == set(pins), what
        for key, pin in pins.items():
            assert have[key][:3] == pin, f"{what} {key}: (VGPRs, AGPRs, scratch) = {have[key][:3]}, pinned at {pin}"


def test_design_records_the_figures_beside_the_twins():
    text = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    sec = text[text.index("\n## Per-instance settings: the fp64 library"):]
    sec = sec[:(sec + "\n## ").index("\n## ", 4)]   # up to the next section, or the end of the file
    cell = lambda f: f"{f[0]} / {f[1]} / {f[2]}"
    for what, ps, twin in (("solve", SOLVE_PS, SOLVE), ("loop", LOOP_PS, LOOP)):
        for key in ps:
            label = f"{what} ({key[0]},{key[1]},{'n≤' + str(key[2]) if key[3] else key[2]})"
            row = f"| {label} | {cell(ps[key])} | {cell(twin[key])} |"
            assert row in sec, f"DESIGN has no row '{row}'"
    for key in THREAD_PS:
        row = f"| thread ({key[0]},{key[1]}) | {cell(THREAD_PS[key])} | {cell(THREAD[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
    for key in STEP_PS:
        row = f"| {'update_slack' if key[2] == 1 else 'termination_condition'} ({key[0]},{key[1]}) | {cell(STEP_PS[key])} | {cell(STEP[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
