"""Static figures of the fp64 per-instance-model kernels (admm_f64_rows_pm.hip, admm_f64_rowsim_pm.hip, admm_f64_thread_pm.hip: the ",pm"
instantiations of admm_f64_rows_kernel and admm_f64_kernel in translation units of their own) beside their shared twins, read from the `hipcc -S`
listings (build.device_asm).  CPU test: hipcc cross-compiles, no GPU needed.  The figures are pinned as built, with no threshold on the growth:
rho and the record address are per-lane values where the twin has scalars ('Per-instance models and the batched Riccati', has the same table and what it shows)."""
from pathlib import Path

import pytest

import accelerated_tinympc_amd as T
from isa_tools import figures, kernels_of

# (NX, NU, N or capacity, RT): (VGPRs, AGPRs, bytes of scratch per lane) of the one-solve pm instantiation | of its shared twin in admm_f64_rows.hip
SOLVE_PM = {(12, 4, 10, 0): (256, 0, 164), (12, 4, 30, 0): (256, 226, 0), (12, 4, 20, 0): (256, 208, 0), (4, 1, 10, 0): (251, 0, 0), (8, 4, 9, 0): (256, 0, 104),
            (12, 4, 32, 1): (256, 152, 0), (4, 1, 32, 1): (256, 110, 0), (8, 4, 32, 1): (256, 130, 0), (12, 2, 32, 1): (256, 148, 0), (4, 2, 32, 1): (256, 116, 0),
            (4, 4, 32, 1): (256, 114, 0), (12, 4, 64, 1): (256, 28, 1040), (4, 1, 64, 1): (256, 114, 1040), (8, 4, 64, 1): (256, 134, 1040),
            (12, 2, 64, 1): (256, 20, 1040), (4, 2, 64, 1): (256, 118, 1040), (4, 4, 64, 1): (256, 126, 1040)}
SOLVE = {(12, 4, 10, 0): (256, 0, 160), (12, 4, 30, 0): (256, 224, 0), (12, 4, 20, 0): (256, 206, 0), (4, 1, 10, 0): (249, 0, 0), (8, 4, 9, 0): (256, 0, 96),
         (12, 4, 32, 1): (256, 152, 0), (4, 1, 32, 1): (256, 110, 0), (8, 4, 32, 1): (256, 136, 0), (12, 2, 32, 1): (256, 148, 0), (4, 2, 32, 1): (256, 114, 0),
         (4, 4, 32, 1): (256, 109, 0), (12, 4, 64, 1): (256, 26, 1040), (4, 1, 64, 1): (256, 112, 1040), (8, 4, 64, 1): (256, 134, 1040),
         (12, 2, 64, 1): (256, 18, 1040), (4, 2, 64, 1): (256, 118, 1040), (4, 4, 64, 1): (256, 128, 1040)}
# the closed loop (Mpc64, Sim64, Models64) | its SIM twin in admm_f64_rowsim.hip (tests/test_isa_sim64.py pins the twins themselves)
LOOP_PM = {(12, 4, 10, 0): (256, 0, 432), (12, 4, 30, 0): (256, 256, 628), (12, 4, 20, 0): (256, 256, 308), (4, 1, 10, 0): (256, 0, 36), (8, 4, 9, 0): (256, 0, 164),
           (12, 4, 32, 1): (256, 256, 84), (4, 1, 32, 1): (256, 218, 0), (8, 4, 32, 1): (256, 252, 0), (12, 2, 32, 1): (256, 256, 52), (4, 2, 32, 1): (256, 218, 0),
           (4, 4, 32, 1): (256, 226, 0)}
LOOP = {(12, 4, 10, 0): (256, 0, 508), (12, 4, 30, 0): (256, 256, 708), (12, 4, 20, 0): (256, 256, 388), (4, 1, 10, 0): (256, 0, 0), (8, 4, 9, 0): (256, 0, 144),
        (12, 4, 32, 1): (256, 256, 160), (4, 1, 32, 1): (256, 210, 0), (8, 4, 32, 1): (256, 248, 0), (12, 2, 32, 1): (256, 256, 76), (4, 2, 32, 1): (256, 214, 0),
        (4, 4, 32, 1): (256, 222, 0)}
# (NX, NU): the thread-per-instance kernel with per-instance models | its twin in admm_f64_thread.hip
THREAD_PM = {(12, 4): (256, 256, 1052), (4, 1): (166, 0, 0), (8, 4): (256, 184, 0), (12, 2): (256, 256, 580), (4, 2): (225, 0, 0), (4, 4): (245, 0, 0), (16, 4): (256, 256, 3292)}
THREAD = {(12, 4): (256, 256, 1528), (4, 1): (256, 22, 0), (8, 4): (256, 256, 1412), (12, 2): (256, 256, 1184), (4, 2): (256, 72, 0), (4, 4): (256, 112, 0), (16, 4): (256, 256, 2696)}
PM_KERNELS = len(SOLVE_PM) + len(LOOP_PM) + len(THREAD_PM)  # 17 + 11 + 7 = 35


@pytest.fixture(scope="module")
def listings():
    units = ("admm_f64_rows_pm.hip", "admm_f64_rowsim_pm.hip", "admm_f64_thread_pm.hip", "admm_f64_rows.hip", "admm_f64_rowsim.hip", "admm_f64_thread.hip")
    return {u: T.build.device_asm(u).read_text() for u in units}


def _rows(listing, loop, pm):
    """keyed (NX, NU, N, RT)"""
    f = figures(listing, "admm_f64_rows_kernel", lambda n: ("Models64" in n) == pm and ("Mpc64" in n) == loop and (not loop or "Sim64" in n))
    return {k[:4]: v for k, v in f.items() if k[4] == int(loop)}


def test_the_new_units_hold_exactly_the_pm_instantiations(listings):
    rows, loop, thread = (list(kernels_of(listings[u])) for u in ("admm_f64_rows_pm.hip", "admm_f64_rowsim_pm.hip", "admm_f64_thread_pm.hip"))
    assert len(rows) == 17 and all("admm_f64_rows_kernel" in n and "Models64" in n and "Mpc64" not in n and "Sim64" not in n for n in rows), rows
    assert len(loop) == 11 and all("admm_f64_rows_kernel" in n and "Mpc64" in n and "Sim64" in n and "Models64" in n for n in loop), loop
    gather = [n for n in thread if "models64_gather_kernel" in n]
    assert len(gather) == 1 and len(thread) == 8 and all("admm_f64_kernel" in n and "Models64" in n for n in thread if n not in gather), thread
    assert len(rows) + len(loop) + len(thread) - 1 == PM_KERNELS == 35
    for u in ("admm_f64_rows.hip", "admm_f64_rowsim.hip", "admm_f64_thread.hip"):  # and none has leaked into a pinned unit
        assert not [n for n in kernels_of(listings[u]) if "Models64" in n], u


def test_every_pm_instantiation_has_its_twin_s_occupancy(listings):
    for pm, twin in ((_rows(listings["admm_f64_rows_pm.hip"], False, True), _rows(listings["admm_f64_rows.hip"], False, False)),
                     (_rows(listings["admm_f64_rowsim_pm.hip"], True, True), _rows(listings["admm_f64_rowsim.hip"], True, False))):
        assert set(pm) == set(twin)
        for key in pm:
            assert pm[key][3] == twin[key][3] == (2 if key[2] <= 12 else 1), (key, pm[key], twin[key])
    # the thread-per-instance kernel states no occupancy (launch bounds of one wave per block): the pm form, which keeps no matrix in registers, fits at
    # least as many waves as its twin
    pm = figures(listings["admm_f64_thread_pm.hip"], "admm_f64_kernel", lambda n: "Models64" in n)
    twin = figures(listings["admm_f64_thread.hip"], "admm_f64_kernel", lambda n: True)
    assert set(pm) == set(twin) == set(THREAD)
    for key in pm:
        assert pm[key][3] >= twin[key][3] >= 1, (key, pm[key], twin[key])


def test_register_and_scratch_figures_are_pinned(listings):
    got = [(_rows(listings["admm_f64_rows_pm.hip"], False, True), SOLVE_PM, "one solve, pm"), (_rows(listings["admm_f64_rows.hip"], False, False), SOLVE, "one solve"),
           (_rows(listings["admm_f64_rowsim_pm.hip"], True, True), LOOP_PM, "closed loop, pm"), (_rows(listings["admm_f64_rowsim.hip"], True, False), LOOP, "SIM"),
           (figures(listings["admm_f64_thread_pm.hip"], "admm_f64_kernel", lambda n: "Models64" in n), THREAD_PM, "thread, pm"),
           (figures(listings["admm_f64_thread.hip"], "admm_f64_kernel", lambda n: True), THREAD, "thread")]
    for have, pins, what in got:
        assert set(have) == set(pins), what
        for key, pin in pins.items():
            assert have[key][:3] == pin, f"{what} {key}: (VGPRs, AGPRs, scratch) = {have[key][:3]}, pinned at {pin}"


def test_design_records_the_figures_beside_the_twins():
    text = (Path(__file__).resolve().parents[1] / "DESIGN.md").read_text()
    sec = text[text.index("### The fp64 library (`tiny_batch64_set_models`)"):text.index("## Closed loop against a separate plant")]
    cell = lambda f: f"{f[0]} / {f[1]} / {f[2]}"
    for what, pm, twin in (("solve", SOLVE_PM, SOLVE), ("loop", LOOP_PM, LOOP)):
        for key in pm:
            label = f"{what} ({key[0]},{key[1]},{'n≤' + str(key[2]) if key[3] else key[2]})"
            row = f"| {label} | {cell(pm[key])} | {cell(twin[key])} |"
            assert row in sec, f"DESIGN has no row '{row}'"
    for key in THREAD_PM:
        row = f"| thread ({key[0]},{key[1]}) | {cell(THREAD_PM[key])} | {cell(THREAD[key])} |"
        assert row in sec, f"DESIGN has no row '{row}'"
