"""The fp64 library's choice of kernel and loop, row by row, against the record of the library before the choice was gathered into resolve_plan64.

tests/golden/kernel_choice64.json was written by tools/kernel_choice64_table.py (its header says what a row is and how the result rows were thinned)
on an MI355X with the library of the commit the table names; it is never regenerated from the library under test.  Every row of every handle is
replayed in the recorded order and every stored field — select_kernel's outcome, the two kernel names, every call's return code and the sha256 over
the workspace, status, iter, residuals, window starts and trajectories it left — must be equal."""
import importlib.util
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_choice64_table", ROOT / "tools" / "kernel_choice64_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


K = _tool()
TABLE = K.load_table(ROOT / "tests" / "golden" / "kernel_choice64.json")


def _body(src, head):
    """the text of the function whose definition starts with `head`, up to the closing brace in the first column"""
    assert src.count("\n" + head) == 1, head
    a = src.index("\n" + head)
    return src[a:src.index("\n}\n", a)]


def test_selection64_is_stated_once():
    """csrc/tinympc_batch64.hip resolves what a call launches in resolve_plan64 and nowhere else: every solve launcher and every plant launcher is
    called from one place, the class lists are asked in resolve_plan64 and tiny_batch64_select_kernel alone, the environment is read once, and the
    scattered forms are gone"""
    src = (ROOT / "accelerated-tinympc_amd" / "csrc" / "tinympc_batch64.hip").read_text()
    for name in ("launch_f64_rows", "launch_f64_rows_pm", "launch_rows64_sim", "launch_rows64_loop_pm", "launch_f64_thread", "launch_f64_thread_pm",
                 "launch_plant64", "launch_plant64_run", "launch_plant64_sim"):
        assert len(re.findall(rf"\b{name}\(", src)) == 1, f"{name} is called from {len(re.findall(rf'{name}[(]', src))} places"
    allowed = _body(src, "int resolve_plan64(") + _body(src, "int tiny_batch64_select_kernel(")
    for fn in ("rows_supported(", "rows_unrolled("):
        assert src.count(fn) == allowed.count(fn) >= 1, f"{fn} outside resolve_plan64 and tiny_batch64_select_kernel"
    assert src.count('getenv("TINYMPC_F64_LOOP")') == 1 and src.count("getenv(") == 1
    for gone in ("rows_chosen", "onchip64", "strlen("):
        assert gone not in src, gone


def test_table_keeps_its_coverage():
    """what the tool asserts when it writes: the full product of name rows, and result rows for every plan the product reaches, every arm of the run
    driver, every plant kernel of a step, a window and a plain reference; and the table names the commit it records"""
    K.check_coverage(TABLE)
    assert re.fullmatch(r"[0-9a-f]{40}", TABLE["commit"])
    assert sum(len(h["names"]) for h in TABLE["handles"]) == 10 * 108


@pytest.mark.gpu
@pytest.mark.parametrize("hi", range(len(TABLE["handles"])), ids=lambda i: "{cls[0]}_{cls[1]}_{cls[2]}-B{batch}".format(**TABLE["handles"][i]))
def test_kernel_choice64_matches_the_record(tinympc, hi):
    h = TABLE["handles"][hi]
    got = K.replay(tinympc, h)
    for part in ("names", "results"):
        assert len(got[part]) == len(h[part])
        for n, (w, g) in enumerate(zip(h[part], got[part])):
            assert g == w, f"{part} row {n} {K.cfg_of(w[0])}: recorded {w[1:]}, now {g[1:]}"
