"""The kernel choice, row by row, against the record of the library before the selection code was gathered into resolve_plan.

tests/golden/kernel_choice.json (with its rows in kernel_choice_rows.json.gz) was written by tools/kernel_choice_table.py (its header says what a row is and how the product was thinned) on
an MI355X with the library of the commit before that refactor; it is never regenerated from the library under test.  Every row of every handle
is replayed in the recorded order and every stored field — kernel names, arithmetic, refusal texts, dispatch_applied(), the checksum of
iter[], the count of captured graphs — must be equal."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def _tool():
    spec = importlib.util.spec_from_file_location("kernel_choice_table", ROOT / "tools" / "kernel_choice_table.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TABLE = _tool().load_table(ROOT / "tests" / "golden" / "kernel_choice.json")  # and kernel_choice_rows.json.gz beside it


def test_table_holds_every_kernel_family(tinympc):
    """every kernel-name prefix of build.KERNEL_SOURCES (the fp64 library's two aside) is chosen by at least one row, and the thinning kept what
    the tool asserts when it writes: every reachable refusal of the variant resolution and every lone-solve / on-chip-run difference of the dispatch order"""
    K = _tool()
    chosen = {name.split("<")[0] for nm in TABLE["names"] for name in nm[:2]}
    want = {k for k, src in tinympc.build.KERNEL_SOURCES.items() if not src.startswith("admm_f64_")}
    assert want <= chosen, sorted(want - chosen)
    assert set(K.FAMILIES) == want
    K.check_coverage(TABLE)
    assert sum(len(h["rows"]) for h in TABLE["handles"]) > 5000
    assert [K.spec_of(h) for h in TABLE["handles"]] == K.handle_specs(TABLE["cu"])


def test_selection_is_stated_once():
    """csrc/tinympc_batch.hip resolves a solve's kernel in resolve_plan and nowhere else: the names of the scattered forms are gone, the dispatch-order
    launchers and every solve launcher are each called from one place"""
    import re
    src = (ROOT / "accelerated-tinympc_amd" / "csrc" / "tinympc_batch.hip").read_text()
    for gone in ("closed_loop_run", "update_kname", "tb->kname", "row_family(", "resolve_variant", "family_keeps_fp32_duals", "kFam", "tile_variant"):
        assert gone not in src, gone
    assert not re.search(r"\bfam(_l)? [=!]= \d", src.replace("out.fam", "").replace("in.fam", "")), "a kernel family compared with an integer literal"
    assert src.count("launch_dispatch_order(") == 1 and src.count("launch_dispatch_order_history(") == 1
    for name in set(re.findall(r"launch_admm_\w+", src)) - {"launch_admm_step"}:
        assert src.count(name + "(") == 1, f"{name} is called from more than one place"
    # ... and so is whether a closed-loop run stays on chip (KernelPlan::loop): the trait is read once, the kind of call travels as a Call, and one
    # function (enqueue_solve) orders and launches a solve kernel
    assert src.split("constexpr const KernelTraits &traits(", 1)[1].count("onchip_mpc") == 1, "onchip_mpc is read outside resolve_plan's plan_of"
    for gone in ("bool sim = false", "bool closed_loop"):
        assert gone not in src, gone
    for name in ("launch_kernel(", "enqueue_dispatch_order("):
        assert src.count(name) == 2, f"{name} its definition and ONE call"
    assert len(re.findall(r"\bint mpc_run_sim\(", src)) == 1, "mpc_run_sim is declared once"


@pytest.fixture(scope="module")
def session():
    K = _tool()
    ses = K.Session(TABLE["long_rows"])
    if ses.cu != TABLE["cu"]:
        pytest.skip(f"the table was recorded on a device with {TABLE['cu']} CUs (the size rules are per CU); this one has {ses.cu}")
    return K, ses


@pytest.mark.gpu
@pytest.mark.parametrize("hi", range(len(TABLE["handles"])), ids=lambda i: "{cls[0]}_{cls[1]}_{cls[2]}-B{batch}-s{storage}".format(**TABLE["handles"][i]).replace(" ", ""))
def test_kernel_choice_matches_the_record(session, hi):
    K, ses = session
    h = TABLE["handles"][hi]
    want = K.unpack_rows(TABLE, h)
    got = ses.run(K.spec_of(h), [r[0] for r in want])
    assert got["storage_refused"] == h["storage_refused"]
    assert got["row_kernels_refused"] == h["row_kernels_refused"]
    assert len(got["rows"]) == len(want)
    for n, (w, g) in enumerate(zip(want, got["rows"])):
        assert g == w, f"row {n} {K.cfg_of(w[0])}: recorded {w[1:]}, now {g[1:]}"
