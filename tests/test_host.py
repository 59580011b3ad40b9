"""CPU tests of the host side: C-ABI surface, Riccati host routine, problem data."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]


def test_library_builds_loads_and_exports_every_declared_symbol(tinympc):
    tinympc.build.build()
    lib = tinympc.load_library()
    syms = tinympc.exported_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/tinympc_batch.h but not exported"
    hdr = (ROOT / "include" / "tinympc_batch.h").read_text()
    # every declaration cites the reference interface it replaces
    assert "tiny_wrapper.hpp:14-23" in hdr and "admm.cpp:111-152" in hdr and "types.hpp:26-34" in hdr


def test_product_does_not_reference_the_oracle():
    """The shipped path must not import, link or call anything under oracle/."""
    pkg = ROOT / "accelerated-tinympc_amd"
    for p in list(pkg.rglob("*.py")) + list(pkg.rglob("*.hip")) + list(pkg.rglob("*.cpp")) + list(pkg.rglob("*.h")):
        txt = p.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle", txt, re.M), p
        assert "libtinympc_oracle" not in txt and "oracle/" not in txt.replace("oracle/ ", ""), p
    # outside the package, only tests/, __graft_entry__.py (smoke) and bench.py (cpu_baseline) may import the oracle
    allowed = {ROOT / "bench.py", ROOT / "__graft_entry__.py"}
    for d in ("tools", "examples", "include"):
        for p in (ROOT / d).rglob("*"):
            if p.is_file() and p.suffix in (".py", ".sh", ".cpp", ".h", ".hip"):
                txt = p.read_text()
                assert not re.search(r"^\s*(from|import)\s+oracle|from oracle import|libtinympc_oracle", txt, re.M), p
    for p in ROOT.glob("*.py"):
        if p not in allowed:
            assert not re.search(r"^\s*(from|import)\s+oracle|from oracle import", p.read_text(), re.M), p
    # bench.py touches the oracle only inside its cpu_baseline leg
    import ast
    tree = ast.parse((ROOT / "bench.py").read_text())
    for fn in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.Module))]:
        body = fn.body if isinstance(fn, ast.Module) else [n for n in ast.walk(fn)]
        for n in body:
            if isinstance(n, (ast.Import, ast.ImportFrom)):
                mods = [a.name for a in n.names] + [getattr(n, "module", "") or ""]
                if any(m.split(".")[0] == "oracle" for m in mods):
                    assert isinstance(fn, ast.FunctionDef) and fn.name == "cpu_baseline", (fn, n.lineno)


def test_host_riccati_matches_reference_codegen(tinympc):
    for name, nx, nu in (("riccati_cartpole", 4, 1), ("riccati_random_32_16", 32, 16)):
        z = np.load(GOLDEN / f"{name}.npz")
        c = tinympc.riccati(nx, nu, z["A"], z["B"], z["Q"], z["R"], float(z["rho"]))
        for k in ("Kinf", "Pinf", "Quu_inv", "AmBKt"):
            np.testing.assert_allclose(c[k], z[k], rtol=1e-8, atol=1e-9 * np.max(np.abs(z[k])))
        if nx == 4:
            assert c["iters"] == 476
    # the shipped quadrotor cache is a fixed point of the same recursion (params.hpp values, 7 decimals)
    q = tinympc.problems.quadrotor(20, 30)
    c = tinympc.riccati(12, 4, q["Adyn"], q["Bdyn"], q["Q"], q["R"], q["rho"])
    np.testing.assert_allclose(c["Kinf"], q["Kinf"], atol=5e-3)
    np.testing.assert_allclose(c["Quu_inv"], q["Quu_inv"], atol=1e-4)


def test_riccati_rejects_bad_arguments(tinympc):
    lib = tinympc.load_library()
    assert lib.tiny_riccati(0, 1, None, None, None, None, 1.0, None, None, None, None, None, None) < 0


def test_trajectory_matches_reference_header(tinympc):
    X = tinympc.problems.y_axis_line()
    assert X.shape == (301, 12) and X[300, 7] == 0.0 and X[0, 7] == 0.2666667 and X[300, 1] == 4.0
    # the numbers of the reference's quadrotor_20hz_y_axis_line.hpp (tests/golden/make_golden.py reference_headers)
    vals = np.load(GOLDEN / "reference_headers.npz")["y_axis_line"]
    assert vals.size == 301 * 12
    assert np.array_equal(vals.reshape(301, 12), X)


def test_problem_data_matches_reference_headers(tinympc):
    # the <name>_data arrays of the reference's quadrotor_20hz_params.hpp (tests/golden/make_golden.py reference_headers)
    z = np.load(GOLDEN / "reference_headers.npz")
    q = tinympc.problems.quadrotor(20, 30)
    for name in ("Adyn", "Bdyn", "Kinf", "Pinf", "Quu_inv", "AmBKt", "Q", "R"):
        vals = z["quadrotor_20hz_" + name]
        assert np.array_equal(vals, np.asarray(q[name]).ravel()), name
    assert q["rho"] == 5.0


def test_batch_generators_are_deterministic(tinympc):
    pr = tinympc.problems
    a, t, s = pr.tracking_batch(100, 30)
    b, _, s2 = pr.tracking_batch(100, 30)
    assert np.array_equal(a, b) and np.array_equal(s, s2) and s.max() + 30 <= 301
    w = pr.expand_windows(t, s, 30)
    assert w.shape == (100, 30, 12) and np.array_equal(w[5, 3], t[s[5] + 3])
    x0, xr = pr.hover_batch(10, 30)
    assert x0.shape == (10, 12) and xr.shape == (30, 12) and xr[0, 2] == 2.0


def test_cpp_example_compiles_and_links_against_the_c_abi(tinympc, tmp_path):
    """examples/quadrotor_tracking_batched.cpp uses nothing but include/tinympc_batch.h: plain g++ must build it."""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tinympc.build.build()
    lib_dir = ROOT / "accelerated-tinympc_amd" / "lib"
    out = tmp_path / "example"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                        str(ROOT / "examples" / "quadrotor_tracking_batched.cpp"), f"-L{lib_dir}", "-ltinympc_hip",
                        f"-Wl,-rpath,{lib_dir}", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (ROOT / "accelerated-tinympc_amd" / "data" / "quadrotor_20hz.bin").stat().st_size == 557 * 8
    # the multi-device example (one handle per GPU, group solve, device-to-device gather) is the C-ABI only as well
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                        str(ROOT / "examples" / "quadrotor_tracking_multigpu.cpp"), f"-L{lib_dir}", "-ltinympc_hip",
                        f"-Wl,-rpath,{lib_dir}", "-o", str(tmp_path / "multigpu")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the hovering example over the reference's own names (include/tinympc_admm.h) links against the wrapper library
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}",
                        str(ROOT / "examples" / "quadrotor_hovering_native.cpp"), f"-L{lib_dir}", "-ltinympc_wrapper",
                        f"-Wl,-rpath,{lib_dir}", "-o", str(tmp_path / "hover_native")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # ... and, as the reference is checked in (typedef double tinytype, N = 10), against the double build of the same names
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DTINYMPC_TINYTYPE_DOUBLE", f"-I{ROOT / 'include'}",
                        str(ROOT / "examples" / "quadrotor_hovering_native.cpp"), f"-L{lib_dir}", "-ltinympc_wrapper64",
                        f"-Wl,-rpath,{lib_dir}", "-o", str(tmp_path / "hover_native64")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def reference_names():
    """Function and member names of the reference's headers, recorded in tests/golden/reference_headers.npz."""
    import json
    return json.loads(bytes(np.load(GOLDEN / "reference_headers.npz")["names"]).decode())


WRAPPER_SYMBOLS = ["set_x0", "set_xref", "set_umin", "set_umax", "set_xmin", "set_xmax", "reset_dual_variables",
                   "call_tiny_solve", "get_x", "get_u"]  # src/tinympc/tiny_wrapper.hpp:14-23


def test_wrapper_library_exports_the_reference_wrapper_names(tinympc):
    tinympc.build.build()
    lib = C.CDLL(str(ROOT / "accelerated-tinympc_amd" / "lib" / "libtinympc_wrapper.so"))
    for s in WRAPPER_SYMBOLS + ["tiny_wrapper_setup", "tiny_wrapper_teardown", "tiny_wrapper_last_status"]:
        assert hasattr(lib, s), s
    # the ten names are exactly the functions of the reference's tiny_wrapper.hpp
    assert sorted(reference_names()["tiny_wrapper_functions"]) == sorted(WRAPPER_SYMBOLS)
    # before setup every call is a reported no-op, never a crash
    lib.reset_dual_variables(0)
    assert lib.tiny_wrapper_last_status(None, None) < 0
    # the generated library also exports four DATA symbols (codegen.cpp:470, :513; SURVEY.md section 8(b) `nm -D` row): a foreign
    # caller that pokes tiny_data_solver links, and tiny_data_solver points at the other three
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "accelerated-tinympc_amd" / "lib" / "libtinympc_wrapper.so")], capture_output=True, text=True).stdout
    data = {l.split()[-1]: l.split()[-2] for l in nm.splitlines() if len(l.split()) >= 3}
    for sym in ("settings", "cache", "work", "tiny_data_solver"):
        assert data.get(sym) in ("B", "D"), (sym, data.get(sym))   # bss / initialised data, not functions
    ptrs = (C.c_void_p * 3).in_dll(lib, "tiny_data_solver")
    assert [ptrs[0], ptrs[1], ptrs[2]] == [C.addressof(C.c_char.in_dll(lib, n)) for n in ("settings", "cache", "work")]


def test_every_function_declared_in_the_wrapper_headers_is_exported(tinympc):
    """include/tinympc_wrapper.h and include/tinympc_admm.h: every declared function is a symbol of libtinympc_wrapper.so."""
    tinympc.build.build()
    lib = C.CDLL(str(ROOT / "accelerated-tinympc_amd" / "lib" / "libtinympc_wrapper.so"))
    for hdr in ("tinympc_wrapper.h", "tinympc_admm.h"):
        txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / hdr).read_text(), flags=re.S)
        names = re.findall(r"^\s*(?:int|void|bool|const char \*)\s*(\w+)\s*\(", txt, re.M)
        assert len(names) >= 8, (hdr, names)
        for n in names:
            assert hasattr(lib, n), f"{n} declared in include/{hdr} but not exported"
    assert hasattr(lib, "tiny_admm_set_optional_terms")


def test_double_native_names_library(tinympc, tmp_path):
    """libtinympc_wrapper64.so (include/tinympc_admm.h under TINYMPC_TINYTYPE_DOUBLE): the header compiles as C with double
    members, the library exports the reference's eight function names, and the ctypes structs have the compiled layout."""
    from accelerated_tinympc_amd import native
    tinympc.build.build()
    lib = C.CDLL(str(ROOT / "accelerated-tinympc_amd" / "lib" / "libtinympc_wrapper64.so"))
    for s in NATIVE_SYMBOLS + ["tiny_admm_set_device", "tiny_admm_last_error_code", "tiny_admm_set_optional_terms"]:
        assert hasattr(lib, s), s
    src = tmp_path / "layout64.c"
    members = ["nx", "x", "y", "primal_residual_state", "iter", "Q", "Xref"]
    src.write_text('#define TINYMPC_TINYTYPE_DOUBLE\n#include <stdio.h>\n#include <stddef.h>\n#include "tinympc_admm.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(tinytype), sizeof(TinyCache), sizeof(TinySettings), sizeof(TinyWorkspace), sizeof(TinySolver));\n' +
                   "".join(f'printf("%zu\\n", offsetof(TinyWorkspace, {m}));\n' for m in members) + "return 0;}\n")
    exe = tmp_path / "layout64"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    TC, TS, TW, TSo = native.TYPES64
    assert out[:5] == [8, C.sizeof(TC), C.sizeof(TS), C.sizeof(TW), C.sizeof(TSo)]
    assert out[5:] == [getattr(TW, m).offset for m in members]


NATIVE_SYMBOLS = ["tiny_solve", "update_primal", "backward_pass_grad", "forward_pass", "update_slack", "update_dual",
                  "update_linear_cost", "termination_condition"]  # src/tinympc/admm.hpp:10-18


def test_native_names_header_is_plain_c_and_matches_the_binding(tinympc, tmp_path):
    """include/tinympc_admm.h compiles as C, declares the functions of the reference's admm.hpp under the same names,
    the library exports them, and the ctypes structs of native.py have the compiled layout."""
    from accelerated_tinympc_amd import native
    tinympc.build.build()
    lib = C.CDLL(str(ROOT / "accelerated-tinympc_amd" / "lib" / "libtinympc_wrapper.so"))
    for s in NATIVE_SYMBOLS:
        assert hasattr(lib, s), s
    assert sorted(reference_names()["admm_functions"]) == sorted(NATIVE_SYMBOLS)   # the functions of the reference's admm.hpp
    members = ["nx", "x", "y", "primal_residual_state", "iter", "Q", "Bdyn", "u_min", "Xref", "Qu"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tinympc_admm.h"\nint main(void){\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(TinyCache), sizeof(TinySettings), sizeof(TinyWorkspace), sizeof(TinySolver));\n' +
                   "".join(f'printf("%zu\\n", offsetof(TinyWorkspace, {m}));\n' for m in members) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:4]] == [C.sizeof(native.TinyCache), C.sizeof(native.TinySettings),
                                         C.sizeof(native.TinyWorkspace), C.sizeof(native.TinySolver)]
    assert [int(v) for v in out[4:]] == [getattr(native.TinyWorkspace, m).offset for m in members]
    # member names and order are the reference's (types.hpp:52-97), with nx,nu,N in front and pointers for matrices
    assert [f[0] for f in native.TinyWorkspace._fields_[3:]] == reference_names()["workspace_members"]


@pytest.mark.parametrize("name", ["r01_bench_default_line.json", "r02_bench_default_line_d.json", "r02_bench_random32_line_b.json",
                                  "r04_bench_default_line_a.json", "r04_bench_random32_line_a.json", "r04_bench_default_line_b.json", "r04_bench_random32_line_b.json", "r04_bench_default_line_c.json", "r04_bench_random32_line_c.json",
                                  "r04_bench_default_line_d.json", "r04_bench_random32_line_d.json", "r04_bench_default_line_e.json"])
def test_recorded_bench_line_has_the_contract_fields(name):
    """profiles/*_bench_*_line*.json are the stdout of `python bench.py [--config random32]` on the MI355X: the keys the driver reads."""
    import json
    d = json.loads((ROOT / "profiles" / name).read_text())
    if name.startswith("r04"):   # round 4: what the round-3 review asked the line to carry so that it can be checked without trusting it
        ac = d["cpu_baseline"]["all_cores"]   # the COMPILED REFERENCE on every usable host core, one process per core
        assert ac["kind"] == "reference" and ac["cores"] == ac["processes"] == d["cpu_baseline"]["host_cores_usable"] and ac["value"] > d["cpu_baseline"]["value"]
        assert "march=native" not in d["cpu_baseline"]["port_all_cores"]["build"].replace("no -march=native", "")
        t = d["transfers"]                     # H2D / D2H timed separately, never part of `value`
        assert t["h2d_ms"] > 0 and t["d2h_ms"] > 0 and t["h2d_bytes"] == d["config"]["instances_per_gpu"] * d["config"]["nx"] * 4
        assert t["pcie_inclusive_solves_per_s"] < d["value"]
        f = d["fixed10"]                       # fixed-iteration throughput in exact arithmetic next to the early-exit headline
        assert f["iterations"] == 10 and f["kernel"].endswith("exact>") and f["solves_per_s"] > d["value"]
        assert d["roofline"]["traffic"] > 0 and "device code" in d["roofline"]["traffic_note"]   # bound to the kernel's ISA, not to the source text
    if name.startswith(("r02", "r04")):   # round 2 made the line self-describing
        assert d["config"]["world_size_seen"] == d["n_gpus"] and "backend" in d["config"] and d["config"]["instances_total"] > 0
        assert d["parity"]["bitwise_u"] is True and d["parity"]["iter_mismatch"] == 0 and d["parity"]["status_mismatch"] == 0
        kk = d["roofline"]["kernel_ms_per_step"]
        assert kk["min"] <= kk["median"] <= kk["max"] and kk["n"] >= 5
        assert d["roofline"]["kernel"].endswith("exact>")   # the exact kernel is the one `value` is measured on
    if "random32" in name:
        assert d["scaling"] == "strong" and d["config"]["nx"] == 32
        d = dict(d, scaling="weak")   # the remaining checks are shared with the weak-scaling default line
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "solves/s" and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["traffic"] is None or r["traffic"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    # value is the throughput of the timed steps
    assert abs(d["value"] - d["config"]["instances_per_gpu"] * d["n_gpus"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
