"""Build the HIP shared library (gfx950 only) in-tree.

    python accelerated-tinympc_amd/build.py [--force]

Produces accelerated-tinympc_amd/lib/libtinympc_hip.so with `hipcc --offload-arch=gfx950`.
hipcc cross-compiles without a GPU.  The .so is git-ignored but travels with the tree.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from types import SimpleNamespace
from typing import NamedTuple

PKG = Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIB = PKG / "lib" / "libtinympc_hip.so"
WRAPPER_LIB = PKG / "lib" / "libtinympc_wrapper.so"  # same-name twin of the reference's generated wrapper library
WRAPPER64_LIB = PKG / "lib" / "libtinympc_wrapper64.so"  # the native names (tiny_solve, forward_pass, ...) for tinytype = double
WRAPPER_SRCS = [CSRC / "wrapper_compat.cpp", CSRC / "admm_compat.cpp"]
HEADERS = [CSRC / "tinympc_internal.h", CSRC / "batch_helpers.h", CSRC / "eigen_orders.h", CSRC / "rowlane_math.h", CSRC / "tile_math.h", CSRC / "wave_math.h", CSRC / "dpp_ops_gen.h", CSRC / "f64_internal.h", CSRC / "f64_math.h", PKG.parent / "include" / "tinympc_batch.h", PKG.parent / "include" / "tinympc_batch64.h"]
# -ffp-contract=off : exact arithmetic must not fuse a*b+c; the fast paths call fma explicitly
# -fno-slp-vectorize: hipcc otherwise pairs scalar fp32 adds into v_pk_add_f32 (+ v_mov to build the pairs), which on
#                     gfx950 is slower than two plain v_add_f32 (measured, tools/micro/*.hip)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize", "-fno-gpu-rdc"]


class Unit(NamedTuple):
    """One translation unit of libtinympc_hip.so.  Everything build() and the tools know about a unit is its row of UNITS (or of ADDED_UNITS)."""
    source: str
    parent: str | None = None      # the kernel source it #includes (a variant unit: the parent's text compiled again): rebuilt with it
    flags: tuple = ()              # extra hipcc flags
    flags_env: str | None = None   # environment variable whose words are appended to flags (A/B runs of the tools)
    family: str | None = None      # the kernel-name prefix it serves (tiny_batch_kernel_name(), up to the '<')
    tails: tuple = ()              # name endings that route to this unit; the family's unit without tails is its default


# per-unit flags.  admm_tile16.hip: the max-ILP scheduling strategy (one wave per SIMD: nothing else hides a latency; measured
# 1.88 -> 1.79 ms, the other kernels do not react to it); MFMA results go to VGPRs (the sums that consume the exact products are VALU instructions,
# which cannot read the accumulator half of the register file: left to its heuristics hipcc parks the products there and
# copies every one of them back, 110 v_accvgpr_read per horizon step)
_MFMA_VGPR = ("-mllvm", "-amdgpu-mfma-vgpr-form=1")
_T16_FLAGS = _MFMA_VGPR + ("-mllvm", "-amdgpu-sched-strategy=max-ilp")
# in link order
UNITS = (
    Unit("tinympc_batch.hip"),
    Unit("batch_helpers.hip"),
    Unit("tinympc_batch64.hip"),
    Unit("batch64_helpers.hip"),
    Unit("admm_f64_thread.hip", family="thread64"),
    Unit("admm_f64_rows.hip", family="rows64"),
    Unit("admm_f64_rowsim.hip", "admm_f64_rows.hip", family="rows64", tails=(",sim>",)),
    Unit("admm_f64_plant.hip"),
    Unit("admm_f64_rows_pm.hip", "admm_f64_rows.hip", family="rows64", tails=(",pm>",)),
    Unit("admm_f64_rowsim_pm.hip", "admm_f64_rows.hip", family="rows64", tails=(",mpc,pm>", ",sim,pm>")),
    Unit("admm_f64_thread_pm.hip", "admm_f64_thread.hip", family="thread64", tails=(",pm>",)),
    Unit("admm_f64_rows_ps.hip", "admm_f64_rows.hip", family="rows64", tails=(",ps>",)),
    Unit("admm_f64_rowloop_ps.hip", "admm_f64_rows.hip", family="rows64", tails=(",mpc,ps>",)),
    Unit("admm_f64_thread_ps.hip", "admm_f64_thread.hip", family="thread64", tails=(",ps>",)),
    Unit("admm_stream.hip", family="stream"),
    Unit("admm_generic.hip", family="generic"),
    Unit("admm_rowlane.hip", family="rowlane", flags_env="TINYMPC_ROWLANE_FLAGS"),
    Unit("admm_rowsim.hip", "admm_rowlane.hip", flags_env="TINYMPC_ROWLANE_FLAGS"),  # (the simulated loop reports its MPC twin's name)
    Unit("admm_rowlane_ps.hip", "admm_rowlane.hip", family="rowlane", tails=(",ps>",), flags_env="TINYMPC_ROWLANE_FLAGS"),
    Unit("admm_rowloop.hip", family="rowloop"),
    Unit("admm_quadlane.hip", family="quadlane"),
    Unit("admm_tile16.hip", flags=_T16_FLAGS, flags_env="TINYMPC_T16_FLAGS", family="tile16"),
    Unit("admm_tile16_pi.hip", "admm_tile16.hip", flags=_T16_FLAGS, flags_env="TINYMPC_T16_FLAGS", family="tile16", tails=(",pi>",)),
    Unit("admm_wave.hip", family="wavestream"),
    Unit("admm_wave_pm.hip", "admm_wave.hip", family="wavestream", tails=(",pm>",)),
    Unit("admm_waveres.hip", flags_env="TINYMPC_WAVERES_FLAGS", family="waveres"),
    Unit("admm_waveres_pm.hip", "admm_waveres.hip", flags_env="TINYMPC_WAVERES_FLAGS", family="waveres", tails=(",pm>",)),
    Unit("admm_tile48.hip", flags=_MFMA_VGPR, flags_env="TINYMPC_T48_FLAGS", family="tile48"),
    Unit("admm_steps.hip", family="rowstream"),
    Unit("admm_steps_ps.hip", "admm_steps.hip", family="rowstream", tails=(",ps>",)),
    Unit("settings_helpers.hip"),
    Unit("dispatch_order.hip"),
    Unit("riccati.cpp"),
    Unit("riccati_batch.hip"),
)
# Units added since tests/golden/device_code.json was written.  That record is one of the suite's fixed files and has exactly the rows of UNITS, so a unit that
# arrives with a feature is listed here: compiled, linked (after UNITS, in this order) and routed like any other, and recorded by the same readers in the record
# beside it, tests/golden/device_code_added.json (tests/test_device_code_added.py; `python tools/device_code.py --write --added`).  A later feature adds its
# rows to this table and that record.  Here: the wave kernels' text compiled once more with per-instance settings, each a variant of its pm sibling's parent.
ADDED_UNITS = (
    Unit("admm_wave_ps.hip", "admm_wave.hip", family="wavestream", tails=(",ps>",)),
    Unit("admm_waveres_ps.hip", "admm_waveres.hip", flags_env="TINYMPC_WAVERES_FLAGS", family="waveres", tails=(",ps>",)),
)
ALL_UNITS = UNITS + ADDED_UNITS
# the views of the tables that build(), bench.py, the tests and the tools read
SOURCES = [u.source for u in UNITS]             # the units of the standing record
ADDED_SOURCES = [u.source for u in ADDED_UNITS]
LINKED_SOURCES = SOURCES + ADDED_SOURCES         # everything build() compiles and links: the rows of the two records together
INCLUDED_SOURCES = {u.source: [u.parent] for u in ALL_UNITS if u.parent}
EXTRA_FLAGS = {u.source: [*u.flags, *os.environ.get(u.flags_env or "", "").split()] for u in ALL_UNITS if u.flags or u.flags_env}
KERNEL_SOURCES = {u.family: u.source for u in ALL_UNITS if u.family and not u.tails}  # family -> its default unit


def unit_of(kernel_name: str) -> str | None:
    """The translation unit that holds the device code behind a kernel name such as 'tile16<12,4,30,exact,pi>': of the family's units the one
    with the longest matching tail, else the family's default unit; None for an unknown family."""
    family = kernel_name.split("<", 1)[0]
    tails = [(t, u.source) for u in ALL_UNITS if u.family == family for t in u.tails if kernel_name.endswith(t)]
    return max(tails, key=lambda t: len(t[0]))[1] if tails else KERNEL_SOURCES.get(family)


def _objs():
    return [(CSRC / s, PKG / "lib" / (Path(s).stem + ".o")) for s in LINKED_SOURCES if (CSRC / s).exists()]


def needs_build() -> bool:
    if not LIB.exists() or not WRAPPER_LIB.exists() or not WRAPPER64_LIB.exists():
        return True
    t = min(LIB.stat().st_mtime, WRAPPER_LIB.stat().st_mtime, WRAPPER64_LIB.stat().st_mtime)
    inc = PKG.parent / "include"
    deps = [s for s, _ in _objs()] + HEADERS + [Path(__file__), *WRAPPER_SRCS, inc / "tinympc_wrapper.h", inc / "tinympc_admm.h", inc / "tinympc_batch.h"]
    return any(d.stat().st_mtime > t for d in deps if d.exists())


def build(force: bool = False, verbose: bool = False) -> Path:
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    LIB.parent.mkdir(parents=True, exist_ok=True)
    hdr_t = max(h.stat().st_mtime for h in HEADERS + [Path(__file__)] if h.exists())
    stale = []
    for src, obj in _objs():
        src_t = max([src.stat().st_mtime] + [(CSRC / i).stat().st_mtime for i in INCLUDED_SOURCES.get(src.name, [])])
        if not force and obj.exists() and obj.stat().st_mtime > max(src_t, hdr_t):
            continue
        cmd = [hipcc, *FLAGS, *EXTRA_FLAGS.get(src.name, []), "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        stale.append((src, cmd))
    # started in table order, at most MAX_JOBS (and never more than 16) at a time
    with ThreadPoolExecutor(min(int(os.environ.get("MAX_JOBS", "16")), 16)) as pool:
        for (src, _), rc in zip(stale, pool.map(lambda c: subprocess.run(c[1]).returncode, stale)):
            if rc != 0:
                raise RuntimeError(f"hipcc failed on {src}")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB)] + [str(o) for _, o in _objs()]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    # libtinympc_wrapper.so: plain host C++ on top of the C-ABI, finds libtinympc_hip.so next to itself
    cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", str(WRAPPER_LIB), *[str(w) for w in WRAPPER_SRCS], f"-L{LIB.parent}",
           "-ltinympc_hip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    # libtinympc_wrapper64.so: the native names over TinySolver with double members (include/tinympc_admm.h, TINYMPC_TINYTYPE_DOUBLE)
    cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-DTINYMPC_TINYTYPE_DOUBLE", "-o", str(WRAPPER64_LIB), str(CSRC / "admm_compat.cpp"),
           f"-L{LIB.parent}", "-ltinympc_hip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB


def device_asm(source: str) -> Path:
    """gfx950 assembly listing of one kernel source, compiled with exactly the flags of build() (`hipcc -S --cuda-device-only`);
    cached under lib/asm/ and redone when the source or a header is newer.  Used by tests/test_isa.py (static hazard and
    register-spill guards over what the compiler actually emitted) and by the developer tools under tools/."""
    src = CSRC / source
    out = PKG / "lib" / "asm" / (Path(source).stem + ".s")
    out.parent.mkdir(parents=True, exist_ok=True)
    newest = max(d.stat().st_mtime for d in [src, Path(__file__), *HEADERS, *[CSRC / i for i in INCLUDED_SOURCES.get(source, [])]] if d.exists())
    if not out.exists() or out.stat().st_mtime < newest:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, *[f for f in FLAGS if f != "-fPIC"], *EXTRA_FLAGS.get(source, []), "-S", "--cuda-device-only", str(src), "-o", str(out)]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def _elf_sections(b: bytes, base: int = 0) -> dict:
    import struct
    assert b[base:base + 4] == b"\x7fELF", "not an ELF image"
    shoff = struct.unpack_from("<Q", b, base + 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, base + 0x3A)
    secs = [struct.unpack_from("<IIQQQQ", b, base + shoff + i * shentsize) for i in range(shnum)]
    stro = base + secs[shstrndx][4]
    out = {}
    for name, typ, _flags, _addr, off, size in secs:
        out[b[stro + name:b.index(b"\0", stro + name)].decode()] = (base + off, size, typ)
    return out


def device_isa_sha(source: str) -> str:
    """sha256 (16 hex digits) over the gfx950 machine code (.text) and kernel descriptors (.rodata) of one translation unit, read from
    the object file build() left in lib/ — the clang offload bundle inside its .hip_fatbin section, parsed here (no tool is executed:
    bench.py calls this with the GPU initialised).  It binds a measured figure (profiles/hbm_traffic.json) to the CODE it was taken
    on: unlike a hash of the source text it does not move when a comment does."""
    import hashlib
    import struct
    obj = PKG / "lib" / (Path(source).stem + ".o")
    b = obj.read_bytes()
    off, size, _ = _elf_sections(b)[".hip_fatbin"]
    fb = b[off:off + size]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    assert fb.startswith(magic), "uncompressed clang offload bundle expected"
    n = struct.unpack_from("<Q", fb, len(magic))[0]
    p = len(magic) + 8
    h = hashlib.sha256()
    found = False
    for _ in range(n):
        eo, es, ts = struct.unpack_from("<QQQ", fb, p)
        p += 24
        triple = fb[p:p + ts].decode()
        p += ts
        if "gfx950" in triple and es:
            found = True
            secs = _elf_sections(fb, eo)
            for name in (".text", ".rodata"):
                if name in secs and secs[name][2] != 8:  # (8 = SHT_NOBITS)
                    o, sz, _ = secs[name]
                    h.update(fb[o:o + sz])
    assert found, f"no gfx950 code object in {obj}"
    return h.hexdigest()[:16]


def kernel_isa_sha(kernel_name: str) -> str | None:
    """device_isa_sha of the translation unit behind a kernel name such as 'tile16<12,4,30,exact>'; None for an unknown family or a missing object."""
    src = unit_of(kernel_name)
    try:
        return device_isa_sha(src) if src else None
    except (OSError, AssertionError, KeyError):
        return None


# the added units as isa_tools.device_code() reads a build: its SOURCES and the two readers
ADDED = SimpleNamespace(SOURCES=ADDED_SOURCES, device_isa_sha=device_isa_sha, device_asm=device_asm)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
