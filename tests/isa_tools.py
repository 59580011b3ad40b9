"""Readers of the gfx950 listings `hipcc -S` writes (build.device_asm): the kernels of a listing and their instruction lines, the DPP hazard
checker, register and scratch figures, the fingerprints that pin instruction streams, and the rows of tests/golden/device_code.json.  Shared by
the tests/test_isa*.py modules, tests/test_device_code.py and tools/device_code.py; no test lives here."""
import hashlib
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

VALU_EXEC_WRITERS = ("v_cmpx",)


def kernels_of(listing: str):
    """{mangled name: [instruction lines]} for every kernel (function body up to its .amdhsa_kernel / end marker)."""
    out, cur, name = {}, None, None
    for line in listing.split("\n"):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            name, cur = m.group(1), []
            out[name] = cur
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end") or line.lstrip().startswith(".amdhsa_kernel") or line.lstrip().startswith(".section"):
            cur = None
            continue
        t = line.strip()
        if not t or t[0] in ";." and not re.match(r"^\.LBB\d+_\d+:", t):
            continue
        cur.append(t.split(";")[0].strip())
    return out


def regs(op: str):
    """VGPR numbers named by one operand: v7 -> {7}, v[4:7] -> {4,5,6,7}; anything else -> {}."""
    op = op.strip().rstrip(",")
    op = re.sub(r"^[-|]+|[|]+$", "", op)
    m = re.match(r"^v(\d+)$", op)
    if m:
        return {int(m.group(1))}
    m = re.match(r"^v\[(\d+):(\d+)\]$", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def is_dpp(ins: str):
    return "_dpp" in ins.split()[0] or re.search(r"\b(row_newbcast|row_shr|row_shl|row_ror|row_bcast|quad_perm|row_mirror|row_half_mirror|wave_shr|wave_ror|row_share|row_xmask):?", ins) is not None


def hazards(lines):
    """[(index, text, reason)] of DPP instructions with a VALU write of their DPP source less than 2 wait states ahead, or a VALU
    write of EXEC less than 5 wait states ahead.  Labels end the look-back (another path may join there)."""
    bad = []
    for i, ins in enumerate(lines):
        if ins.endswith(":") or not ins.startswith("v_") or not is_dpp(ins):
            continue
        ops = [o for o in re.split(r",\s*", ins.split(None, 1)[1])] if len(ins.split(None, 1)) > 1 else []
        if len(ops) < 2:
            continue
        src = regs(ops[1].split()[0])  # src0 is the operand that goes through the DPP network
        ws, j = 0, i - 1
        while j >= 0 and ws < 5:
            p = lines[j]
            if p.endswith(":"):
                break
            op = p.split()[0]
            if op == "s_nop":
                ws += int(p.split()[1]) + 1
                j -= 1
                continue
            if op.startswith("v_") and not op.startswith(("v_cmp_", "v_readlane", "v_readfirstlane")):
                if op.startswith(VALU_EXEC_WRITERS):
                    bad.append((i, ins, f"VALU write of EXEC {ws} wait states ahead: {p}"))
                elif ws < 2:
                    pops = p.split(None, 1)[1] if len(p.split(None, 1)) > 1 else ""
                    dst = regs(re.split(r",\s*", pops)[0]) if pops else set()
                    if dst & src:
                        bad.append((i, ins, f"VALU write of the DPP source {ws} wait states ahead: {p}"))
            ws += 1
            j -= 1
    return bad


def scratch_sizes(listing: str):
    out, name = {}, None
    for line in listing.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r"^; ScratchSize: (\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    return out


def iteration_loop(lines):
    """(first, last) line of the ADMM iteration loop of a tile16 kernel: the innermost loop of the listing that contains the MFMAs of a whole
    iteration (58 unrolled sweep steps); the tile-queue loop around it is longer."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.search(r"s_branch\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 10 ** 9) < i:
            loops.append((labels[m.group(1)], i))
    with_mfma = [(a, b) for a, b in loops if sum(1 for l in lines[a:b] if l.startswith("v_mfma")) >= 200]
    assert with_mfma
    return min(with_mfma, key=lambda t: t[1] - t[0])


def figures(listing, kernel, want):
    """{template literals: (VGPRs, AGPRs, scratch, waves per SIMD)} of the instantiations of `kernel` whose mangled name satisfies want(name)"""
    out = {}
    for m in re.finditer(rf"^(_Z\w*\d+{kernel}I\w*):", listing, re.M):
        if not want(m.group(1)):
            continue
        tail = listing[m.start():]
        g = lambda k: int(re.search(rf"^; {k}: (\d+)", tail, re.M).group(1))
        out[tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))] = (g("NumVgprs"), g("NumAgprs"), g("ScratchSize"), g("Occupancy"))
    return out


def loop_figures(listing, want_sim):
    """{(NX, NU, N, RT): (VGPRs, AGPRs, scratch, waves per SIMD)} of the closed-loop instantiations of admm_f64_rows_kernel in a listing"""
    out = {}
    for m in re.finditer(r"^(_Z\w*admm_f64_rows_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb1E\w*):", listing, re.M):
        if ("Sim64" in m.group(1)) != want_sim:
            continue
        tail = listing[m.start():]
        g = lambda k: int(re.search(rf"^; {k}: (\d+)", tail, re.M).group(1))
        out[tuple(int(v) for v in m.groups()[1:])] = (g("NumVgprs"), g("NumAgprs"), g("ScratchSize"), g("Occupancy"))
    return out


def kernel_key(name):
    """mangled kernel name -> what it instantiates: (kernel, template literals, closed loop, simulated)"""
    base = re.search(r"\d+([a-z_0-9]+?_kernel)", name).group(1)
    lits = tuple(int(v) for v in re.findall(r"L[ib](\d+)E", name))
    return (base, lits, "Mpc64" in name, "Sim64" in name)


def fingerprint(listings):
    """(kernels, instruction lines, sha256[:16]) over the instruction streams of every kernel of the listings, whichever unit holds it and whatever
    it is called there: keyed by kernel_key, block labels unnumbered, the kernel's own name replaced"""
    ks = {}
    for text in listings:
        for name, lines in kernels_of(text).items():
            k = kernel_key(name)
            assert k not in ks, k
            ks[k] = [re.sub(r"\.LBB\d+_", ".LBB_", l).replace(name, "K") for l in lines]
    h = hashlib.sha256()
    for k in sorted(ks):
        h.update((repr(k) + "\n" + "\n".join(ks[k]) + "\n").encode())
    return len(ks), sum(map(len, ks.values())), h.hexdigest()[:16]


def unit_fingerprint(listing):
    """(kernels, instruction lines, sha256[:16]) of ONE unit's listing as tests/golden/device_code.json records it: the kernels sorted by mangled
    name, each its name and its instruction lines, block labels unnumbered as in fingerprint()"""
    ks = kernels_of(listing)
    h = hashlib.sha256()
    for name in sorted(ks):
        h.update((name + "\n" + "\n".join(re.sub(r"\.LBB\d+_", ".LBB_", l) for l in ks[name]) + "\n").encode())
    return len(ks), sum(map(len, ks.values())), h.hexdigest()[:16]


def device_code(build):
    """What tests/golden/device_code.json records, from the tree `build` belongs to: the first line of `hipcc --version` and, for every unit of
    build.SOURCES, {isa_sha, kernels, instructions, fingerprint} from the object build() left (device_isa_sha) and the listing (device_asm, made
    a bounded number at a time); a unit whose object holds no device code records None / 0"""
    def row(unit):
        try:
            sha = build.device_isa_sha(unit)
        except KeyError:   # no .hip_fatbin section: a host-only unit
            return {"isa_sha": None, "kernels": 0, "instructions": 0, "fingerprint": None}
        n, lines, fp = unit_fingerprint(build.device_asm(unit).read_text())
        return {"isa_sha": sha, "kernels": n, "instructions": lines, "fingerprint": fp}
    version = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True, check=True).stdout
    with ThreadPoolExecutor(min(int(os.environ.get("MAX_JOBS", "16")), 16)) as pool:
        return {"hipcc": version.strip().splitlines()[0].strip(), "units": dict(zip(build.SOURCES, pool.map(row, build.SOURCES)))}


def moved_units(record, built):
    """the units whose row differs between two device_code() records, a unit only one of them has included"""
    return [u for u in dict.fromkeys([*record["units"], *built["units"]]) if record["units"].get(u) != built["units"].get(u)]
