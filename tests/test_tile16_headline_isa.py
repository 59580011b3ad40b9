"""Static checks of the headline instantiations admm_tile16_kernel<N, exact, cold> on the listing the compiler emitted (CPU test, like
tests/test_isa.py; the listing helpers are those of tests/isa_tools.py).

These instantiations run each sweep of an ADMM iteration under ONE narrowed EXEC (admm_tile16.hip: exec_narrow / exec_restore) instead of
narrowing it around each of the sixty state updates.  hipcc is not told about the narrowed EXEC, so what it emitted is checked here, inside
the iteration loop:

  1. its size (N = 30): at most the instruction count reached when this was written, with all 261 MFMAs and no scratch access;
  2. the EXEC writes: the two asm pairs and the one structured `if (active)` of the termination check;
  3. that the sweeps are inside the pairs;
  4. two register rules.  A lane that is switched off skips every vector instruction of a region except the MFMAs (which ignore EXEC), so
     after the region each of its registers holds what it held at the region's entry.
     HOME: a value the compiler carries through the region is right in such a lane only if it sits in the SAME register at the end as at the
     entry and no MFMA of the region wrote that register.  The check follows every register of the entry through the region's copies (v_mov,
     v_accvgpr_read / _write) and through the tied state writes of the asm statements (which update a register in place).
     OPERAND: an MFMA reads its A operand (the gain block: lane c holds row c) from ALL lanes, those of switched-off instances included, and
     these feed the products of the active columns: a register that an MFMA of the region reads as A must not be written anywhere in the
     region — a copy, a rematerialisation or a reload under the narrowed EXEC would leave the switched-off lanes stale.
     Neither rule covers a value that is MADE inside a region and read under full EXEC behind it: by the design these are the four residual
     maxima alone, which `active` guards (the bitwise GPU tests are the check of that).
"""
import re

import pytest

import accelerated_tinympc_amd as T
from isa_tools import iteration_loop, kernels_of, scratch_sizes

HEAD = "admm_tile16_kernelILi{N}ELb1ELb1ELb0ELb0ELb0EEE"
# loop size of the N = 30 kernel, instructions per ADMM iteration (labels not counted): the parent of this change 4 794 (60 EXEC regions, the
# per-step clamp of the window row, two counted LDS waits per sweep step), this change 4 452
LOOP_PARENT = 4794
LOOP_PIN = 4452
HORIZONS = (30, 25, 20, 10)   # every horizon's instantiation runs its sweeps the same way; the size is pinned for the headline one


def loop_of(lines, n_mfma):
    """test_isa.iteration_loop for any horizon: the shortest backward-branch loop that holds the MFMAs of a whole iteration"""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 10 ** 9) < i:
            loops.append((labels[m.group(1)], i))
    loops = [(a, b) for a, b in loops if sum(1 for l in lines[a:b] if l.startswith("v_mfma")) >= n_mfma]
    assert loops
    return min(loops, key=lambda t: t[1] - t[0])


def loop_parts(N):
    txt = T.build.device_asm("admm_tile16.hip").read_text()
    ks = kernels_of(txt)
    (name,) = [k for k in ks if HEAD.format(N=N) in k]
    lines = ks[name]
    a, b = loop_of(lines, 9 * (N - 1))
    if N == 30:
        assert (a, b) == iteration_loop(lines)
    strip = lambda ls: [l for l in ls if not l.endswith(":")]
    return {"N": N, "body": strip(lines[a:b + 1]), "after": strip(lines[b + 1:]), "scratch": scratch_sizes(txt)[name]}


@pytest.fixture(scope="module")
def head():
    return loop_parts(30)


@pytest.fixture(scope="module", params=HORIZONS)
def any_head(request):
    return loop_parts(request.param)


def reg_set(op):
    """registers named by one operand: v7 -> {'v7'}, a[4:7] -> {'a4', .., 'a7'}; anything else -> {}"""
    op = re.sub(r"^[-|]+|[|]+$", "", op.strip())
    m = re.match(r"^([va])(\d+)$", op)
    if m:
        return [m.group(1) + m.group(2)]
    m = re.match(r"^([va])\[(\d+):(\d+)\]$", op)
    if m:
        return [f"{m.group(1)}{i}" for i in range(int(m.group(2)), int(m.group(3)) + 1)]
    return []


def operands(ins):
    parts = ins.split(None, 1)
    return [o.split()[0] for o in re.split(r",\s*", parts[1])] if len(parts) > 1 else []


def is_narrow(l):
    return l.startswith("s_and_saveexec_b64")


def is_restore(l):
    return re.match(r"s_(mov|or)_b64 exec,", l) is not None


def regions(body):
    """[(first, last)] of the instructions between a narrowing of EXEC and the write that restores it"""
    out, start = [], None
    for k, l in enumerate(body):
        if is_narrow(l):
            assert start is None, "nested narrowing"
            start = k
        elif is_restore(l):
            assert start is not None
            out.append((start, k))
            start = None
    assert start is None
    return out


def tied_writes(body, a, b):
    """indices of the asm statements' state writes inside [a, b]: the raw (suffix-less) v_sub_f32 / v_add_f32 and the accumulator writes that
    stand directly in front of the statement's last instruction (four before the ds_write_b128, three before the raw v_add_f32)"""
    tied = set()
    for k in range(a, b + 1):
        l = body[k]
        if re.match(r"v_(sub|add)_f32 v\d+,", l):
            tied.add(k)
        n = 4 if l.startswith("ds_write_b128") else 3 if re.match(r"v_add_f32 v\d+,", l) else 0
        for j in range(k - n, k):
            assert body[j].startswith("v_accvgpr_write_b32 a"), (k, l, body[j])
            tied.add(j)
    return tied


def accesses(l, tied=False):
    """(registers written, registers read) by one instruction; a tied state write reads what it writes over (the lanes that are off keep it)"""
    mn = l.split()[0]
    ops = operands(l)
    if mn.startswith("s_") or not ops:
        return [], []
    has_dst = not re.search(r"store|ds_write|^s_", mn)
    dst = reg_set(ops[0]) if has_dst else []
    src = [r for o in ops[1 if has_dst else 0:] for r in reg_set(o)]
    return dst, src + (dst if tied else [])


def live_after(r, seqs):
    """whether register r is read before it is written on one of the instruction sequences that follow the region"""
    for seq in seqs:
        for l, tied in seq:
            dst, src = accesses(l, tied)
            if r in src:
                return True
            if r in dst:
                break
    return False


def home_violations(body, a, b, after=()):
    """registers that, at the end of the region [a, b], hold a value of the region's entry that (a) entered in ANOTHER register or (b) sat in a
    register an MFMA of the region wrote — and that are read again before they are written: around the loop once, or (`after`) behind it"""
    tied = tied_writes(body, a, b)
    all_tied = set()
    for ra, rb in regions(body):
        all_tied |= tied_writes(body, ra, rb)
    marked = [(l, k in all_tied) for k, l in enumerate(body)]
    seqs = [marked[b + 1:] + marked[:b + 1], marked[b + 1:] + [(l, False) for l in after]]
    var, clobbered = {}, set()   # register -> the entry register whose value it carries (absent: itself); None: a value made inside the region

    def get(r):
        return var.get(r, r)

    for k in range(a + 1, b):
        l = body[k]
        mn = l.split()[0]
        if not (mn.startswith("v_") or mn.startswith("ds_read")):
            assert mn.startswith(("s_", "ds_write")), l
            continue
        ops = operands(l)
        dst = reg_set(ops[0])
        if k in tied:
            continue   # in place: the register goes on carrying its variable
        if mn.startswith("v_mfma"):
            clobbered.update(dst)
            for r in dst:
                var[r] = None
        elif re.match(r"v_(mov_b32|mov_b64|accvgpr_read_b32|accvgpr_write_b32|accvgpr_mov_b32)", mn) and len(ops) == 2 and reg_set(ops[1]):
            for d, s in zip(dst, reg_set(ops[1])):
                var[d] = get(s)
        else:
            assert not mn.startswith(("v_swap", "v_permlane", "v_readlane", "v_writelane")), l
            for r in dst:
                var[r] = None
    bad = []
    regs = {f"{c}{i}" for c in "va" for i in range(256)}
    for r in sorted(regs):
        v = get(r)
        if v is not None and (v != r or r in clobbered) and live_after(r, seqs):
            bad.append((r, v, "clobbered by an MFMA" if v == r else "moved"))
    return bad


def test_headline_loop_size(head):
    body = head["body"]
    n_mfma = sum(1 for l in body if l.startswith("v_mfma"))
    n_scratch = sum(1 for l in body if l.startswith("scratch_"))
    print(f"headline iteration loop: {len(body)} instructions (parent {LOOP_PARENT}), {n_mfma} MFMAs, {n_scratch} scratch accesses, ScratchSize {head['scratch']}")
    assert len(body) <= LOOP_PIN
    assert n_mfma >= 261
    assert n_scratch == 0
    assert head["scratch"] <= 8   # the parent's


def sweeps(body):
    """the two long regions (the sweeps); the short third one is the termination check"""
    rg = sorted(regions(body), key=lambda t: t[1] - t[0])
    assert len(rg) == 3 and rg[0][1] - rg[0][0] < 100 and rg[1][1] - rg[1][0] > 10 * (rg[0][1] - rg[0][0]), rg
    return sorted(rg[1:])


def test_headline_loop_exec_writes(any_head):
    """Four from the asm pairs of the two sweeps; two more from the structured `if (active)` around the termination check between them, which
    hipcc owns (s_and_saveexec_b64 / s_or_b64 exec): six in all, against 120 (N = 30) with one region per state update."""
    body = any_head["body"]
    writes = [l for l in body if is_narrow(l) or is_restore(l) or re.match(r"\S+\s+exec\b", l)]
    assert len(writes) <= 6, writes
    assert len(sweeps(body)) == 2


def test_the_sweeps_sit_inside_their_regions(any_head):
    """every MFMA, every LDS access, every packed sum, every projection and every tied state write of the loop lies inside one of the two long regions"""
    body = any_head["body"]
    rg = sweeps(body)
    inside = lambda k: any(a < k < b for a, b in rg)
    for k, l in enumerate(body):
        # (ds_bpermute_b32 is not among them: the residual maxima across the four lanes of an instance, behind the sweep)
        if l.startswith(("v_mfma", "ds_read_b", "ds_write_b", "v_pk_add_f32", "v_med3_f32")) or re.match(r"v_(sub|add)_f32 v\d+,", l):
            assert inside(k), (k, l)


def test_state_keeps_its_home_registers_through_the_regions(any_head):
    body = any_head["body"]
    for a, b in sweeps(body):
        bad = home_violations(body, a, b, any_head["after"])
        assert not bad, (any_head["N"], a, b, bad[:8])


def test_no_mfma_gain_operand_is_written_inside_a_region(any_head):
    """the OPERAND rule: the A operands of the region's MFMAs are loaded once per tile, outside the loop, and only read here"""
    body = any_head["body"]
    for a, b in sweeps(body):
        src_a = {r for l in body[a + 1:b] if l.startswith("v_mfma") for r in reg_set(operands(l)[1])}
        assert len(src_a) == 4, sorted(src_a)   # forward sweep: A1[3], A2; backward sweep: A3[3], A45 (one VGPR each, loaded once per launch)
        for k in range(a + 1, b):
            dst, _ = accesses(body[k])
            assert not (set(dst) & src_a), (any_head["N"], k, body[k])


def test_the_home_check_sees_a_moved_value():
    """self-test on a made-up region: a value that leaves the region in another register, and one whose register an MFMA wrote"""
    body = ["s_and_saveexec_b64 s[0:1], s[2:3]", "v_add_f32_e32 v1, v2, v3", "v_mov_b32_e32 v9, v4", "v_accvgpr_write_b32 a3, v5",
            "v_mfma_f32_16x16x1_4b_f32 v[16:31], v1, v9, v[32:47]", "v_add_f32_e32 v5, v1, v1", "v_accvgpr_read_b32 v5, a3", "s_mov_b64 exec, s[0:1]"]
    after = ["global_store_dword v0, v9, s[4:5]", "global_store_dword v0, v5, s[4:5]", "v_mov_b32_e32 v4, 0", "v_accvgpr_write_b32 a3, v4"]
    assert home_violations(body, 0, len(body) - 1, after) == [("v9", "v4", "moved")]   # v5: parked and brought back (the lanes that are off never
    body[4] = "v_mfma_f32_16x16x1_4b_f32 v[4:19], v1, v1, v[32:47]"                       # left); a3: a stale copy nobody reads
    assert ("v5", "v5", "clobbered by an MFMA") in home_violations(body, 0, len(body) - 1, after)
