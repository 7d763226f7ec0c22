#!/usr/bin/env python3
"""Instruction histogram of k_hash_rows' steady-state absorb block (one Poseidon2 permutation per lane), by opcode class and
modelled issue cycles, against the multiply floor — the evidence behind "Poseidon2 is at its instruction floor".

    python tools/isa_histogram.py > profiles/r03_hash_rows_isa_histogram.txt
    python tools/isa_histogram.py --csrc <another checkout>/zeth_amd/csrc      (the same count for another tree's hash.hip)
    python tools/isa_histogram.py --kernel fold                                 (k_hash_fold: one permutation, no block loop)
    python tools/isa_histogram.py --grouped                                     (the instantiation with the grouped partial rounds)
    python tools/isa_histogram.py --loads                                       (both kernels: registers and the table loads only)

Compiles zeth_amd/csrc/hash.hip for gfx950 with the build's flags (`-S`, device only), takes the first copy of the block
loop of k_hash_rows (interior blocks of the sponge: 16 absorbed columns, one permutation), finds its inner loops from the
backward branches and weights them by their trip counts (4 full rounds, 7 groups of three partial rounds, 4 full rounds, or
3 where the last full round is peeled out of its loop and follows it as straight-line code).  Where the partial rounds run as
matrix products (poseidon2_linear.h) there are two inner loops, the full rounds', and the section between them is straight-line
code that runs once per permutation; v_mfma_* instructions are counted apart from the VALU (another pipe) with their passes,
and the half-wave swaps (v_permlane32_swap) are modelled at 4.0 cycles like the other two-register instructions.
Code that a steady-state block does not run is weighted by what it is (path_weights): inside a loop of N trips the special
cases of one trip (first / last partial group) count once per permutation; at block level the tail block's predicated loads
and the alternative that the last block of a sponge takes count zero.
Issue cycles per wave64 instruction from tools/ubench_valu.hip (profiles/r01_ubench_valu.txt): 32-bit multiplies,
v_mad_*64*, fp64 and v_cvt_f64 4.0; plain add / sub / logic / shift / mov 2.5 (measured 2.46); v_min / v_add3 / v_lshl_add 4.0;
compare-select pairs 2.1 + 2.1.
Table loads (table_loads): every scalar, global, flat or LDS load of the permutation that reads a constant table, by kind, and for each
the number of VALU + MFMA instructions issued between the load and the s_waitcnt that covers it.  A wait that directly follows its
load (distance 0) exposes a whole cache round trip to the in-order wave.
"""
from __future__ import annotations

import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64", "v_add_f64", "v_fma_f64", "v_mul_f64", "v_cvt_f64", "v_min_u32", "v_max",
        "v_add3", "v_lshl_add", "v_lshl_or", "v_and_or", "v_permlane32_swap")
MFMA_PASSES = {"v_mfma_i32_32x32x32_i8": 16}     # 4 cycles per pass on the matrix pipe
TRIPS = {"full": 4, "partial": 7}
CLASSES = [
    ("s-box + reduction multiplies (v_mad_i64_i32, v_mad_u64_u32)", ("v_mad_i64", "v_mad_u64")),
    ("low-word multiplies (v_mul_lo_u32: the Montgomery m)", ("v_mul_lo", "v_mul_hi")),
    ("M_ext on doubles (v_add_f64, v_fma_f64)", ("v_add_f64", "v_fma_f64", "v_mul_f64")),
    ("int -> double (v_cvt_f64_*)", ("v_cvt_f64",)),
    ("round-constant / plain adds, subs (v_add_u32, v_sub_u32, v_add_co ...)", ("v_add_u32", "v_sub_u32", "v_subrev_u32", "v_add_co", "v_addc", "v_sub_co", "v_subrev_co", "v_subb")),
    ("select / min (modular corrections, canonicalisation)", ("v_cndmask", "v_min_u32", "v_max")),
    ("64-bit shift-adds (v_lshl_add_u64: unreduced sum folds)", ("v_lshl_add", "v_lshlrev_b64", "v_lshrrev_b64", "v_ashrrev_i64")),
    ("half-wave swaps (v_permlane32_swap: B operands, accumulator gather)", ("v_permlane32_swap",)),
    ("moves, logic, shifts (v_mov, v_and, v_or, v_xor, v_ashrrev, v_lshl ...)", ("v_mov", "v_and", "v_or", "v_xor", "v_ashrrev", "v_lshlrev", "v_lshrrev", "v_bfe", "v_perm", "v_readlane", "v_writelane", "v_readfirstlane", "v_accvgpr")),
]


def cycles(op: str) -> float:
    return 4.0 if op.startswith(FOUR) else 2.5


def valu_count(body, a, b):
    return sum(1 for i in range(a, b) if body[i].startswith("\tv_") and not body[i].startswith("\tv_mfma"))


def path_weights(body, labels, outer, merged, trips):
    """weight[i] of every line of the block loop on a steady-state block.  Conditional code is found from the scalar branches:
    (a) a forward conditional branch skips region A = (branch, target); if A ends in a forward jump, the lines from the target
        to that jump's target are the alternative B (if / else);
    (b) the lines between a backward conditional branch and a following backward `s_branch` to the same label run only when
        the loop does not repeat (the compiler's place for what only the last trip does); if the two labels differ, the lines
        between the labels and the lines after the branch are alternatives, as in (a).
    Inside a loop of N trips: (b) and a lone A run once per permutation; of A and B the longer is the special case (once) and
    the shorter the common one (N - 1).  At block level: (b) and an A with branches of its own (the tail block's per-column
    loads) are not steady state (0); a plain A is."""
    def resolve(lbl):                                   # through trampolines: a label followed only by a jump
        for _ in range(4):
            i = labels.get(lbl)
            if i is None:
                return None
            j = i + 1
            while j < len(body) and (not body[j].strip() or body[j].strip().startswith(";")):
                j += 1
            m = re.match(r"\s+s_branch\s+(\.LBB\d+_\d+)", body[j]) if j < len(body) else None
            if not m:
                return i
            lbl = m.group(1)
        return labels.get(lbl)
    def loop_of(i):
        for k, (a, b) in enumerate(merged):
            if a <= i <= b:
                return k
        return None
    weight = [1.0] * len(body)
    for k, (a, b) in enumerate(merged):
        for i in range(a, b + 1):
            weight[i] = trips[k]
    br = re.compile(r"\s+(s_cbranch_(?:scc|vcc)\S*|s_cbranch_exec\S*|s_branch)\s+(\.LBB\d+_\d+)")
    i = outer[0]
    while i <= outer[1]:
        m = br.match(body[i])
        if not m or not m.group(1).startswith(("s_cbranch_scc", "s_cbranch_vcc")):
            i += 1
            continue
        k = loop_of(i)
        n = trips[k] if k is not None else None
        raw = labels.get(m.group(2))
        if raw is not None and raw < i:                 # (b): backward conditional, then code, then a backward jump
            j = i + 1
            while j <= outer[1] and not br.match(body[j]) and not re.match(r"^\.LBB", body[j]):
                j += 1
            m2 = br.match(body[j]) if j <= outer[1] else None
            raw2 = labels.get(m2.group(2), 1 << 30) if m2 and m2.group(1) == "s_branch" else 1 << 30
            if raw2 == raw and valu_count(body, i + 1, j):
                for x in range(i + 1, j):
                    weight[x] = 1.0 if n else 0.0
            elif raw < raw2 < i and n:                  # two alternatives: [raw, raw2) or the lines after the branch
                long_a = valu_count(body, raw, raw2) >= valu_count(body, i + 1, j)
                for x in range(raw, raw2):
                    weight[x] = 1.0 if long_a else n - 1.0
                for x in range(i + 1, j):
                    weight[x] = n - 1.0 if long_a else 1.0
            i += 1
            continue
        t = resolve(m.group(2))
        if t is None or t <= i or t > outer[1] or (k is not None and t > merged[k][1]) or (k is None and loop_of(t - 1) is not None):
            i += 1
            continue
        a_lo, a_hi = i + 1, t                           # region A = [a_lo, a_hi)
        last = next((x for x in range(a_hi - 1, a_lo - 1, -1) if body[x].startswith("\t") and not body[x].strip().startswith(";")), None)
        m3 = br.match(body[last]) if last is not None else None
        b_hi = None
        if m3 and m3.group(1) in ("s_branch", "s_cbranch_execnz", "s_cbranch_execz"):
            t2 = resolve(m3.group(2))
            if t2 is not None and t2 > a_hi and t2 <= (merged[k][1] if k is not None else outer[1]):
                b_hi = t2
        nested = any(br.match(body[x]) for x in range(a_lo, (last if m3 else a_hi)))
        if n:
            if b_hi is not None:
                long_a = valu_count(body, a_lo, a_hi) >= valu_count(body, a_hi, b_hi)
                for x in range(a_lo, a_hi):
                    weight[x] = 1.0 if long_a else n - 1.0
                for x in range(a_hi, b_hi):
                    weight[x] = n - 1.0 if long_a else 1.0
            else:
                for x in range(a_lo, a_hi):
                    weight[x] = 1.0
        elif nested:
            for x in range(a_lo, a_hi):
                weight[x] = 0.0
        i = (b_hi if b_hi is not None else a_hi) if (n or nested) else i + 1
    return weight


def compile_asm(csrc=None):
    """hash.hip of `csrc` (default: this tree's) as gfx950 assembly lines, with the build's flags"""
    sys.path.insert(0, ROOT)
    from zeth_amd import build as B
    csrc = csrc or B.CSRC
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "hash.s")
        cmd = [B.HIPCC, *B.FLAGS, *B.EXTRA_FLAGS.get("hash.hip", []), "-I", B.CSRC, "--cuda-device-only", "-S", os.path.join(csrc, "hash.hip"), "-o", out]
        subprocess.run(cmd, check=True, capture_output=True)
        return open(out).read().split("\n")


VM_OPS = ("global_", "flat_", "scratch_", "buffer_")
LGKM_OPS = ("s_load", "s_buffer_load", "ds_", "flat_")


def load_kind(op):
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar"
    if op.startswith("global_load"):
        return "global"
    if op.startswith("flat_load"):
        return "flat"
    if op.startswith(("ds_read", "ds_load")):
        return "LDS"
    return None


def table_loads(body, lo, hi, loops, first_loop):
    """The table loads among body[lo..hi] as (line, kind, distance): distance = VALU + MFMA instructions between the load and the wait
    that covers it, None if no wait in the region does.  Not table loads: the kernel's arguments (scalar loads off s[0:1] ahead of the
    first wait) and its data, which are the vector loads ahead of the first full-round loop (columns, child digests).
    Counters as the hardware keeps them: vector memory returns in order (vmcnt(N) covers a load once N others were issued behind it);
    scalar loads return out of order (only lgkmcnt(0) covers them); LDS in order unless a scalar load is in flight beside it; a flat
    load needs both.  A load in a loop body may be waited for at the top of the next trip: the shorter of the two ways counts."""
    def opcode(i):
        l = body[i]
        if not l.startswith("\t") or not l.strip() or l.strip().startswith((".", ";")):
            return None
        return l.strip().split()[0]
    def walk(start, kind, path):
        n_vm = n_lgkm = n_smem = dist = 0
        need_vm, need_lgkm = kind in ("global", "flat"), kind in ("scalar", "LDS", "flat")
        for i in path:
            op = opcode(i)
            if op is None:
                continue
            if op == "s_waitcnt":
                vm, lg = re.search(r"vmcnt\((\d+)\)", body[i]), re.search(r"lgkmcnt\((\d+)\)", body[i])
                if need_vm and vm and n_vm >= int(vm.group(1)):
                    need_vm = False
                if need_lgkm and lg and (int(lg.group(1)) == 0 or (kind == "LDS" and not n_smem and n_lgkm >= int(lg.group(1)))):
                    need_lgkm = False
                if not need_vm and not need_lgkm:
                    return dist
                continue
            if op.startswith("v_"):
                dist += 1
            if op.startswith(VM_OPS):
                n_vm += 1
            if op.startswith(LGKM_OPS):
                n_lgkm += 1
                n_smem += op.startswith("s_")
        return None
    found, first_wait = [], next((i for i in range(lo, hi + 1) if opcode(i) == "s_waitcnt"), hi)
    for i in range(lo, hi + 1):
        op = opcode(i)
        kind = load_kind(op) if op else None
        if kind is None:
            continue
        if kind == "scalar" and i < first_wait and re.search(r",\s*s\[0:1\],", body[i]):
            continue                                    # a kernel argument
        if kind in ("global", "flat") and i < first_loop:
            continue                                    # the kernel's data
        ways = [walk(i, kind, range(i + 1, hi + 1))]
        for a, b in loops:
            if a <= i <= b:
                ways.append(walk(i, kind, list(range(i + 1, b + 1)) + list(range(a, i))))
        ways = [w for w in ways if w is not None]
        found.append((i, kind, min(ways) if ways else None))
    return found


def resources(lines, start):
    """registers, scratch and occupancy of the kernel whose label is lines[start], from the compiler's own summary behind it"""
    res = {}
    for l in lines[start:]:
        m = re.match(r";\s*(NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", l)
        if m:
            res[m.group(1)] = int(m.group(2))
        if "Occupancy" in res and "ScratchSize" in res and "NumVgprs" in res and "TotalNumSgprs" in res:
            break
    return res


def analyze(lines, kernel="rows", grouped=False):
    """Everything the report prints, as a dict (tests/test_hash_table_loads_static.py reads it)."""
    heads = [i for i, l in enumerate(lines) if re.match(r"^_ZN\S*k_hash_%s(I\S*Ev|E)\S*:" % kernel, l)]
    want = "ILb0E" if grouped else "ILb1E"           # templated on the linear partial rounds where that path exists
    start = next((i for i in heads if want in lines[i]), heads[0])
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start + 1:end]
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    back = []                                           # (target index, branch index) of backward branches = loops
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 1 << 30) < i:
            back.append((labels[m.group(1)], i))
    back.sort()
    # first loop nest = the block loop: from its header to the last branch back to that header (blocks the compiler placed
    # after that latch belong to the tail block's predicated loads and are not part of a steady-state block)
    if kernel == "rows":
        head = max(back, key=lambda b: b[1] - b[0])[0]     # the widest loop nest (a short staging loop may come first)
        outer = (head, max(b[1] for b in back if b[0] == head))
    else:                                               # no block loop: the whole kernel is one permutation
        outer = (0, len(body) - 1)
    inner = [b for b in back if outer[0] < b[0] and b[1] < outer[1]]
    # merge loops that share a region (rotated loops produce two backward branches into the same body)
    merged = []
    for b in inner:
        if merged and b[0] <= merged[-1][1]:
            merged[-1] = (min(merged[-1][0], b[0]), max(merged[-1][1], b[1]))
        else:
            merged.append(b)
    kinds = ["full", "partial", "full"] if len(merged) == 3 else ["full", "full"] if len(merged) == 2 else ["?"] * len(merged)
    trips = [TRIPS.get(kind, 1) for kind in kinds]
    # a peeled last full round: one more round body (hundreds of VALU instructions) between the last loop and the block loop's end
    peeled = len(merged) in (2, 3) and valu_count(body, merged[-1][1] + 1, outer[1] + 1) > 300
    if peeled:
        trips[-1] -= 1
    weight = path_weights(body, labels, outer, merged, trips)
    hist = collections.Counter()
    static = collections.Counter()
    other = collections.Counter()
    mfma = collections.Counter()
    for i in range(outer[0], outer[1] + 1):
        l = body[i]
        if not l.startswith("\t") or not l.strip() or l.strip().startswith((".", ";")):
            continue
        op = l.strip().split()[0]
        if weight[i] == 0:
            continue
        if op.startswith("v_mfma"):
            mfma[op.replace("_e64", "")] += weight[i]
        elif op.startswith("v_"):
            hist[op] += weight[i]
            static[op] += 1
        else:
            other[op.split("_")[0] + "_" + op.split("_")[1] if "_" in op else op] += weight[i]
    total = sum(hist.values())
    tot_cyc = sum(cycles(op) * n for op, n in hist.items())
    loads = table_loads(body, outer[0], outer[1], merged, merged[0][0] if merged else outer[0])
    return dict(name=lines[start].split(":")[0], kernel=kernel, body=body, outer=outer, merged=merged, kinds=kinds, trips=trips, peeled=peeled,
                weight=weight, hist=hist, static=static, other=other, mfma=mfma, total=total, tot_cyc=tot_cyc, loads=loads,
                resources=resources(lines, start))


def loads_summary(d):
    """by kind: (count, [distances]); and the count of loads that no wait in the region covers"""
    kinds = {k: [x[2] for x in d["loads"] if x[1] == k and x[2] is not None] for k in ("scalar", "global", "flat", "LDS")}
    return kinds, sum(1 for x in d["loads"] if x[2] is None)


def print_loads(d):
    kinds, unwaited = loads_summary(d)
    r = d["resources"]
    print(f"# {d['name']}")
    print(f"#   VGPRs {r.get('NumVgprs')}, AGPRs {r.get('NumAgprs')}, SGPRs {r.get('TotalNumSgprs')}, scratch {r.get('ScratchSize')} bytes, occupancy {r.get('Occupancy')} waves per SIMD;"
          f" VALU per wave-permutation {d['total']:.0f}, MFMA {sum(d['mfma'].values()):.0f}")
    print("#   table loads (static), and the VALU + MFMA instructions between each load and the wait that covers it:")
    print(f"#   {'kind':8s} {'loads':>6s} {'min':>6s} {'median':>7s} {'zero':>6s}")
    for k, ds in kinds.items():
        n = sum(1 for x in d["loads"] if x[1] == k)
        sd = sorted(ds)
        print(f"    {k:8s} {n:6d} {(str(sd[0]) if sd else '-'):>6s} {(str(sd[len(sd) // 2]) if sd else '-'):>7s} {sum(1 for x in ds if x == 0):6d}")
    every = sorted(x for ds in kinds.values() for x in ds)
    print(f"    {'all':8s} {len(d['loads']):6d} {(str(every[0]) if every else '-'):>6s} {(str(every[len(every) // 2]) if every else '-'):>7s} {sum(1 for x in every if x == 0):6d}"
          + (f"   ({unwaited} requested and never read in this region)" if unwaited else ""))


def main():
    csrc = sys.argv[sys.argv.index("--csrc") + 1] if "--csrc" in sys.argv else None
    lines = compile_asm(csrc)
    if "--loads" in sys.argv:
        for kernel in ("rows", "fold"):
            print_loads(analyze(lines, kernel, "--grouped" in sys.argv))
        return
    kernel = sys.argv[sys.argv.index("--kernel") + 1] if "--kernel" in sys.argv else "rows"
    d = analyze(lines, kernel, "--grouped" in sys.argv)
    body, outer, merged, kinds, trips, peeled, weight = d["body"], d["outer"], d["merged"], d["kinds"], d["trips"], d["peeled"], d["weight"]
    hist, static, other, mfma, total, tot_cyc, start = d["hist"], d["static"], d["other"], d["mfma"], d["total"], d["tot_cyc"], 0
    lines = [d["name"] + ":"]
    print(f"# {lines[start].rstrip(':')}")
    print("# k_hash_%s, %s = ONE Poseidon2 permutation per lane (gfx950, hipcc -O3 -enable-misched=0)" %
          (kernel, "steady-state absorb block" if kernel == "rows" else "the whole kernel"))
    print(f"# block loop at asm lines {outer[0]}..{outer[1]} of the kernel; inner loops " +
          ", ".join(f"{k} x{n} [{a}..{b}]" for (a, b), k, n in zip(merged, kinds, trips)) + (" + the last full round peeled" if peeled else ""))
    print(f"# dynamic VALU instructions per wave-permutation (static count x trip counts): {total:.0f}"
          f"   (hardware: SQ_INSTS_VALU / (leaves x blocks / 64) = 6.44 k, profiles/r02_sq_counters.txt)")
    print(f"# modelled issue cycles per wave-permutation: {tot_cyc:.0f}  (1024 SIMDs: {tot_cyc / 1024:.1f} SIMD-cycles per 64 permutations)")
    if mfma:
        print("# matrix pipe (not VALU): " + ", ".join(f"{n:.0f} x {op} = {n * MFMA_PASSES.get(op, 16) * 4:.0f} cycles" for op, n in mfma.items()) +
              f"; straight-line VALU between the loops: {valu_count(body, merged[0][1] + 1, merged[1][0]) if len(merged) == 2 else 0}")
    print("#")
    print(f"# {'class':82s} {'instr':>7s} {'share':>6s} {'cycles':>8s} {'share':>6s}")
    seen = set()
    for name, prefixes in CLASSES:
        ops = [op for op in hist if op.startswith(prefixes)]
        seen.update(ops)
        n = sum(hist[o] for o in ops)
        cy = sum(cycles(o) * hist[o] for o in ops)
        print(f"  {name:82s} {n:7.0f} {100 * n / total:5.1f}% {cy:8.0f} {100 * cy / tot_cyc:5.1f}%")
    rest = [op for op in hist if op not in seen]
    n = sum(hist[o] for o in rest)
    cy = sum(cycles(o) * hist[o] for o in rest)
    print(f"  {'other VALU (' + ', '.join(sorted(rest)[:6]) + ')':82s} {n:7.0f} {100 * n / total:5.1f}% {cy:8.0f} {100 * cy / tot_cyc:5.1f}%")
    print("#")
    print("# per opcode (dynamic):")
    for op, n in hist.most_common():
        print(f"  {op:28s} {n:7.0f}  x {cycles(op):.1f} cycles")
    print("# non-VALU in the same block (dynamic): " + ", ".join(f"{k} {v:.0f}" for k, v in other.most_common(8)))
    # the floor
    prods = (8 * 24 + 21) * 4 + 21 * 24                        # s-box products (x^7 = 4 products) + one diagonal product per cell per partial round
    reds = 8 * 24                                              # one Montgomery reduction per cell after each full round's M_ext
    floor = 3 * prods + 2 * reds
    print("#")
    print(f"# FLOOR: {8 * 24 + 21} s-boxes x 4 products = {(8 * 24 + 21) * 4}, plus one diagonal product per cell per partial round ({21 * 24}):")
    print(f"#   {prods} Montgomery products x 3 instructions (multiply-add, low multiply, multiply-add) = {3 * prods}, plus the {reds} reductions")
    print(f"#   that bring every full round's M_ext output back to a word (low multiply + multiply-add) = {2 * reds}:  {floor} instructions, {4 * floor} issue cycles.")
    mult = sum(hist[o] for o in hist if o.startswith(("v_mad_i64", "v_mad_u64", "v_mul_lo", "v_mul_hi")))
    print(f"#   This build spends {mult:.0f} instructions in those opcodes ({100 * mult / total:.0f} % of all VALU) = {mult / floor:.2f} x that floor.")
    print(f"#   Everything that is not a multiply — M_ext on doubles ({sum(hist[o] for o in hist if 'f64' in o and 'cvt' not in o):.0f}), int->double conversions "
          f"({sum(hist[o] for o in hist if 'cvt' in o):.0f}), round-constant adds, the corrections at the partial-round borders —")
    print(f"#   is {total - mult:.0f} instructions ({100 * (total - mult) / total:.0f} %).  The whole block is {total / floor:.2f} x the multiply floor; in issue cycles "
          f"{tot_cyc / (4 * floor):.2f} x.")
    print("# What is left to take: the per-block scale fixes / canonicalisation at the loop borders (the segments outside the three")
    out_loops = sum(n for op, n in static.items()) - 0
    print("#   inner loops) are ~%d instructions per block (%.1f %%); v_cvt_f64 (3.3 %%) has no cheaper form; nothing else is not a multiply or an M_ext add." %
          (sum(1 for i in range(outer[0], outer[1] + 1) if weight[i] == 1.0 and body[i].startswith("\tv_")), 100.0 * sum(1 for i in range(outer[0], outer[1] + 1) if weight[i] == 1.0 and body[i].startswith("\tv_")) / total))
    print("#")
    print_loads(d)


if __name__ == "__main__":
    main()
