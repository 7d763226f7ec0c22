#!/usr/bin/env python3
"""Static VALU mix of the lazy forward NTT kernels (no GPU: hipcc -S cross-compiles gfx950) — what profiles/r10_ntt_lazy_pairs_static.txt
is made from.

    python tools/ntt_static.py [--expand-bits 2] [--kernels all | PATTERN ...] [--source FILE] [--brief]

Compiles zeth_amd/csrc/ntt.hip with the build's flags (device only) and prints, for k_ntt_high<10 | 8, false, true> and
k_ntt_low12<false, true>: VALU instructions per lane by opcode, modelled issue cycles (4.0 for the half-rate class, 2.5 for add / shift /
move, as tools/isa_histogram.py), VGPRs, SGPRs, scratch.  The kernels are straight-line code, one lane = 16 elements; k_ntt_low12 takes
expand_bits as an argument and so holds the paths of every value: --expand-bits N counts a copy with that argument fixed, i.e. what a lane
executes.  --kernels takes substrings of mangled names instead of those three, or `all` for every k_ntt_* / k_zk_shift instantiation;
--source compiles another copy of ntt.hip (an earlier commit's, for a side-by-side listing); --brief prints the summary lines only.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR = ("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64", "v_min_u32", "v_max", "v_add3", "v_lshl_add", "v_lshl_or", "v_and_or")
KERNELS = ("k_ntt_highILi10ELb0ELb1E", "k_ntt_highILi8ELb0ELb1E", "k_ntt_low12ILb0ELb1E")
LOW12_CALL = "radix_layers<4, false, true, 1, LAZY>(v, ltab, 0, (int)p.expand_bits);"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--expand-bits", type=int, default=None)
    ap.add_argument("--kernels", nargs="+", default=list(KERNELS))
    ap.add_argument("--source", default=None)
    ap.add_argument("--brief", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from zeth_amd import build as B
    with tempfile.TemporaryDirectory() as tmp:
        src = args.source or os.path.join(B.CSRC, "ntt.hip")
        if args.expand_bits is not None:
            text = open(src).read()
            assert LOW12_CALL in text, "k_ntt_low12's first round has changed: update LOW12_CALL"
            src = os.path.join(tmp, "ntt_fixed.hip")
            open(src, "w").write(text.replace(LOW12_CALL, LOW12_CALL.replace("(int)p.expand_bits", str(args.expand_bits))))
        out = os.path.join(tmp, "ntt.s")
        subprocess.run([B.HIPCC, *B.FLAGS, "-I", B.CSRC, "--cuda-device-only", "-S", src, "-o", out], check=True, capture_output=True)
        asm = open(out).read()
    pats = args.kernels
    if pats == ["all"]:
        pats = sorted(set(re.findall(r"^_Z\S*?(k_(?:ntt_\w+?|zk_shift)(?:I\w+?E)?)(?:v|N12_)\S*:", asm, re.M)))
    for pat in pats:
        m = re.search(rf"^(_Z\S*{pat}\S*):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.S | re.M)
        name, body = m.group(1), m.group(2)
        c = collections.Counter()
        for ln in body.split("\n"):
            t = ln.strip().split()
            if not t or t[0].startswith((";", ".", "/")) or t[0].endswith(":"):
                continue
            op = t[0]
            if op.startswith("v_"):
                c[re.sub(r"_e(32|64)$", "", op)] += 1
            elif op.startswith(("global_", "ds_", "s_load", "s_nop", "s_waitcnt", "scratch_")):
                c["~" + "_".join(op.split("_")[:2])] += 1
        valu = sum(n for o, n in c.items() if o.startswith("v_"))
        cyc = sum((4.0 if o.startswith(FOUR) else 2.5) * n for o, n in c.items() if o.startswith("v_"))
        meta = asm[asm.index(".amdhsa_kernel " + name):]
        vg, sg, scr, lds = (re.search(rf"\.amdhsa_{k} (\d+)", meta).group(1)
                            for k in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size"))
        print(f"## {pat}: VALU {valu}  modelled issue cycles {cyc:.0f}  vgprs {vg}  sgprs {sg}  scratch {scr}  lds {lds}")
        for o, n in [] if args.brief else sorted(c.items(), key=lambda kv: -kv[1]):
            print(f"   {o:28s} {n}")


if __name__ == "__main__":
    main()
