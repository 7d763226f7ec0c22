"""P2-PAGE: a page-out of the committed memory image proven from root to root (DESIGN.md §2 ARGUMENTS, "P2-PAGE").

Statement: starting from `root_before`, apply D single-word updates one after the other; update i opens word a_i as in_i under the
current root and replaces it with out_i, which gives the next root; the last root is `root_after`.  The tree is the one of
include/zkhal.h "THE IMAGE'S COMMITMENT": leaves are eight words verbatim, a node is `hash_pair` of its children, h = log2 L.  Words
are residues, as Montgomery words in the trace: the space the tree lives in.

NOT constrained here: that the addresses strictly increase (P2-PAGE-ordered, p2_page_ordered.py, is this circuit plus that), and that
the rows (a_i, in_i, out_i) are the page table of a particular paging segment's seal (P2-PAGE-tied, p2_page_tied.py, is P2-PAGE-ordered
plus that).  This circuit proves "D single-word updates take
root_before to root_after" and nothing else.

Trace (A = n - zk_cycles active rows, blocks of 31 rows with P2-JOIN's row roles k = 0 .. 30, K = A // 31 blocks).  A PATH is h
consecutive blocks, so there are N = K // h path slots; h >= 1 is a parameter of the code group as (po2, zk_cycles) are.  Block 0 of a
path hashes the pair of leaves that holds the word (16 words), block t >= 1 the on-path digest with its sibling.  Every row holds TWO
permutations side by side, the old path and the new one: they share their siblings, and a block's on-path input is the output row of
the block before it (back 1), so every constraint is local and no wiring argument is needed.  Slots D .. N - 1 are no-op updates of
address 0 (in = out = the word held there): real paths that satisfy every constraint.  Active rows past 31 h N are zero.

  data (125 columns): S_old[24] Q_old[24] S_new[24] Q_new[24] (each pair is P2-JOIN's S, Q)
      96..111 e[16]   one-hot of a & 15, on a path's first row (zero elsewhere)
      112 b           the path bit (a >> (3 + t)) & 1, on the input row of a block t >= 1 (zero elsewhere)
      113 addr  114 w_in  115 w_out   constant along a path
      116 acc         the address rebuilt so far: a mod 2^(4 + t) on the rows of block t
      117..124 cur[8] the root this path must open, constant along a path
  code (39 columns, a function of (po2, zk_cycles, h)): 0 active 1 first 2 body (accum argument)  3 lin 4 fullr 5 partr 6 lf 7 lp
      (P2-JOIN's round selectors)  8 leaf_in (input row of a path's block 0)  9 node_in (input row of a block t >= 1)
      10 path_first (leaf_in of a slot other than 0)  11 top_out (output row of a path's last block)  12 last_top (top_out of slot
      N - 1)  13 carry (every row inside a path but its first)  14 pow (2^(3 + t) on node_in rows)  15..38 the round constants
  accum: P2-JOIN's argument verbatim, one Fp4 running product of (mix + data column 0) (data column 0 is S_old[0]).
Globals: out = root_before (8) ‖ root_after (8);  mix = 4 words.
The address is rebuilt in the field, so 2^(3 + h) must stay below P: h <= MAX_H = 27 (images of at most 2^30 words).

A table of D > N rows is sealed as a chain of PARTS (`parts`, `reference_page_part`; DESIGN.md "PARTS"): the same circuit on the run of
updates [first, first + min(N, D - first)), out = the root before update `first` ‖ the root after the run's last update.
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import numpy as np

from . import p2_blocks
from .desc import (GLOBAL_OUT, GROUP_CODE, GROUP_DATA, OP_ADD, OP_AND_EQZ, OP_CONST, OP_CONST_EXT, OP_GET, OP_GET_GLOBAL, OP_MUL, OP_SUB, OP_TRUE, P, Circuit,
                   CircuitBuilder)
from .p2_blocks import enc, gated, tree_height  # noqa: F401  (tree_height: what callers of this module size an image with)
from .p2_join import BLOCK_ROWS, R, RINV, T, block_rows, hash_pair_words

KIND_P2_PAGE = 5
WC, WD, WA, OUT_WORDS = 39, 125, 4, 16
C_LIN, C_FULLR, C_PARTR, C_LF, C_LP, C_LEAF_IN, C_NODE_IN, C_PATH_FIRST, C_TOP_OUT, C_LAST_TOP, C_CARRY, C_POW, C_RC = range(3, 16)
ROUND_COLS = (C_LIN, C_FULLR, C_PARTR, C_LF, C_LP, C_RC)
D_SO, D_QO, D_SN, D_QN, D_E, D_B, D_ADDR, D_W_IN, D_W_OUT, D_ACC, D_CUR = 0, 24, 48, 72, 96, 112, 113, 114, 115, 116, 117
MAX_H = 27

# the constraint families, in the order build_p2_page emits them: (name, first step, end step) over the ZKC1 step list
FAMILIES: List[Tuple[str, int, int]] = []


def slots(po2: int, zk_cycles: int, h: int) -> int:
    """N: the path slots of a trace of 2^po2 rows"""
    return (((1 << po2) - zk_cycles) // BLOCK_ROWS) // h


def build_page(kind: int, sizes: Tuple[int, int, int], out_words: int, after_roots=None, builder=None, accum=None):
    """-> (blob, families): P2-PAGE's constraint text over a circuit of `sizes` (accum, code, data) columns and `out_words` outputs.
    after_roots = (name, emit): emit(b, chain) -> chain emits one more family, `name`, between `roots` and `accum`
    (p2_page_ordered.py); without it this is P2-PAGE word for word.  builder: the CircuitBuilder to emit into, one of these sizes
    that the caller made (p2_page_tied.py: a LogupBuilder, which also holds the argument's terms); accum(b, chain, first, body) ->
    chain emits the `accum` family in place of the running product."""
    b = CircuitBuilder(sizes, (out_words, WA), kind=kind) if builder is None else builder
    code = lambda c, back=0: b.get(GROUP_CODE, c, back)
    dat = lambda c, back=0: b.get(GROUP_DATA, c, back)
    out = lambda i: b.get_global(GLOBAL_OUT, i)
    one = b.const(1)
    active, first, body = code(0), code(1), code(2)
    cst = {v: b.const(v) for v in (2, 3, 4, 5, 6, 7)}
    families, family = p2_blocks.family_log(b)

    def times(c, x):
        return x if c == 1 else b.mul(cst[c], x)

    def total(xs):
        e = xs[0]
        for x in xs[1:]:
            e = b.add(e, x)
        return e

    chain = b.true()
    leaf_in, node_in = code(C_LEAF_IN), code(C_NODE_IN)
    # 1. rounds: P2-JOIN's constraints on both permutations; the capacity cells are zero on every input row
    start = len(b.steps)
    chain = p2_blocks.emit_rounds(b, chain, code, dat, cst, ((D_SO, D_QO), (D_SN, D_QN)), ROUND_COLS, lambda: b.add(leaf_in, node_in))
    family("rounds", start)

    So = lambda j, back=0: dat(D_SO + j, back)
    Sn = lambda j, back=0: dat(D_SN + j, back)
    e = [dat(D_E + j) for j in range(16)]
    bit, addr, w_in, w_out, acc = dat(D_B), dat(D_ADDR), dat(D_W_IN), dat(D_W_OUT), dat(D_ACC)
    cur = [dat(D_CUR + j) for j in range(8)]
    # 2. leaf_in: the word a & 15 of the pair of leaves is w_in on the old side, w_out on the new one; every other word is shared
    start = len(b.steps)
    chain = gated(b, chain, leaf_in,
                  [b.mul(e[j], b.sub(one, e[j])) for j in range(16)] + [b.sub(total(e), one)]
                  + [b.mul(b.sub(one, e[j]), b.sub(So(j), Sn(j))) for j in range(16)]
                  + [b.sub(total([b.mul(e[j], So(j)) for j in range(16)]), w_in), b.sub(total([b.mul(e[j], Sn(j)) for j in range(16)]), w_out),
                     b.sub(acc, total([times(j, e[j]) if j < 8 else b.mul(b.const(j), e[j]) for j in range(1, 16)]))])
    family("leaf_in", start)
    # 3. node_in: the output of the block below enters on the side the bit names, the other side is one sibling for old and new
    start = len(b.steps)
    nb = b.sub(one, bit)
    cons = [b.mul(bit, nb)]
    for X in (So, Sn):
        cons += [b.add(b.mul(nb, b.sub(X(j), X(j, 1))), b.mul(bit, b.sub(X(8 + j), X(j, 1)))) for j in range(8)]
    cons += [b.add(b.mul(nb, b.sub(So(8 + j), Sn(8 + j))), b.mul(bit, b.sub(So(j), Sn(j)))) for j in range(8)]
    cons += [b.sub(acc, b.add(dat(D_ACC, 1), b.mul(code(C_POW), bit)))]
    chain = gated(b, chain, node_in, cons)
    family("node_in", start)
    # 4. carry: what is constant along a path; acc moves on node_in rows only
    start = len(b.steps)
    chain = gated(b, chain, code(C_CARRY), [b.sub(dat(c), dat(c, 1)) for c in [D_ADDR, D_W_IN, D_W_OUT] + [D_CUR + j for j in range(8)]])
    chain = gated(b, chain, b.sub(code(C_CARRY), node_in), [b.sub(acc, dat(D_ACC, 1))])
    family("carry", start)
    # 5. top_out: the old path ends on the root in hand, at the address it claims
    start = len(b.steps)
    chain = gated(b, chain, code(C_TOP_OUT), [b.sub(So(j), cur[j]) for j in range(8)] + [b.sub(acc, addr)])
    family("top_out", start)
    # 6. roots: the first path opens root_before, every later one the new root of the path before it, the last leaves root_after
    start = len(b.steps)
    chain = gated(b, chain, first, [b.sub(cur[j], out(j)) for j in range(8)])
    chain = gated(b, chain, code(C_PATH_FIRST), [b.sub(cur[j], Sn(j, 1)) for j in range(8)])
    chain = gated(b, chain, code(C_LAST_TOP), [b.sub(Sn(j), out(8 + j)) for j in range(8)])
    family("roots", start)
    if after_roots is not None:
        start = len(b.steps)
        chain = after_roots[1](b, chain)
        family(after_roots[0], start)
    # 7. accum: one Fp4 running product of (mix + data column 0), and the selector sanity, as in P2-JOIN
    start = len(b.steps)
    chain = p2_blocks.running_product(b, chain, first, body, So(0)) if accum is None else accum(b, chain, first, body)
    family("accum", start)
    start = len(b.steps)
    chain = p2_blocks.sanity(b, chain, active, first, body)
    family("sanity", start)
    return b.finish(chain), families


@functools.lru_cache(maxsize=None)
def build_p2_page() -> np.ndarray:
    blob, FAMILIES[:] = build_page(KIND_P2_PAGE, (WA, WC, WD), OUT_WORDS)
    return blob


def p2_page_circuit() -> np.ndarray:
    return build_p2_page().copy()


def family_of(step: int) -> str:
    """the constraint family (rounds, leaf_in, node_in, carry, top_out, roots, accum, sanity) of a step of the description"""
    build_p2_page()
    return p2_blocks.family_of(FAMILIES, step)


def constraint_degrees(desc) -> List[int]:
    """The builder's degree check: the degree, in the trace cells, of the value of every and_eqz step of a description, BEFORE the
    selectors that gate it (a tap has degree 1, a constant or a global 0, a sum the larger degree, a product the sum)."""
    c = desc if isinstance(desc, Circuit) else Circuit.parse(desc)
    deg, out = [], []
    for op, a, b2, _, _ in c.steps:
        if op in (OP_CONST, OP_CONST_EXT, OP_GET_GLOBAL):
            deg.append(0)
        elif op == OP_GET:
            deg.append(1)
        elif op in (OP_ADD, OP_SUB):
            deg.append(max(deg[a], deg[b2]))
        elif op == OP_MUL:
            deg.append(deg[a] + deg[b2])
        elif op == OP_AND_EQZ:
            out.append(deg[b2])
        elif op < OP_TRUE:
            raise ValueError(f"unknown value step {op}")
    return out


# ------------------------------------------------------------------------------------------------ host twins
def reference_page_code(po2: int, zk_cycles: int, h: int) -> np.ndarray:
    """The code group zkh_page_circuit_code writes, (39, 2^po2) Montgomery words: a function of (po2, zk_cycles, h)."""
    if not 1 <= h <= MAX_H:
        raise ValueError(f"h {h} (1 .. {MAX_H})")
    N = slots(po2, zk_cycles, h)
    code = p2_blocks.reference_round_code(WC, po2, zk_cycles, h * N, ROUND_COLS)
    for r in range(BLOCK_ROWS * h * N):
        k, blk = r % BLOCK_ROWS, r // BLOCK_ROWS
        t, s = blk % h, blk // h
        if k == 0 and t == 0:
            code[C_LEAF_IN, r] = R
            if s:
                code[C_PATH_FIRST, r] = R
        if k == 0 and t:
            code[C_NODE_IN, r] = R
            code[C_POW, r] = enc(1 << (3 + t))
        if k == BLOCK_ROWS - 1 and t == h - 1:
            code[C_TOP_OUT, r] = R
            if s == N - 1:
                code[C_LAST_TOP, r] = R
        if k or t:
            code[C_CARRY, r] = R
    return code


def reference_page_trace(po2: int, zk_cycles: int, W: int, table: Sequence[Tuple[int, int, int]], image_before):
    """-> (data, root_before, root_after): the active rows of the data trace, (125, A) Montgomery words, of the page-out `table` (rows
    (a, in, out): an address and two residues as Montgomery words, addresses strictly increasing and below W) over `image_before` (W
    raw Montgomery words), and both roots.  The updates are applied ONE AT A TIME to a plain Python tree, hashing through
    hash_pair_words: the yardstick of the device generator's two-tree shortcut, which it therefore does not use."""
    image = [int(w) % P for w in np.asarray(image_before, dtype=np.uint32).reshape(-1)]
    if len(image) != W or W <= 8:
        raise ValueError(f"an image of {len(image)} words for W = {W} (W > 8)")
    h = tree_height(W)
    L = 1 << h
    n = 1 << po2
    A = n - zk_cycles
    N = slots(po2, zk_cycles, h)
    D = len(table)
    if D > N:
        raise ValueError(f"D {D} updates, but h {h} at po2 {po2} leaves N {N} path slots")
    nodes = [[0] * 8 for _ in range(2 * L)]
    for a, w in enumerate(image):
        nodes[L + (a >> 3)][a & 7] = w
    for i in range(L - 1, 0, -1):
        nodes[i] = hash_pair_words(nodes[2 * i], nodes[2 * i + 1])
    root_before = list(nodes[1])
    data = np.zeros((WD, A), dtype=np.uint32)
    canon = lambda ws: [w * RINV % P for w in ws]
    before = -1
    for s in range(N):
        if s < D:
            a, w_in, w_out = (int(x) for x in table[s])
            if not before < a < W:
                raise ValueError(f"row {s}: address {a} does not follow {before} below {W}")
            before = a
            if nodes[L + (a >> 3)][a & 7] != w_in:
                raise ValueError(f"row {s}: in {w_in} at address {a}, but the tree holds {nodes[L + (a >> 3)][a & 7]}")
        else:
            a = 0
            w_in = w_out = nodes[L][0]
        cur = list(nodes[1])
        r0 = BLOCK_ROWS * h * s
        pair = a >> 4
        old = nodes[L + 2 * pair] + nodes[L + 2 * pair + 1]
        new = list(old)
        new[a & 15] = w_out
        for t in range(h):
            if t:
                x = a >> (3 + t)                       # the on-path node of layer t, the layer of L >> t nodes
                sib = nodes[(L >> t) + (x ^ 1)]
                old, new = (sib + d_old, sib + d_new) if x & 1 else (d_old + sib, d_new + sib)
            ro, rn = block_rows(canon(old) + [0] * 8), block_rows(canon(new) + [0] * 8)
            for k in range(BLOCK_ROWS):
                r = r0 + BLOCK_ROWS * t + k
                for base, v in ((D_SO, ro[k][0]), (D_QO, ro[k][1]), (D_SN, rn[k][0]), (D_QN, rn[k][1])):
                    data[base:base + T, r] = [x * R % P for x in v]
                data[D_ACC, r] = enc(a % (1 << (4 + t)))
            if t == 0:
                data[D_E + (a & 15), r0] = R
            else:
                data[D_B, r0 + BLOCK_ROWS * t] = R * ((a >> (3 + t)) & 1)
            d_old, d_new = ([x * R % P for x in rows[-1][0][:8]] for rows in (ro, rn))
        rows = slice(r0, r0 + BLOCK_ROWS * h)
        data[D_ADDR, rows], data[D_W_IN, rows], data[D_W_OUT, rows] = enc(a), w_in, w_out
        for j in range(8):
            data[D_CUR + j, rows] = cur[j]
        # the plain tree takes the update on its own: the leaf's word, then hash_pair up the path
        nodes[L + (a >> 3)][a & 7] = w_out
        i = (L + (a >> 3)) >> 1
        while i:
            nodes[i] = hash_pair_words(nodes[2 * i], nodes[2 * i + 1])
            i >>= 1
        if d_old != cur or d_new != nodes[1]:
            raise AssertionError(f"slot {s}: the paths' top digests are not the tree's roots")
    return data, np.asarray(root_before, dtype=np.uint32), np.asarray(nodes[1], dtype=np.uint32)


def parts(po2: int, zk_cycles: int, W: int, D: int) -> List[Tuple[int, int]]:
    """The plan of a page-out of D rows over an image of W words as a chain of P2-PAGE traces: [(first, count), ...], part p the updates
    [first, first + count) with count = min(N, D - first), so only the last part has no-op slots.  D = 0 is the one part (0, 0)."""
    N = slots(po2, zk_cycles, tree_height(W)) if W > 8 else 0
    if N < 1:
        raise ValueError(f"no path slot for an image of {W} words at po2 {po2} with {zk_cycles} zk_cycles")
    return [(first, min(N, D - first)) for first in range(0, D, N)] or [(0, 0)]


def reference_page_part(po2: int, zk_cycles: int, W: int, table: Sequence[Tuple[int, int, int]], image_before, first: int):
    """-> (data, root_before, root_after) of the part of `table` that starts at update `first`, as reference_page_trace gives them: the
    updates [0, first) are applied to a copy of the image in plain numpy, and the rows [first, first + N) are then a whole table over
    that image.  No tree code of its own: the yardstick of zkh_page_circuit_witgen_part, which reads both trees of the WHOLE page-out."""
    D = len(table)
    if not (0 <= first < D or first == D == 0):
        raise ValueError(f"first {first}, but the table has {D} rows")
    image = np.array(image_before, dtype=np.uint32).reshape(-1)
    for a, _, w_out in table[:first]:
        image[int(a)] = int(w_out)
    N = slots(po2, zk_cycles, tree_height(W))
    return reference_page_trace(po2, zk_cycles, W, table[first:first + N], image)


if __name__ == "__main__":      # python -m zeth_amd.circuits.p2_page out.desc   (blob for non-Python hosts)
    import sys
    blob = p2_page_circuit()
    np.asarray(blob, dtype="<u4").tofile(sys.argv[1])
    print(f"{sys.argv[1]}: {blob.size} words")
