"""P2-PAGE-ordered: P2-PAGE (p2_page.py) plus the constraint that a page-out's addresses strictly increase (DESIGN.md §2 ARGUMENTS,
"P2-PAGE-ordered").

Statement: the LIVE updates of the part have strictly increasing addresses, all at or above `lo`; `hi` is one more than the last of
them, or `lo` if there is none; those updates, in that order, take `root_before` to `root_after`.  A chain of parts whose part 0 has
lo = 0 and whose part p + 1 starts at the `hi` (and the root) part p left therefore seals a SET of addresses, each written once, in
order (prover.verify_page_ordered_chain).

The trace is P2-PAGE's: data columns 0 .. 124 and code columns 0 .. 38 have the same meaning and the same constraints (one
constraint text: p2_page.build_page).  What is new:

  data (129 columns)
      125 live   1 on the rows of a real update's path, 0 on a no-op's; constant along a path
      126 lo     the exclusive lower bound of this slot's address: one more than the last live address before it, in this part or an
                 earlier one, 0 if there is none; constant along a path
      127 gbit   bit k - 1 of the gap g = addr - lo on row k = 1 .. 29 of a path's block 0, zero on every other row
      128 gacc   g mod 2^k on those rows, zero on every other row (a no-op's gap counts as 0: gbit = gacc = 0 on its whole path)
  code (42 columns), set for every path slot
      39 gsel    rows k = 1 .. 29 of block 0      40 gpow   2^(k - 1) on those rows      41 gend   row k = 29 of block 0
Globals: out = root_before (8) ‖ root_after (8) ‖ lo ‖ hi, lo and hi field elements as the trace holds them (Montgomery words);
mix = 4 words.

The `order` family (every constraint has degree <= 2 before its selector):
  leaf_in     live (1 - live) = 0;  (1 - live)(w_in - w_out) = 0 (a dead slot changes nothing);  gacc = 0
  carry       live and lo are constant along a path
  gsel        gbit (1 - gbit) = 0;  gacc = gacc[back 1] + gpow gbit
  gend        live (addr - lo - gacc) = 0
  first       lo = out[16]
  path_first  (back 1 is the top row of the slot before)  live (1 - live[back 1]) = 0: live slots come first;
              lo = live[back 1] (addr[back 1] + 1) + (1 - live[back 1]) lo[back 1]
  last_top    out[17] = live (addr + 1) + (1 - live) lo

WHY 29 BITS, AND WHY h <= 26.  P2-PAGE forces addr < 2^(3 + h) through acc and top_out.  With h <= 26: addr < 2^29; lo <= 2^29 by
induction from a checked out[16] (lo is out[16], an earlier address plus one, or an earlier lo); gacc < 2^29 (29 boolean bits).  Then
lo + gacc < 2^30 < P, so the field equation addr = lo + gacc is an integer one and gives addr >= lo; every honest gap fits 29 bits.
MAX_H is therefore 26 (images of up to 2^29 words), one less than P2-PAGE's.

NOT constrained here: that the rows (a_i, in_i, out_i) are the page table of a particular paging segment's seal.  P2-PAGE-tied
(p2_page_tied.py) is this circuit with its live rows on a bus shared with that seal.
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import numpy as np

from . import p2_blocks, p2_page
from .desc import GLOBAL_OUT, GROUP_CODE, GROUP_DATA
from .p2_blocks import GAP_BITS, decode, enc, gated, tree_height  # noqa: F401  (decode: what the chain verifier reads out[16], out[17] with)
from .p2_join import BLOCK_ROWS, R
from .p2_page import D_ADDR, D_W_IN, D_W_OUT, slots

KIND_P2_PAGE_ORDERED = 6
WC, WD, WA, OUT_WORDS = 42, 129, 4, 18
C_GSEL, C_GPOW, C_GEND = 39, 40, 41
D_LIVE, D_LO, D_GBIT, D_GACC = 125, 126, 127, 128
OUT_LO, OUT_HI = 16, 17
MAX_H = 26

# the constraint families, in the order the description emits them: (name, first step, end step) over the ZKC1 step list
FAMILIES: List[Tuple[str, int, int]] = []


def _order(b, chain):
    """the `order` family, after P2-PAGE's `roots` (every tap of P2-PAGE's it names has been emitted there).  P2-TREE's `order` states
    the same gap decomposition over (leaf, id) but emits it in another order: the two are not shared (p2_blocks.py)."""
    code = lambda c, back=0: b.get(GROUP_CODE, c, back)
    dat = lambda c, back=0: b.get(GROUP_DATA, c, back)
    out = lambda i: b.get_global(GLOBAL_OUT, i)
    one, addr, w_in, w_out = b.const(1), dat(D_ADDR), dat(D_W_IN), dat(D_W_OUT)
    live, lo, gbit, gacc = dat(D_LIVE), dat(D_LO), dat(D_GBIT), dat(D_GACC)
    dead = b.sub(one, live)
    chain = gated(b, chain, code(p2_page.C_LEAF_IN), [b.mul(live, dead), b.mul(dead, b.sub(w_in, w_out)), gacc])
    chain = gated(b, chain, code(p2_page.C_CARRY), [b.sub(live, dat(D_LIVE, 1)), b.sub(lo, dat(D_LO, 1))])
    chain = gated(b, chain, code(C_GSEL), [b.mul(gbit, b.sub(one, gbit)), b.sub(gacc, b.add(dat(D_GACC, 1), b.mul(code(C_GPOW), gbit)))])
    chain = gated(b, chain, code(C_GEND), [b.mul(live, b.sub(b.sub(addr, lo), gacc))])
    chain = gated(b, chain, code(1), [b.sub(lo, out(OUT_LO))])
    live_b, dead_b = dat(D_LIVE, 1), b.sub(one, dat(D_LIVE, 1))
    chain = gated(b, chain, code(p2_page.C_PATH_FIRST),
                  [b.mul(live, dead_b), b.sub(lo, b.add(b.mul(live_b, b.add(dat(D_ADDR, 1), one)), b.mul(dead_b, dat(D_LO, 1))))])
    chain = gated(b, chain, code(p2_page.C_LAST_TOP), [b.sub(out(OUT_HI), b.add(b.mul(live, b.add(addr, one)), b.mul(dead, lo)))])
    return chain


@functools.lru_cache(maxsize=None)
def build_p2_page_ordered() -> np.ndarray:
    blob, FAMILIES[:] = p2_page.build_page(KIND_P2_PAGE_ORDERED, (WA, WC, WD), OUT_WORDS, after_roots=("order", _order))
    return blob


def p2_page_ordered_circuit() -> np.ndarray:
    return build_p2_page_ordered().copy()


def family_of(step: int) -> str:
    """the constraint family (P2-PAGE's, with `order` after `roots`) of a step of the description"""
    build_p2_page_ordered()
    return p2_blocks.family_of(FAMILIES, step)


# ------------------------------------------------------------------------------------------------ host twins
def reference_ordered_code(po2: int, zk_cycles: int, h: int) -> np.ndarray:
    """The code group zkh_page_ordered_code writes, (42, 2^po2) Montgomery words: P2-PAGE's 39 columns, then gsel, gpow, gend."""
    if not 1 <= h <= MAX_H:
        raise ValueError(f"h {h} (1 .. {MAX_H}: the gap between two addresses is decomposed into {GAP_BITS} bits)")
    n = 1 << po2
    code = np.zeros((WC, n), dtype=np.uint32)
    code[:p2_page.WC] = p2_page.reference_page_code(po2, zk_cycles, h)
    path = BLOCK_ROWS * h
    for s in range(slots(po2, zk_cycles, h)):
        r0 = path * s
        code[C_GSEL, r0 + 1:r0 + 1 + GAP_BITS] = R
        code[C_GPOW, r0 + 1:r0 + 1 + GAP_BITS] = [enc(1 << k) for k in range(GAP_BITS)]
        code[C_GEND, r0 + GAP_BITS] = R
    return code


def order_columns(po2: int, zk_cycles: int, h: int, addrs: Sequence[int], first: int) -> Tuple[np.ndarray, int, int]:
    """-> (the four new columns on the active rows, (4, A) Montgomery words; lo; hi) of the part at `first` of a table with the
    addresses `addrs` (all of them: lo looks back past the part).  lo and hi are plain integers."""
    A = (1 << po2) - zk_cycles
    N = slots(po2, zk_cycles, h)
    D = len(addrs)
    cols = np.zeros((4, A), dtype=np.uint32)
    path = BLOCK_ROWS * h
    out_lo = hi = 0
    for s in range(N):
        row = first + s
        live = row < D
        before = row if live else D                    # the table's rows before this slot: the last of them bounds it from below
        lo = int(addrs[before - 1]) + 1 if before else 0
        a = int(addrs[row]) if live else 0
        g = a - lo if live else 0
        if not 0 <= g < 1 << GAP_BITS:
            raise ValueError(f"row {row}: address {a} does not follow {lo - 1} by a gap of {GAP_BITS} bits")
        r0 = path * s
        cols[0, r0:r0 + path] = R * live
        cols[1, r0:r0 + path] = enc(lo)
        cols[2, r0 + 1:r0 + 1 + GAP_BITS], cols[3, r0 + 1:r0 + 1 + GAP_BITS] = p2_blocks.gap_columns(g)
        if s == 0:
            out_lo = lo
        hi = a + 1 if live else lo
    return cols, out_lo, hi


def reference_ordered_part(po2: int, zk_cycles: int, W: int, table: Sequence[Tuple[int, int, int]], image_before, first: int = 0):
    """-> (data, out) of the part of `table` that starts at update `first`: the active rows of the data trace, (129, A) Montgomery
    words, and out = root_before ‖ root_after ‖ lo ‖ hi (18 words).  Columns 0 .. 124 are p2_page.reference_page_part's; the four
    new ones are plain numpy over the table (order_columns).  The yardstick of zkh_page_ordered_witgen."""
    h = tree_height(W)
    if h > MAX_H:
        raise ValueError(f"an image of {W} words has h {h} (1 .. {MAX_H})")
    page, root_before, root_after = p2_page.reference_page_part(po2, zk_cycles, W, table, image_before, first)
    cols, lo, hi = order_columns(po2, zk_cycles, h, [int(row[0]) for row in table], first)
    data = np.concatenate([page, cols])
    out = np.concatenate([root_before, root_after, [enc(lo), enc(hi)]]).astype(np.uint32)
    return data, out


if __name__ == "__main__":      # python -m zeth_amd.circuits.p2_page_ordered out.desc   (blob for non-Python hosts)
    import sys
    blob = p2_page_ordered_circuit()
    np.asarray(blob, dtype="<u4").tofile(sys.argv[1])
    print(f"{sys.argv[1]}: {blob.size} words")
