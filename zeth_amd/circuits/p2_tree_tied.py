"""P2-TREE-tied: P2-TREE (p2_tree.py) whose touched words are tied to a paging segment's page table (DESIGN.md §2 ARGUMENTS, "THE TIE").

Statement: P2-TREE's (a set of pairs of leaves with increasing ids in [lo, hi) is replaced, and the replacement takes `root_before` to
`root_after`), AND the sum over the TOUCHED words of the part's pair blocks of -1 / (alpha - (2 + beta a + beta^2 in + beta^3 out)) is F,
with alpha, beta and F words of `out`, exactly as in P2-PAGE-tied (p2_page_tied.py).  A group verifier (prover.verify_tied_tree) checks
the chain of parts as P2-TREE's is checked, that every part states base = 16 * 2^(h-1) for the h it is told, that every seal of the
group states the one challenge the group's data roots give, and that F of the segment's seal and the F of the parts add up to zero.  The
touched words of all pair blocks are then the segment's page table as a multiset; a pair block's id fixes its addresses and ids strictly
increase along the chain, so no address appears twice and the words are the table's rows.  A page-out of 662 267 addresses over 2^20
words is 4 such seals where P2-PAGE-tied takes 334.

The trace is P2-TREE's with 32 more data columns.  The code group (41 columns) is P2-TREE's, so zkh_page_tree_code serves both kinds and
the control root still does not depend on the image's size.  Data columns 0 .. 105 have P2-TREE's meaning and P2-TREE's constraints
(one constraint text: p2_tree.build_tree).  New, read only on the input row of a block:

  106 .. 121  ch[j], j < 16   word j of this pair of leaves is a row of the table: TOUCHED, not "changed" (a row with in = out is a row)
  122 .. 137  wa[j], j < 16   that word's address

  data 138 columns; accum 48 columns = 12 Fp4 columns; out 31 words:
  out = P2-TREE's 18 ‖ base (word 18) ‖ alpha (19 .. 22) ‖ beta (23 .. 26) ‖ F (27 .. 30).  base = Montgomery(2^(h+3)), 16 times the id of
  the first pair of leaves: the circuit does not know h, the group verifier is told it and checks the word (`out_base`), as it checks lo
  of part 0.  For h <= 27 every address and base are below 2^30 < P, so the field equation below names one integer.
Globals: mix = 8 words, which no constraint reads.

The family `words` (between `root` and `bus`), gated by in_row, every constraint of degree <= 3 before its selector, for j < 16:
  ch[j] (1 - ch[j]) = 0
  ch[j] (1 - leaf) = 0                                   only a pair block has words
  leaf (1 - ch[j]) (S_old[j] - S_new[j]) = 0             a word that is no row of the table keeps its value
  ch[j] (wa[j] - (16 id - out[18] + j)) = 0              a touched word's address is the one its block's id gives it
(an inner block's halves are constrained by P2-TREE's dl / dr rule; its ch are zero, so it puts nothing on the open bus), and, gated by
out_row - last_top (the output row of every slot but the last; leaf, up, dl, dr are constant along a block):
  leaf (1 - up) = 0      dl (1 - up) = 0      dr (1 - up) = 0          NO BLOCK THAT MATTERS IS CUT OFF

WHY THE LAST THREE.  P2-TREE only makes `up` boolean, and p2_tree.py says what follows: a block with up = 0 that is not the root slot is
cut off from the tree, nothing reads it.  There that is harmless: such a block proves nothing.  Here a cut-off pair block would still put
its touched words on the OPEN bus: rows whose `in` is not the image's word under root_before and whose `out` never reaches root_after,
with a digest bus that balances because nothing is on it.  The same holds one level up: a pair block that produces, consumed by an inner
block (or a second block of id 1) that is itself cut off, while the root slot is a no-op.  So every block outside the root slot that is a
pair block or consumes a child must produce.  Then the digests of a pair block with a touched word are consumed by a block of id >> 1
that is the root slot or produces in turn, and the ascent can only end in the root slot (p2_tree.py "WHY THE BUS FORCES A TREE": a
producer of id 1 has no consumer): the touched words are words of the tree under root_before, replaced in the tree under root_after.
An honest block other than the root has up = 1 whenever it is live, so no witness changes.

THE BUS is open (logup.py "THE OPEN BUS"; ZKA1 version 8 as it stands) over 12 Fp4 accum columns:
  columns 0 .. 5    P2-TREE's 18 digest terms, unchanged but for their tags: 1 .. 6 would collide with TIE_TAG = 2, so they are 11 .. 16
  columns 6 .. 11   the 16 open terms, three per column (the last column holds one): sign -1, selector in_row, multiplicity ch[j],
                    tuple (wa[j], S_old[j], S_new[j]), tag TIE_TAG.  The column degree is 5, as the digest columns'.

THE CLOSING STEP IS SPLIT (logup.py "THE SPLIT CLOSURE"; `LogupBuilder(..., split_close=True)`).  An open builder without the option closes
on sum over ALL columns S_c = F.  A digest tuple that is produced and never consumed would then only move this part's F, and the group
check sum F = 0 would force the digest tuples to balance across the whole group, not inside a part: a child produced in one part could be
consumed in another, and p2_tree.py's "WHY THE BUS FORCES A TREE" would no longer hold per part.  Under the option the description states
two equations on `last`: sum over the closed columns 0 .. 5 S_c = 0, and sum over the open columns 6 .. 11 S_c = out[27 .. 31).  The
challenge is the hash of every data root of the group (prover.seal_tied_tree draws it after all of them are fixed), so each seal's digest
bus balances inside that seal with the usual probability, P2-TREE's argument holds part by part (with the three constraints above: for
every block that states a word), and F is the open terms alone.  No
column mixes open and closed terms: the builder refuses one.  The blob needs nothing new: `check_open` allows several terms of the open
tag, zkh_accumulate_open fills all 12 columns, and zkh_check_bus skips the open tag's keys.

NOT constrained here: nothing about the segment; the group verifier holds the other half.
Not a shipped circuit: it is loaded the way P2-TREE is, and its control root is zkh_code_root of its code group.
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import numpy as np

from . import p2_blocks, p2_tree
from .desc import GLOBAL_OUT, GROUP_CODE, GROUP_DATA
from .logup import TIE_TAG, Arguments, LogupBuilder, reference_accumulate, _enc
from .p2_blocks import enc, gated, tree_height
from .p2_join import BLOCK_ROWS
from .p2_tree import C_IN_ROW, C_LAST_TOP, C_OUT_ROW, D_DL, D_DR, D_ID, D_LEAF, D_SN, D_SO, D_UP, MAX_H, MIN_H, MIX_WORDS, WC, block_slots, decode  # noqa: F401  (the shape is P2-TREE's; callers size and decode with these)

KIND_P2_TREE_TIED = 9
WD, WA, OUT_WORDS = 138, 48, 31
D_CH, D_WA = 106, 122
PAIR_WORDS = 16
PREFIX_WORDS = p2_tree.OUT_WORDS                # what the witness generator returns: root_before ‖ root_after ‖ lo ‖ hi
OUT_BASE, OUT_ALPHA, OUT_BETA, OUT_TOTAL = 18, 19, 23, 27
DIGEST_TAG = 11                                 # the digest terms' tags are 11 .. 16: clear of TIE_TAG
DIGEST_COLS = 6                                 # accum Fp4 columns 0 .. 5 are closed, 6 .. 11 open

# the constraint families, in the order the description emits them: (name, first step, end step) over the ZKC1 step list
FAMILIES: List[Tuple[str, int, int]] = []


def out_base(h: int) -> int:
    """out[18] of every part over a tree of height h: the Montgomery word of 2^(h+3) = 16 * 2^(h-1), sixteen times the id of the first pair
    of leaves, so that 16 id - base + j is the address of word j of the pair block id"""
    if not MIN_H <= h <= MAX_H:
        raise ValueError(f"h {h} ({MIN_H} .. {MAX_H})")
    return enc(1 << (h + 3))


def _words(b, chain):
    """the `words` family"""
    dat = lambda c: b.get(GROUP_DATA, c)
    one, sixteen = b.const(1), b.const(16)
    leaf = dat(D_LEAF)
    first_word = b.sub(b.mul(sixteen, dat(D_ID)), b.get_global(GLOBAL_OUT, OUT_BASE))
    cons = []
    for j in range(PAIR_WORDS):
        ch, wa = dat(D_CH + j), dat(D_WA + j)
        cons += [b.mul(ch, b.sub(one, ch)), b.mul(ch, b.sub(one, leaf)),
                 b.mul(b.mul(leaf, b.sub(one, ch)), b.sub(dat(D_SO + j), dat(D_SN + j))),
                 b.mul(ch, b.sub(wa, b.add(first_word, b.const(j)) if j else first_word))]
    chain = gated(b, chain, b.get(GROUP_CODE, C_IN_ROW), cons)
    # no block outside the root slot that is a pair block or consumes a child is cut off from the tree
    off = b.sub(one, dat(D_UP))
    return gated(b, chain, b.sub(b.get(GROUP_CODE, C_OUT_ROW), b.get(GROUP_CODE, C_LAST_TOP)), [b.mul(dat(c), off) for c in (D_LEAF, D_DL, D_DR)])


def open_terms() -> List[dict]:
    """the 16 open terms as LogupBuilder.term keywords: word j of a pair block, on accum column 6 + j // 3"""
    return [dict(col=DIGEST_COLS + j // 3, tuple_cols=[(GROUP_DATA, D_WA + j), (GROUP_DATA, D_SO + j), (GROUP_DATA, D_SN + j)], sign=-1, sel=C_IN_ROW,
                 mult=(GROUP_DATA, D_CH + j), tag=TIE_TAG) for j in range(PAIR_WORDS)]


@functools.lru_cache(maxsize=None)
def build_p2_tree_tied(split_close: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ZKC1 description, ZKA1 argument blob).  split_close=False: the description whose one closing step is sum over all columns
    S_c = F, which is NOT sound per part (the module docstring): it exists for the test that shows what the option closes."""
    b = LogupBuilder((WA, WC, WD), (OUT_WORDS, MIX_WORDS), alpha=OUT_ALPHA, beta=OUT_BETA, kind=KIND_P2_TREE_TIED, open_bus=(TIE_TAG, OUT_TOTAL),
                     split_close=split_close)
    blobs, families = p2_tree.build_tree(b, after_root=("words", _words), terms=p2_tree.bus_terms(DIGEST_TAG) + open_terms())
    if split_close:
        FAMILIES[:] = families
    return blobs


def p2_tree_tied_circuit() -> np.ndarray:
    return build_p2_tree_tied()[0].copy()


def arguments() -> np.ndarray:
    """the ZKA1 blob of the bus: what SegmentProver(hal, p2_tree_tied_circuit(), arguments=arguments()) hands zkh_accumulate_open"""
    return build_p2_tree_tied()[1].copy()


def family_of(step: int) -> str:
    """the constraint family (rounds, in_row, carry, order, root, words, bus, sanity) of a step of the description"""
    build_p2_tree_tied()
    return p2_blocks.family_of(FAMILIES, step)


# ------------------------------------------------------------------------------------------------ host twins
def reference_word_columns(po2: int, zk_cycles: int, W: int, tree_data: np.ndarray, addrs: Sequence[int]) -> np.ndarray:
    """ch ‖ wa, (32, A) Montgomery words, over the active rows of a P2-TREE data trace `tree_data` of an image of W words whose part
    touches the addresses `addrs`: on the input row of a pair block wa[j] = 16 (id - 2^(h-1)) + j and ch[j] = that address is touched;
    zeros on every other row and in every other block"""
    h, B = tree_height(W), block_slots(po2, zk_cycles)
    half, touched = 1 << (h - 1), {int(a) for a in addrs}
    cols = np.zeros((2 * PAIR_WORDS, tree_data.shape[1]), dtype=np.uint32)
    for slot in range(B):
        r0 = BLOCK_ROWS * slot
        ident = decode(tree_data[D_ID, r0])
        if ident < half:
            continue
        for j in range(PAIR_WORDS):
            a = PAIR_WORDS * (ident - half) + j
            cols[j, r0] = p2_blocks.R * (a in touched)
            cols[PAIR_WORDS + j, r0] = enc(a)
    return cols


def reference_tree_tied_part(po2: int, zk_cycles: int, W: int, table: Sequence[Tuple[int, int, int]], image_before, first: int, count: int, challenge):
    """-> (data, accum, out) of the part [first, first + count) of `table` under the challenge alpha ‖ beta (8 Montgomery words): the active
    rows of the data trace, (138, A) Montgomery words (p2_tree.reference_tree_part's 106 columns and the 32 of `reference_word_columns`);
    the accum trace zkh_accumulate_open must produce over the full 2^po2 rows with zero blinding rows, (48, 2^po2); out = root_before ‖
    root_after ‖ lo ‖ hi ‖ base ‖ alpha ‖ beta ‖ F (31 words)."""
    n = 1 << po2
    A = n - zk_cycles
    tree_data, prefix = p2_tree.reference_tree_part(po2, zk_cycles, W, table, image_before, first, count)
    addrs = [int(row[0]) for row in table[first:first + count]]
    data = np.concatenate([tree_data, reference_word_columns(po2, zk_cycles, W, tree_data, addrs)])
    full = np.zeros((WD, n), dtype=np.uint32)
    full[:, :A] = data
    challenge = np.asarray(challenge, dtype=np.uint32).reshape(8)
    accum, total = reference_accumulate(Arguments.parse(arguments()), po2, zk_cycles, p2_tree.reference_tree_code(po2, zk_cycles), full, challenge)
    out = np.concatenate([prefix, [out_base(tree_height(W))], challenge, _enc(np.asarray(total, dtype=np.uint64)).astype(np.uint32)]).astype(np.uint32)
    return data, accum.reshape(WA, n), out


if __name__ == "__main__":      # python -m zeth_amd.circuits.p2_tree_tied out.desc out.args   (blobs for non-Python hosts)
    import sys
    desc, args = build_p2_tree_tied()
    np.asarray(desc, dtype="<u4").tofile(sys.argv[1])
    print(f"{sys.argv[1]}: {desc.size} words")
    if len(sys.argv) > 2:
        np.asarray(args, dtype="<u4").tofile(sys.argv[2])
        print(f"{sys.argv[2]}: {args.size} words")
