"""P2-TREE: a page-out of the committed memory image sealed by its DIRTY NODES, not by one path per word (DESIGN.md §2 ARGUMENTS,
"P2-TREE").

Statement: a set of pairs of leaves (a pair is 16 words), given in strictly increasing order, is replaced; the replacement takes
`root_before` to `root_after`.  out = root_before ‖ root_after ‖ lo ‖ hi (18 words): lo and hi bound the heap ids of the part's pair
blocks as P2-PAGE-ordered's bound addresses, hi one more than the last pair block's id, or lo if there is none.  A chain of parts
whose part 0 has lo = 2^(h-1), whose part p + 1 opens the root and starts at the hi part p left, and whose last hi is at most 2^h
(prover.verify_page_tree_chain) seals a page-out of any size.  The tree is the one of include/zkhal.h "THE IMAGE'S COMMITMENT".

Trace.  A = n - zk_cycles active rows, B = A // 31 block slots of P2-JOIN's 31 rows (an input row, 29 round rows, an output row);
every row holds the old and the new permutation side by side, as in P2-PAGE.  A block computes ONE node of the tree and its id is that
node's heap index (csrc/image_tree.h): the root block has id 1, a pair block (its inputs are two leaves, 16 memory words) an id in
[L/2, L) with L = 2^h leaves, and the children of block id are 2 id and 2 id + 1.  h = 2 .. 27 (W > 16).  The code group does not
depend on h: there is one control root per (po2, zk_cycles) for every image size, and the chain verifier is told h.

  data (106 columns): S_old[24] Q_old[24] S_new[24] Q_new[24] at P2-PAGE's offsets
      96 id   97 idl = 2 id   98 idr = 2 id + 1
      99 leaf  (a pair block)   100 up (the block's digests go on the bus: every live block but the root)
      101 dl  102 dr  (the left / right child is a block of this trace: its digests come off the bus)
      103 lo   the exclusive lower bound of a pair block's id: one more than the pair block before it, in this part or an earlier one,
               2^(h-1) if there is none; behind the pair blocks: one more than the last of them (= hi)
      104 gbit  105 gacc   bit k - 1 of g = id - lo on row k = 1 .. 29 of a pair block, and g mod 2^k; gacc stays g on row 30
  code (41 columns, a function of (po2, zk_cycles)): 0 active 1 first 2 body  3 lin 4 fullr 5 partr 6 lf 7 lp (the round selectors)
      8 in_row 9 out_row  10 block_first (in_row of a slot other than 0)  11 carry (rows 1 .. 30 of a block)  12 last_top (out_row of
      slot B - 1)  13 gsel (rows 1 .. 29)  14 gpow (2^(k-1) on them)  15 gend (row 29)  16 .. 39 the round constants  40 last (row A - 1)
  accum (24 columns = 6 Fp4 columns): the bus below, through logup.LogupBuilder; zkh_accumulate fills it from the ZKA1 blob.
Globals: out 18 words; mix 8 words, alpha at offset 0 and beta at offset 4.

Slot order: the pair blocks first, in increasing id; then the other live blocks: for every pair block in order, the nodes it STARTS
(those above it that are not above the pair block before it), bottom up, the root excepted; then dead blocks (16 zeros hashed on both
sides, every flag zero, id 0, so idr = 1; lo carried); the root block is always slot B - 1.  Rows past 31 B are zero.

Constraint families (`FAMILIES`, `family_of`; every one of degree <= 3 before its selector, backs 0 and 1):
  rounds  P2-PAGE's (p2_blocks.emit_rounds) on both permutations; the capacity cells are zero on in_row
  in_row  leaf, up, dl, dr boolean; idl = 2 id, idr = 2 id + 1; leaf dl = leaf dr = 0; (1 - leaf)(1 - dl)(S_old[j] - S_new[j]) = 0 for
          j < 8 and the same with dr for j in 8 .. 15: a clean child is ONE sibling serving both sides
  carry   id, idl, idr, leaf, up, dl, dr, lo are constant along a block; gacc too, except on gsel rows; gbit = 0 on the output row
  order   in_row: gbit = gacc = 0;  gsel: gbit boolean, gacc = gacc[back 1] + gpow gbit;  gend: leaf (id - lo - gacc) = 0;
          block_first: leaf (1 - leaf[back 1]) = 0 (pair blocks come first), lo = leaf[back 1] (id[back 1] + 1) + (1 - leaf[back 1])
          lo[back 1];  first: lo = out[16];  last_top: out[17] = leaf (id + 1) + (1 - leaf) lo
  root    last_top: id = 1, up = 0, S_old[0..8) = out[0..8), S_new[0..8) = out[8..16)
  bus     18 terms.  The 16 words X = old[0..8) ‖ new[0..8) of a digest pair travel as six tuples (key, X[3k], X[3k+1], X[3k+2]), tags
          1 .. 6, the last of width 2.  Producer: sign -1, selector out_row, multiplicity up, key id, the words S_old[0..8), S_new[0..8)
          of the output row.  Left consumer: +1, in_row, dl, key idl, S_old[0..8), S_new[0..8) of the input row.  Right consumer: +1,
          in_row, dr, key idr, S_old[8..16), S_new[8..16).  The three terms of a tag share one accum column.  No records: nothing is
          derived.
  sanity  P2-PAGE's (p2_blocks.sanity)

WHY THE BUS FORCES A TREE.  Every produced tuple must be consumed by a block whose id is the producer's id >> 1, on the matching side
(the key is idl or idr of the consumer).  The only block that produces nothing is the root slot (up = 0 there, and id = 1).  A second
producer of one id would force a second consumer of id >> 1, and so on up: the chain ends at a second block of id 1 that is not the
root slot, so it produces, and its tuple has no consumer, because consumers read keys of at least 2.  So ids are unique and parents
are forced by the keys.  Depth is forced too: leaf = 1 blocks are range-checked into [lo, hi), which the chain verifier checks to lie
inside [2^(h-1), 2^h), so a pair block sits h - 1 levels below the root, and leaf = 0 blocks that consume nothing have old = new on
both halves: they are no-ops.  (A block with up = 0 that is not the root slot is cut off from the tree: nothing reads it.)

NOT constrained here: which words of a pair were touched, and that the updates are the page table of a particular paging segment's seal.
P2-TREE-tied (p2_tree_tied.py, kind 9) is this circuit plus both: this constraint text (`build_tree`) with the family `words` over 32 more
data columns, and the touched words of its pair blocks on the bus across seals that p2_page_tied.py put P2-PAGE-ordered's rows on.
Not a shipped circuit: it is loaded the way SYN-LOOKUP is, and its control root is zkh_code_root of its code group.
"""
from __future__ import annotations

import functools
from typing import List, Sequence, Tuple

import numpy as np

from . import p2_blocks
from .desc import GLOBAL_OUT, GROUP_CODE, GROUP_DATA, P
from .logup import LogupBuilder
from .p2_blocks import GAP_BITS, decode, enc, gated, tree_height  # noqa: F401  (decode: what the chain verifier reads out[16], out[17] with)
from .p2_join import BLOCK_ROWS, R, RINV, T, block_rows

KIND_P2_TREE = 7
WC, WD, WA, OUT_WORDS, MIX_WORDS = 41, 106, 24, 18, 8
(C_LIN, C_FULLR, C_PARTR, C_LF, C_LP, C_IN_ROW, C_OUT_ROW, C_BLOCK_FIRST, C_CARRY, C_LAST_TOP, C_GSEL, C_GPOW, C_GEND, C_RC) = range(3, 17)
C_LAST = 40
ROUND_COLS = (C_LIN, C_FULLR, C_PARTR, C_LF, C_LP, C_RC)
D_SO, D_QO, D_SN, D_QN = 0, 24, 48, 72
D_ID, D_IDL, D_IDR, D_LEAF, D_UP, D_DL, D_DR, D_LO, D_GBIT, D_GACC = range(96, 106)
OUT_LO, OUT_HI = 16, 17
MIN_H, MAX_H = 2, 27

# the constraint families, in the order the description emits them: (name, first step, end step) over the ZKC1 step list
FAMILIES: List[Tuple[str, int, int]] = []


def block_slots(po2: int, zk_cycles: int) -> int:
    """B: the block slots of a trace of 2^po2 rows"""
    return ((1 << po2) - zk_cycles) // BLOCK_ROWS


@functools.lru_cache(maxsize=None)
def build_p2_tree() -> Tuple[np.ndarray, np.ndarray]:
    """-> (ZKC1 description, ZKA1 argument blob)"""
    b = LogupBuilder((WA, WC, WD), (OUT_WORDS, MIX_WORDS), alpha=0, beta=4, kind=KIND_P2_TREE)
    blobs, FAMILIES[:] = build_tree(b)
    return blobs


def build_tree(b, after_root=None, terms=None):
    """-> ((ZKC1 description, ZKA1 argument blob), families): P2-TREE's constraint text emitted into the LogupBuilder `b`, whose data
    columns 0 .. 105 and code columns are P2-TREE's.  after_root = (name, emit): emit(b, chain) -> chain emits one more family, `name`,
    between `root` and `bus`; terms: the bus's terms as LogupBuilder.term keywords in place of `bus_terms()` (p2_tree_tied.py gives
    both); without them this is P2-TREE word for word."""
    code = lambda c, back=0: b.get(GROUP_CODE, c, back)
    dat = lambda c, back=0: b.get(GROUP_DATA, c, back)
    out = lambda i: b.get_global(GLOBAL_OUT, i)
    one = b.const(1)
    active, first, body = code(0), code(1), code(2)
    cst = {v: b.const(v) for v in (2, 3, 4, 5, 6, 7)}
    families, family = p2_blocks.family_log(b)

    chain = b.true()
    in_row = code(C_IN_ROW)
    start = len(b.steps)
    chain = p2_blocks.emit_rounds(b, chain, code, dat, cst, ((D_SO, D_QO), (D_SN, D_QN)), ROUND_COLS, lambda: in_row)
    family("rounds", start)

    So = lambda j, back=0: dat(D_SO + j, back)
    Sn = lambda j, back=0: dat(D_SN + j, back)
    ident, idl, idr, leaf, up, dl, dr, lo, gbit, gacc = (dat(c) for c in range(D_ID, D_GACC + 1))
    inner_node = b.sub(one, leaf)
    start = len(b.steps)
    cons = [b.mul(x, b.sub(one, x)) for x in (leaf, up, dl, dr)]
    cons += [b.sub(idl, b.mul(cst[2], ident)), b.sub(idr, b.add(b.mul(cst[2], ident), one)), b.mul(leaf, dl), b.mul(leaf, dr)]
    for side, lo_j in ((dl, 0), (dr, 8)):
        clean = b.mul(inner_node, b.sub(one, side))
        cons += [b.mul(clean, b.sub(So(lo_j + j), Sn(lo_j + j))) for j in range(8)]
    chain = gated(b, chain, in_row, cons)
    family("in_row", start)

    start = len(b.steps)
    chain = gated(b, chain, code(C_CARRY), [b.sub(dat(c), dat(c, 1)) for c in range(D_ID, D_LO + 1)])
    chain = gated(b, chain, b.sub(code(C_CARRY), code(C_GSEL)), [b.sub(gacc, dat(D_GACC, 1)), gbit])
    family("carry", start)

    start = len(b.steps)
    chain = gated(b, chain, in_row, [gbit, gacc])
    chain = gated(b, chain, code(C_GSEL), [b.mul(gbit, b.sub(one, gbit)), b.sub(gacc, b.add(dat(D_GACC, 1), b.mul(code(C_GPOW), gbit)))])
    chain = gated(b, chain, code(C_GEND), [b.mul(leaf, b.sub(b.sub(ident, lo), gacc))])
    leaf_b, inner_b = dat(D_LEAF, 1), b.sub(one, dat(D_LEAF, 1))
    chain = gated(b, chain, code(C_BLOCK_FIRST),
                  [b.mul(leaf, inner_b), b.sub(lo, b.add(b.mul(leaf_b, b.add(dat(D_ID, 1), one)), b.mul(inner_b, dat(D_LO, 1))))])
    chain = gated(b, chain, first, [b.sub(lo, out(OUT_LO))])
    chain = gated(b, chain, code(C_LAST_TOP), [b.sub(out(OUT_HI), b.add(b.mul(leaf, b.add(ident, one)), b.mul(inner_node, lo)))])
    family("order", start)

    start = len(b.steps)
    chain = gated(b, chain, code(C_LAST_TOP), [b.sub(ident, one), up] + [b.sub(So(j), out(j)) for j in range(8)] + [b.sub(Sn(j), out(8 + j)) for j in range(8)])
    family("root", start)

    if after_root is not None:
        start = len(b.steps)
        chain = after_root[1](b, chain)
        family(after_root[0], start)

    # the bus: three terms per tag, one accum column per tag
    for term in (bus_terms() if terms is None else terms):
        b.term(**term)
    start = len(b.steps)
    chain = b.arguments(chain, first, body, code(C_LAST))
    family("bus", start)

    start = len(b.steps)
    chain = p2_blocks.sanity(b, chain, active, first, body)
    family("sanity", start)
    return b.finish_all(chain), families


def bus_terms(first_tag: int = 1) -> List[dict]:
    """the 18 terms as LogupBuilder.term keywords: per tag first_tag .. first_tag + 5 (P2-TREE: 1 .. 6) the producer, the left
    consumer, the right consumer"""
    words = lambda lo_j: [D_SO + lo_j + j for j in range(8)] + [D_SN + lo_j + j for j in range(8)]      # X = old ‖ new of one digest pair
    terms = []
    for k in range(6):
        cut = slice(3 * k, min(3 * k + 3, 16))
        for sign, sel, mult, key, xs in ((-1, C_OUT_ROW, D_UP, D_ID, words(0)), (1, C_IN_ROW, D_DL, D_IDL, words(0)), (1, C_IN_ROW, D_DR, D_IDR, words(8))):
            terms.append(dict(col=k, tuple_cols=[(GROUP_DATA, key)] + [(GROUP_DATA, c) for c in xs[cut]], sign=sign, sel=sel,
                              mult=(GROUP_DATA, mult), tag=first_tag + k))
    return terms


def p2_tree_circuit() -> np.ndarray:
    return build_p2_tree()[0].copy()


def arguments() -> np.ndarray:
    """the ZKA1 blob of the bus: what SegmentProver(hal, p2_tree_circuit(), arguments=arguments()) hands zkh_accumulate"""
    return build_p2_tree()[1].copy()


def family_of(step: int) -> str:
    """the constraint family (rounds, in_row, carry, order, root, bus, sanity) of a step of the description"""
    build_p2_tree()
    return p2_blocks.family_of(FAMILIES, step)


# ------------------------------------------------------------------------------------------------ host twins
def reference_tree_code(po2: int, zk_cycles: int) -> np.ndarray:
    """The code group zkh_page_tree_code writes, (41, 2^po2) Montgomery words: a function of (po2, zk_cycles) alone."""
    B = block_slots(po2, zk_cycles)
    code = p2_blocks.reference_round_code(WC, po2, zk_cycles, B, ROUND_COLS)
    code[C_LAST, (1 << po2) - zk_cycles - 1] = R
    rows = lambda k: slice(k, BLOCK_ROWS * B, BLOCK_ROWS)
    code[C_IN_ROW, rows(0)] = R
    code[C_BLOCK_FIRST, BLOCK_ROWS::BLOCK_ROWS][:max(B - 1, 0)] = R
    code[C_OUT_ROW, rows(BLOCK_ROWS - 1)] = R
    for k in range(1, BLOCK_ROWS):
        code[C_CARRY, rows(k)] = R
    for k in range(1, GAP_BITS + 1):
        code[C_GSEL, rows(k)] = R
        code[C_GPOW, rows(k)] = enc(1 << (k - 1))
    code[C_GEND, rows(GAP_BITS)] = R
    if B:
        code[C_LAST_TOP, BLOCK_ROWS * B - 1] = R
    return code


def pair_cost(h: int, q: int, before) -> int:
    """the nodes the pair of leaves q starts in a part whose pair before it is `before` (None: it is the part's first, all h of its path)"""
    return h if before is None else (q ^ before).bit_length()


def slot_ids(h: int, B: int, pairs: Sequence[int]) -> List[int]:
    """the ids of the B block slots of a part that replaces the pairs of leaves `pairs` (increasing): the module docstring's slot order"""
    half = 1 << (h - 1)
    ids = [half + q for q in pairs]
    before = None
    for q in pairs:
        ids += [(half + q) >> t for t in range(1, min(pair_cost(h, q, before), h - 1))]     # t = h - 1 is the root
        before = q
    if len(ids) + 1 > B:
        raise ValueError(f"the part's {len(ids) + 1} nodes exceed the {B} block slots")
    return ids + [0] * (B - 1 - len(ids)) + [1]


def plan_shape(po2: int, zk_cycles: int, W: int) -> Tuple[int, int]:
    """(h, B) of a plan, or the ValueError of a shape no plan exists for"""
    if W <= 16:
        raise ValueError(f"an image of {W} words has a single pair of leaves (W > 16)")
    h, B = tree_height(W), block_slots(po2, zk_cycles)
    if not MIN_H <= h <= MAX_H:
        raise ValueError(f"an image of {W} words has h {h} ({MIN_H} .. {MAX_H})")
    if B < h:
        raise ValueError(f"no room for the h {h} nodes of one path in {B} block slots (po2 {po2}, {zk_cycles} zk_cycles)")
    return h, B


def parts(po2: int, zk_cycles: int, W: int, addrs: Sequence[int]) -> List[Tuple[int, int]]:
    """The plan of a page-out with the addresses `addrs` (strictly increasing, below W) as a chain of P2-TREE traces: [(first, count)],
    part p the updates [first, first + count).  Greedy: a part takes whole pairs of leaves while its node count stays at most B; its
    first pair costs h nodes, every later one bit_length(pair index xor the pair index before).  No address: the one part (0, 0).
    zkh_page_tree_plan is the same plan in C."""
    h, B = plan_shape(po2, zk_cycles, W)
    plan, first, nodes, before = [], 0, 0, None
    for i, a in enumerate(addrs):
        q = int(a) >> 4
        if before is not None and q == before:
            continue
        cost = pair_cost(h, q, before)
        if nodes + cost > B:
            plan.append((first, i - first))
            first, nodes, cost = i, 0, h
        nodes += cost
        before = q
    return plan + [(first, len(addrs) - first)] if len(addrs) else [(0, 0)]


def cost_sums(addrs: Sequence[int]) -> np.ndarray:
    """S of the plan as a scan (DESIGN.md "THE PLAN AS A SCAN"): S[i] = c_0 + .. + c_i with c_0 = 0 and c_i = bit_length(q_i xor
    q_{i-1}) for the pair indices q = a >> 4, which is 0 where row i stays in row i - 1's pair of leaves"""
    q = np.asarray(addrs, dtype=np.int64).reshape(-1) >> 4
    c = np.zeros(q.size, dtype=np.int64)
    if q.size > 1:
        c[1:] = np.frexp((q[1:] ^ q[:-1]).astype(np.float64))[1]             # bit_length of an integer below 2^53; frexp(0) has exponent 0
    return np.cumsum(c)


def parts_by_scan(po2: int, zk_cycles: int, W: int, addrs: Sequence[int]) -> List[Tuple[int, int]]:
    """`parts` as a prefix sum and a search, the formulation zkh_page_tree_plan_device runs on the GPU: a part that starts at row f
    holds h + S[i] - S[f] nodes after row i, so the next part starts at the first i with S[i] > S[f] + B - h (S rises only where a
    new pair starts, so the search lands on one), and D ends the last part.  The same ValueErrors as `parts`."""
    h, B = plan_shape(po2, zk_cycles, W)
    S = cost_sums(addrs)
    D, plan, f = S.size, [], 0
    while f < D:
        nxt = int(np.searchsorted(S, S[f] + B - h, side="right"))            # the first i with S[i] > S[f] + B - h, D if there is none
        plan.append((f, nxt - f))
        f = nxt
    return plan or [(0, 0)]


def part_nodes(h: int, addrs: Sequence[int], plan: Sequence[Tuple[int, int]]) -> List[int]:
    """the dirty nodes of every part of `plan` over the table's addresses, from the same S: h + S[first + count - 1] - S[first]; the
    empty part of an empty table is the root block alone"""
    S = cost_sums(addrs)
    return [h + int(S[first + count - 1] - S[first]) if count else 1 for first, count in plan]


@functools.lru_cache(maxsize=4096)
def _block(inputs: Tuple[int, ...]) -> np.ndarray:
    """(48, 31) Montgomery words: the S and Q columns of one permutation over 16 raw Montgomery input words"""
    rows = block_rows([w * RINV % P for w in inputs] + [0] * 8)
    return np.array([[x * R % P for x in s + q] for s, q in rows], dtype=np.uint32).T


def reference_tree_part(po2: int, zk_cycles: int, W: int, table: Sequence[Tuple[int, int, int]], image_before, first: int, count: int):
    """-> (data, out) of the part [first, first + count) of `table` (rows (a, in, out), addresses strictly increasing and below W):
    the active rows of the data trace, (106, A) Montgomery words, and out = root_before ‖ root_after ‖ lo ‖ hi.  The yardstick of
    zkh_page_tree_witgen: the updates [0, first) are applied to a numpy copy of the image, plain trees (logup.reference_image_tree)
    are built before and after the part's own updates, and every block reads its 16 + 16 input words from those two trees."""
    from .logup import reference_image_tree
    image = np.array(image_before, dtype=np.uint32).reshape(-1)
    D = len(table)
    if image.size != W or W <= 16:
        raise ValueError(f"an image of {image.size} words for W = {W} (W > 16)")
    if not (0 <= first and 0 <= count and first + count <= D and (count or D == 0)):
        raise ValueError(f"the part [{first}, {first + count}) of a table of {D} rows")
    addrs = [int(row[0]) for row in table]
    for i, a in enumerate(addrs):
        if not (addrs[i - 1] if i else -1) < a < W:
            raise ValueError(f"row {i}: address {a} does not follow {addrs[i - 1] if i else -1} below {W}")
    for edge in (first, first + count):
        if 0 < edge < D and addrs[edge - 1] >> 4 == addrs[edge] >> 4:
            raise ValueError(f"the part [{first}, {first + count}) splits the pair of leaves {addrs[edge] >> 4} (rows {edge - 1} and {edge})")
    h, B = tree_height(W), block_slots(po2, zk_cycles)
    half, A = 1 << (h - 1), (1 << po2) - zk_cycles
    for a, _, w_out in table[:first]:
        image[a] = int(w_out)
    old = reference_image_tree(image)
    for a, w_in, w_out in table[first:first + count]:
        if int(image[a]) % P != int(w_in) % P:
            raise ValueError(f"address {a}: in {w_in}, but the image holds {int(image[a]) % P}")
        image[a] = int(w_out)
    new = reference_image_tree(image)
    pairs = sorted({a >> 4 for a in addrs[first:first + count]})
    ids = slot_ids(h, B, pairs)
    live = set(i for i in ids if i)
    base = half + (addrs[first - 1] >> 4) + 1 if first else half
    hi = half + pairs[-1] + 1 if pairs else base
    data = np.zeros((WD, A), dtype=np.uint32)
    for slot, i in enumerate(ids):
        rows = slice(BLOCK_ROWS * slot, BLOCK_ROWS * (slot + 1))
        for tree, at in ((old, D_SO), (new, D_SN)):
            inputs = tuple(int(w) for w in np.concatenate([tree[2 * i], tree[2 * i + 1]])) if i else (0,) * 16
            blk = _block(inputs)
            data[at:at + T, rows], data[at + T:at + 2 * T, rows] = blk[:T], blk[T:]
        leaf = i >= half
        lo = (ids[slot - 1] + 1 if slot else base) if leaf else hi
        g = i - lo if leaf else 0
        if not 0 <= g < 1 << GAP_BITS:
            raise ValueError(f"slot {slot}: id {i} does not follow {lo - 1} by a gap of {GAP_BITS} bits")
        r0 = BLOCK_ROWS * slot
        data[D_ID, rows], data[D_IDL, rows], data[D_IDR, rows] = enc(i), enc(2 * i), enc(2 * i + 1)
        data[D_LEAF, rows], data[D_UP, rows] = R * leaf, R * (i > 1)
        data[D_DL, rows], data[D_DR, rows] = R * (0 < i < half and 2 * i in live), R * (0 < i < half and 2 * i + 1 in live)
        data[D_LO, rows] = enc(lo)
        data[D_GBIT, r0 + 1:r0 + 1 + GAP_BITS], data[D_GACC, r0 + 1:r0 + 1 + GAP_BITS] = p2_blocks.gap_columns(g)
        data[D_GACC, r0 + BLOCK_ROWS - 1] = enc(g)
    out = np.concatenate([old[1], new[1], [enc(base), enc(hi)]]).astype(np.uint32)
    return data, out


if __name__ == "__main__":      # python -m zeth_amd.circuits.p2_tree out.desc out.args   (blobs for non-Python hosts)
    import sys
    desc, args = build_p2_tree()
    np.asarray(desc, dtype="<u4").tofile(sys.argv[1])
    print(f"{sys.argv[1]}: {desc.size} words")
    if len(sys.argv) > 2:
        np.asarray(args, dtype="<u4").tofile(sys.argv[2])
        print(f"{sys.argv[2]}: {args.size} words")
