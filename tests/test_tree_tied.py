"""P2-TREE-tied on the host (zeth_amd/circuits/p2_tree_tied.py; logup.py "THE SPLIT CLOSURE"; DESIGN.md §2 "THE TIE"): the description
and its blob; the descriptions that must not have moved, against hashes recorded on the parent commit; the reference witness against
every constraint (circuits/check.py) and the parts' totals against the plain-Python fingerprint of their table; each new constraint and
the split closing step biting, named by family; and what prover.link_tied_tree_chain refuses of the parts' `out` words.

Shapes are page_tree_cases': (10, 500, 64) is a tree of 7 blocks, (12, 1994, 8 * 17 + 3) has a partial last leaf, (10, 500, 512) with every
word takes several parts.  The split closure is shown on an image of 32 words at po2 7: a root block over one pair block."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import page_tree_cases as tc
import tree_tied_cases as cases
from tied_cases import f4_add
from zeth_amd.circuits import check, logup, p2_blocks, p2_page_ordered, p2_page_tied, p2_tree, p2_tree_tied as TT, syn_lookup
from zeth_amd.circuits.desc import GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import link_tied_tree_chain

P, ONE, CHALLENGE = cases.P, cases.ONE, cases.CHALLENGE
BLOCK = p2_blocks.BLOCK_ROWS
MIX = np.zeros(TT.MIX_WORDS, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ nothing moved
def test_the_descriptions_that_were_there_have_not_moved():
    sha = lambda a: hashlib.sha256(np.asarray(a, dtype="<u4").tobytes()).hexdigest()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_tied_nothing_moved.json")) as fh:
        want = json.load(fh)
    got = {}
    for name, blobs in (("p2_tree", p2_tree.build_p2_tree()), ("p2_page_tied", p2_page_tied.build_p2_page_tied()), ("syn_lookup_tiny_tied", syn_lookup.syn_lookup_tiny_tied())):
        got[name + ".desc"], got[name + ".args"] = sha(blobs[0]), sha(blobs[1])
    got["p2_page_ordered.desc"] = sha(p2_page_ordered.build_p2_page_ordered())
    assert got == want
    assert [t["tag"] for t in p2_tree.bus_terms()] == [k // 3 + 1 for k in range(18)]             # the first-tag argument defaults to P2-TREE's tags


# ------------------------------------------------------------------------------------------------ the description
def test_the_description_is_kind_9_with_an_open_bus_of_34_terms_in_12_columns():
    desc, blob = TT.build_p2_tree_tied()
    assert [int(desc[i]) for i in (3, 4, 5, 7, 13)] == [48, 41, 138, 31, 9] == [TT.WA, TT.WC, TT.WD, TT.OUT_WORDS, TT.KIND_P2_TREE_TIED]
    args = logup.Arguments.parse(blob)
    assert blob[1] == 8 and args.version == 8 and np.array_equal(args.blob(), blob)
    assert (args.open.tag, args.open.alpha, args.open.beta, args.open.total, args.open.out_words) == (logup.TIE_TAG, 19, 23, 27, 31)
    assert len(args.terms) == 34 and args.k == 12
    cols = args.by_column()
    assert [len(ts) for ts in cols] == [3] * 11 + [1]
    digest, open_ = [t for ts in cols[:6] for t in ts], [t for ts in cols[6:] for t in ts]
    assert len(digest) == 18 and sorted({t.tag for t in digest}) == list(range(11, 17)) and logup.TIE_TAG not in {t.tag for t in digest}
    assert len(open_) == 16 and all(t.tag == logup.TIE_TAG and t.sign == -1 and t.sel == TT.C_IN_ROW for t in open_)
    assert [t.mult for t in open_] == [(GROUP_DATA, TT.D_CH + j) for j in range(16)]
    assert [t.tuple_cols for t in open_] == [((GROUP_DATA, TT.D_WA + j), (GROUP_DATA, TT.D_SO + j), (GROUP_DATA, TT.D_SN + j)) for j in range(16)]
    assert max(logup.column_degree(ts) for ts in cols) <= logup.MAX_DEGREE == 5
    # the digest terms are P2-TREE's but for the tags, and the families are P2-TREE's with `words` before the bus
    plain = logup.Arguments.parse(p2_tree.arguments()).terms
    assert [(t.col, t.tuple_cols, t.sign, t.sel, t.mult, t.tag + 10) for t in plain] == [(t.col, t.tuple_cols, t.sign, t.sel, t.mult, t.tag) for t in digest]
    p2_tree.build_p2_tree()
    assert [f[0] for f in TT.FAMILIES] == ["rounds", "in_row", "carry", "order", "root", "words", "bus", "sanity"]
    assert [f[0] for f in TT.FAMILIES if f[0] != "words"] == [f[0] for f in p2_tree.FAMILIES]
    # the code group is P2-TREE's: the blob of the option-less description is the same blob, only the description differs
    loose = TT.build_p2_tree_tied(split_close=False)
    assert np.array_equal(loose[1], blob) and not np.array_equal(loose[0], desc)


def test_the_builder_refuses_a_column_that_mixes_open_and_closed_terms_under_the_option():
    make = lambda **kw: logup.LogupBuilder((8, 2, 4), (16, 8), alpha=4, beta=8, open_bus=(logup.TIE_TAG, 12), **kw)
    b = make(split_close=True)
    b.term(0, [(GROUP_DATA, 0)], tag=1)
    with pytest.raises(ValueError, match=r"^accum column 0 mixes terms of the open tag 2 with others \(split_close: a column is open or closed\)$"):
        b.term(0, [(GROUP_DATA, 1)], sign=-1, tag=logup.TIE_TAG)
    assert len(b.terms) == 1
    b.term(1, [(GROUP_DATA, 1)], sign=-1, tag=logup.TIE_TAG)                                    # a column of its own
    b.term(1, [(GROUP_DATA, 2)], sign=-1, tag=logup.TIE_TAG)
    with pytest.raises(ValueError, match="^accum column 1 mixes"):
        b.term(1, [(GROUP_DATA, 3)], tag=5)
    b = make()                                                                                  # without the option a column may mix them, as before
    b.term(0, [(GROUP_DATA, 0)], tag=1)
    b.term(0, [(GROUP_DATA, 1)], sign=-1, tag=logup.TIE_TAG)
    with pytest.raises(ValueError, match="split_close is an option of the open bus"):
        logup.LogupBuilder((8, 2, 4), (16, 8), split_close=True)


# ------------------------------------------------------------------------------------------------ the reference witness
def _check(desc, po2, accum, code, data, out):
    return check.first_failure(check.reference_check_rows(desc, po2, accum, code, data, out, MIX))


@pytest.mark.parametrize("g", cases.grid(), ids=cases.grid_id)
def test_the_reference_witness_satisfies_every_constraint(g):
    (po2, zk, W), what, p = g
    data, accum, out, code = cases.part(po2, zk, W, what, p)
    assert _check(TT.p2_tree_tied_circuit(), po2, accum, code, data, out) == (-1, check.NONE, 0)
    # the first 106 columns and the first 18 words are P2-TREE's, word for word; base is the word of the image's height
    tree_data, tree_out, _ = tc.part(po2, zk, W, what, p)
    assert np.array_equal(data[:p2_tree.WD], tree_data) and np.array_equal(out[:TT.PREFIX_WORDS], tree_out)
    t = tc.table(po2, zk, W, what)
    assert int(out[TT.OUT_BASE]) == TT.out_base(t["h"]) and TT.decode(out[TT.OUT_BASE]) == 16 << (t["h"] - 1)
    assert np.array_equal(out[TT.OUT_ALPHA:TT.OUT_TOTAL], CHALLENGE)
    # the touched words are the part's rows: ch marks count of them, each at its address, on input rows only
    first, count = t["plan"][p]
    ch, wa = data[TT.D_CH:TT.D_WA], data[TT.D_WA:]
    assert int((ch == ONE).sum()) == count and not ch[:, np.arange(ch.shape[1]) % BLOCK != 0].any() and not wa[:, np.arange(ch.shape[1]) % BLOCK != 0].any()
    assert sorted(TT.decode(w) for w in wa[ch == ONE]) == [int(a) for a in t["addrs"][first:first + count]]


@pytest.mark.parametrize("s,what", cases.TABLES, ids=lambda v: str(v))
def test_the_parts_totals_and_the_tables_fingerprint_cancel(s, what):
    t = tc.table(*s, what)
    parts = range(len(t["plan"]))
    fingerprint = logup.table_fingerprint(t["table"], CHALLENGE[:4], CHALLENGE[4:])
    totals = [cases.part(*s, what, p)[2][TT.OUT_TOTAL:] for p in parts]
    assert not f4_add(fingerprint, *totals).any()
    if not t["table"]:                                                                          # no row to alter: an empty table's total is zero
        assert not fingerprint.any() and not totals[0].any()
        return
    assert fingerprint.any() and (len(totals) == 1 or f4_add(fingerprint, *totals[:-1]).any())
    # one `out` word of one row altered on the page-out side only: the parts seal another table, and the sum is not zero
    forged = [cases.part(*s, what, p, altered=True)[2][TT.OUT_TOTAL:] for p in parts]
    assert f4_add(fingerprint, *forged).any()
    assert not f4_add(logup.table_fingerprint(cases.altered_table(t["table"]), CHALLENGE[:4], CHALLENGE[4:]), *forged).any()


# ------------------------------------------------------------------------------------------------ each new constraint bites
def _tampered(edit, out_edit=None):
    """the first failure of H3 one_pair's part after `edit(data)` (the accum recomputed, so that the bus agrees with the tampered data)
    -> (row, the family of its step)"""
    po2, zk, W = cases.H3
    data, _, out, code = cases.part(po2, zk, W, "one_pair")
    data = data.copy()
    edit(data)
    accum, out = cases.reaccumulate(po2, zk, data, out)
    if out_edit:
        out_edit(out)
    row, step, _ = _check(TT.p2_tree_tied_circuit(), po2, accum, code, data, out)
    return row, TT.family_of(step) if row >= 0 else None


def test_each_new_constraint_bites():
    po2, zk, W = cases.H3
    data, _, out, _ = cases.part(po2, zk, W, "one_pair")                                        # addresses 3, 12, 63: pair blocks 4 and 7 in slots 0 and 1
    t = tc.table(po2, zk, W, "one_pair")
    assert [TT.decode(data[TT.D_ID, BLOCK * s]) for s in range(2)] == [4, 7] and data[TT.D_LEAF, BLOCK * 2] == 0
    assert data[TT.D_CH + 3, 0] == ONE and data[TT.D_SO + 3, 0] != data[TT.D_SN + 3, 0]         # word 3 is touched, and changed
    assert _tampered(lambda d: None) == (-1, None)
    # ch cleared on a changed word
    def clear(d): d[TT.D_CH + 3, 0] = 0
    assert _tampered(clear) == (0, "words")
    # ch set in an inner block (slot 2 is the first block above the pairs)
    def inner(d): d[TT.D_CH + 5, BLOCK * 2] = ONE
    assert _tampered(inner) == (BLOCK * 2, "words")
    # wa off by one on a touched word, in the second pair block
    def off_by_one(d): d[TT.D_WA + 15, BLOCK] = p2_blocks.enc(64)
    assert data[TT.D_CH + 15, BLOCK] == ONE and TT.decode(data[TT.D_WA + 15, BLOCK]) == 63
    assert _tampered(off_by_one) == (BLOCK, "words")
    # ... but not on a word that is not touched: its address is no row of anything
    def untouched(d): d[TT.D_WA + 4, 0] = p2_blocks.enc(99)
    assert data[TT.D_CH + 4, 0] == 0 and _tampered(untouched) == (-1, None)
    # out[18] of another h: every touched word's address is off by 16 * 2^(h-1)
    def other_h(o): o[TT.OUT_BASE] = TT.out_base(t["h"] + 1)
    assert _tampered(lambda d: None, other_h) == (0, "words")
    # a set ch that is not boolean
    def two(d): d[TT.D_CH + 3, 0] = p2_blocks.enc(2)
    assert _tampered(two) == (0, "words")


def test_the_split_closure_bites_where_the_single_closing_step_does_not():
    """a digest pair that is produced and never consumed: with one closing step sum_c S_c = F the prover moves the surplus into F and
    every constraint holds (the hole: the group check would then balance digest tuples ACROSS parts); with the split closure the
    closed columns must sum to zero on `last`, and do not"""
    po2, zk, W = cases.TWO_BLOCKS
    data, accum, out, code = cases.two_blocks()
    tight, loose = TT.build_p2_tree_tied()[0], TT.build_p2_tree_tied(split_close=False)[0]
    assert _check(tight, po2, accum, code, data, out) == (-1, check.NONE, 0) and _check(loose, po2, accum, code, data, out) == (-1, check.NONE, 0)
    root = slice(BLOCK, 2 * BLOCK)
    assert (data[p2_tree.D_DL, root] == ONE).all() and not data[p2_tree.D_DR, root].any() and TT.decode(data[TT.D_ID, BLOCK]) == 1
    assert np.array_equal(data[TT.D_SO:TT.D_SO + 16, BLOCK], data[TT.D_SN:TT.D_SN + 16, BLOCK])   # in = out: old = new, so a clean child is no lie
    forged = data.copy()
    forged[p2_tree.D_DL, root] = 0                                                                   # the root no longer consumes its left child's digests
    accum2, out2 = cases.reaccumulate(po2, zk, forged, out)                                     # F = the true sum of ALL columns
    assert not np.array_equal(out2[TT.OUT_TOTAL:], out[TT.OUT_TOTAL:])
    assert _check(loose, po2, accum2, code, forged, out2) == (-1, check.NONE, 0)                # the hole
    row, step, failing = _check(tight, po2, accum2, code, forged, out2)
    assert (row, failing) == ((1 << po2) - zk - 1, 1) and TT.family_of(step) == "bus"           # the `last` row, and only it
    reads = check.explain_step(tight, step)
    assert {c // 4 for g, c, _ in reads["taps"] if g == 0} == set(range(TT.DIGEST_COLS)) and not reads["globals"]     # sum over the closed columns = 0
    # and F alone cannot be anything but the open columns' sum
    out3 = out.copy()
    out3[TT.OUT_TOTAL] = (int(out3[TT.OUT_TOTAL]) + ONE) % P
    row, step, failing = _check(tight, po2, accum, code, data, out3)
    assert (row, failing) == ((1 << po2) - zk - 1, 1) and TT.family_of(step) == "bus"
    reads = check.explain_step(tight, step)
    assert {c // 4 for g, c, _ in reads["taps"] if g == 0} == set(range(TT.DIGEST_COLS, 12)) and (0, TT.OUT_TOTAL) in reads["globals"]


def _cut_off(shape, fake_root):
    """the forgery of a part that states a row with in != out and leaves root_after = root_before -> (first failing row, its family, the
    number of failing rows).
    The pair block keeps its touched word on the open bus; the root slot becomes a no-op (dl = 0, new side = old side), and `out` says
    root_after = root_before.  fake_root False: the pair block is cut off itself (up = 0).  fake_root True: it still produces, and the
    dead slot between becomes a second block of id 1 with up = 0 that consumes it; the digest bus balances either way"""
    po2, zk, W = shape
    data, _, out, code = cases.two_blocks(shape, changed=True)
    B = p2_tree.block_slots(po2, zk)
    pair, root = slice(0, BLOCK), slice(BLOCK * (B - 1), BLOCK * B)
    assert not np.array_equal(out[:8], out[8:16]) and data[TT.D_CH + 5, 0] == ONE and data[TT.D_SO + 5, 0] != data[TT.D_SN + 5, 0]
    forged = data.copy()
    if fake_root:
        forged[:p2_tree.WD, BLOCK:2 * BLOCK] = data[:p2_tree.WD, root]                        # id 1, up 0, dl 1: the honest root block, one slot early
    else:
        forged[p2_tree.D_UP, pair] = 0
    forged[p2_tree.D_DL, root] = 0
    forged[TT.D_SN:TT.D_SN + 48, root] = data[TT.D_SO:TT.D_SO + 48, root]                     # S_new ‖ Q_new := S_old ‖ Q_old
    accum, forged_out = cases.reaccumulate(po2, zk, forged, out)
    forged_out[8:16] = out[:8]
    assert np.array_equal(forged_out[TT.OUT_TOTAL:], out[TT.OUT_TOTAL:]) and forged_out[TT.OUT_TOTAL:].any()      # F still states the row
    row, step, failing = _check(TT.p2_tree_tied_circuit(), po2, accum, code, forged, forged_out)
    return row, TT.family_of(step) if row >= 0 else None, failing


def test_a_block_that_states_a_word_cannot_be_cut_off_from_the_tree():
    """P2-TREE lets a block with up = 0 outside the root slot stand: nothing reads it.  Here its touched words would still reach the open
    bus, so a part could state rows that never pass through the roots it names.  Every other constraint holds for both forgeries (the
    digest bus balances: the split closure does not see them); `words` refuses them on the cut-off block's output row, the one row that
    fails"""
    assert _cut_off(cases.TWO_BLOCKS, fake_root=False) == (BLOCK - 1, "words", 1)
    assert _cut_off(cases.THREE_BLOCKS, fake_root=False) == (BLOCK - 1, "words", 1)
    assert _cut_off(cases.THREE_BLOCKS, fake_root=True) == (2 * BLOCK - 1, "words", 1)
    for shape in (cases.TWO_BLOCKS, cases.THREE_BLOCKS):                                      # the honest witnesses of the same two shapes pass
        data, accum, out, code = cases.two_blocks(shape, changed=True)
        assert _check(TT.p2_tree_tied_circuit(), shape[0], accum, code, data, out) == (-1, check.NONE, 0)


# ------------------------------------------------------------------------------------------------ the links
def test_the_link_checks_of_verify_tied_tree():
    s, what = cases.H6, "all"
    t = tc.table(*s, what)
    h = t["h"]
    outs = [cases.part(*s, what, p)[2] for p in range(len(t["plan"]))]
    assert len(outs) >= 3
    root_before, root_after, hi = link_tied_tree_chain(outs, h)
    assert np.array_equal(root_before, logup.reference_image_root(t["image"])) and np.array_equal(root_after, logup.reference_image_root(t["image_after"]))
    assert hi == 1 << h
    half = 1 << (h - 1)
    with pytest.raises(HalError, match=re.escape(f"verify_page_tree_chain: part 0 starts at lo {half}, not 2^{h} = {2 * half}")):
        link_tied_tree_chain(outs, h + 1)                                                       # a wrong h
    bad = [o.copy() for o in outs]
    bad[1][TT.OUT_BASE] = TT.out_base(h + 1)
    with pytest.raises(HalError, match=re.escape(f"verify_tied_tree: part 1: base {32 * half} is not {16 * half} = 16 * 2^{h - 1}")):
        link_tied_tree_chain(bad, h)                                                            # a wrong base
    bad = [o.copy() for o in outs]
    lo1 = TT.decode(outs[1][p2_tree.OUT_LO])
    bad[1][p2_tree.OUT_LO] = p2_blocks.enc(lo1 + 1)
    with pytest.raises(HalError, match=re.escape(f"verify_page_tree_chain: part 1 starts at lo {lo1 + 1}, but part 0 left hi {lo1}")):
        link_tied_tree_chain(bad, h)                                                            # a part that does not start at the hi before it
    with pytest.raises(ValueError, match=r"^h 28 \(2 \.\. 27\)$"):
        TT.out_base(28)
