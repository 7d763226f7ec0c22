"""THE TIE of a wide memory on the host (zeth_amd/circuits/syn_lookup.py SYN-LOOKUP-tied-wide; logup.py FLAT): the tiny tied-wide segment
at po2 8 over a flat image of 64 words, that is 32 addresses of two value words and a tree of height 3.  Its open total under tied_cases'
fixed challenge is the fingerprint of its FLAT table of 64 rows (2 a + j, in_j, out_j); it cancels in Fp4 against the totals of the
page-out's parts, P2-TREE-tied's two and P2-PAGE-tied's three, which know nothing of V; one altered `out` word on the page-out side leaves
a sum that is not zero.  circuits/check.py on the open-bus witness; what `_refuse_wide` still refuses.  No GPU."""
import numpy as np
import pytest

import flat_cases as fc
from tied_cases import CHALLENGE, ONE, P, enc, f4_add
from zeth_amd import page_seal
from zeth_amd.circuits import check, logup, p2_page, p2_page_tied as T, p2_tree, p2_tree_tied as TT, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_DATA
from zeth_amd.hal import HalError

SEG_PO2, SEG_ZK, WORDS = fc.SEG_PO2, fc.SEG_ZK, fc.WORDS


def test_what_the_cases_rest_on_holds_for_the_wide_witness_of_seed_3():
    """before anything else: the figures the tests below, and the GPU tests, take for granted"""
    s = fc.segment()
    table = s["table"]
    addrs = [a for a, _, _ in table]
    assert len(table) == 64 and addrs == list(range(64))                     # D = 32 addresses: every one of the image's, 64 flat rows
    assert {a >> 4 for a in addrs} == {0, 1, 2, 3}                           # in the pair blocks 0 .. 3
    assert sum(i == o for _, i, o in table) == 2 and sum(i != o for _, i, o in table) == 62
    assert p2_tree.parts(*fc.TWO_PARTS, WORDS, addrs) == [(0, 48), (48, 16)] and p2_tree.parts(*fc.ONE_PART, WORDS, addrs) == [(0, 64)]
    assert len(p2_page.parts(fc.PAGE_PO2, fc.PAGE_ZK, WORDS, 64)) == 3
    assert logup._tree_height(WORDS) == fc.H


def test_the_circuit_is_its_own_and_the_named_ones_follow():
    desc, blob = sl.syn_lookup_tiny_tied_wide()
    args = logup.Arguments.parse(blob)
    assert blob[1] == 11 and args.flat and args.wide and args.open is not None and args.open.tag == logup.TIE_TAG and int(desc[7]) == sl.TIED_OUT == 16
    tie = [t for t in args.terms if t.tag == logup.TIE_TAG]
    pg = args.pages
    assert [t.tuple_cols for t in tie] == [((GROUP_DATA, pg.flats[j]), (GROUP_DATA, pg.p_ins[j]), (GROUP_DATA, pg.p_outs[j])) for j in range(2)]
    assert all(t.sign == 1 and t.mult == (GROUP_DATA, pg.p_on) for t in tie) and args.terms[-2:] == tie
    closed = sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, wide=True, flat=True)
    paged_wide = sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, wide=True)
    tied = sl.syn_lookup_tiny_tied()
    assert int(closed[0][7]) == 4 and int(closed[0][5]) == int(desc[5]) == int(paged_wide[0][5]) + 2
    assert len(logup.Arguments.parse(closed[1]).terms) + 2 == len(args.terms)
    digests = {bytes(np.asarray(d, dtype=np.uint32).tobytes()) for d in (desc, closed[0], paged_wide[0], tied[0])}
    assert len(digests) == 4                                                 # four descriptions, hence four control roots
    full, fblob = sl.syn_lookup_tied_wide()
    assert fblob[1] == 11 and int(full[7]) == 16 and logup.Arguments.parse(fblob).pages.ng == 3 and len(logup.Arguments.parse(fblob).pages.dsts) == 13
    pdesc, pblob = sl.build_syn_lookup(sl.MULTI, link=True, reads=True, pages=True, wide=True, flat=True, tied=True, ports=True)
    assert pblob[1] == 11 and int(pblob[7]) & logup.PORTS_BIT and logup.Arguments.parse(pblob).ports


def test_the_segments_open_total_is_the_fingerprint_of_its_flat_table():
    s = fc.segment()
    _, total = fc.segment_total()
    assert np.array_equal(total, logup.table_fingerprint(s["table"], CHALLENGE[:4], CHALLENGE[4:])) and total.any()
    # the table read off p_flat_j is the same one: the columns hold 2 a + j
    n, A = 1 << SEG_PO2, (1 << SEG_PO2) - SEG_ZK
    d, pg = s["data"].reshape(-1, n), s["args"].pages
    flat = np.stack([logup._dec(d[c, :32]) for c in pg.flats], axis=1).reshape(-1)
    assert [int(a) for a in flat] == [a for a, _, _ in s["table"]] and not d[list(pg.flats), 32:A].any()
    # every other term nets to zero inside the seal, and the tie's keys are the 64 flat rows
    assert logup.reference_bus(s["args"], SEG_PO2, SEG_ZK, s["code"], s["data"])["row"] == -1
    closed = logup.Arguments(s["args"].k, 0, 4, s["args"].terms, [r for r in s["args"].records if not isinstance(r, logup.Open)])
    found = logup.reference_bus(closed, SEG_PO2, SEG_ZK, s["code"], s["data"])
    assert found["tag"] == logup.TIE_TAG and found["unbalanced_keys"] == 64


def test_the_ported_segments_open_total_is_the_fingerprint_of_its_flat_table():
    s = fc.segment(ports=True)
    _, total = fc.segment_total(ports=True)
    assert s["args"].ports and len(s["table"]) == 64
    assert np.array_equal(total, logup.table_fingerprint(s["table"], CHALLENGE[:4], CHALLENGE[4:])) and total.any()


def test_the_totals_cancel_against_the_tree_parts_and_against_the_page_parts():
    _, seg_total = fc.segment_total()
    tree = [out[TT.OUT_TOTAL:] for _, _, out in fc.tree_parts()]
    assert len(tree) == 2 and not f4_add(seg_total, *tree).any() and f4_add(seg_total, tree[0]).any()
    page = [out[T.OUT_TOTAL:] for _, _, out in fc.page_parts()]
    assert len(page) == 3 and not f4_add(seg_total, *page).any() and f4_add(seg_total, *page[:2]).any()
    assert all(np.array_equal(out[TT.OUT_ALPHA:TT.OUT_TOTAL], CHALLENGE) for _, _, out in fc.tree_parts())


def test_one_altered_out_word_of_one_flat_row_leaves_a_sum_that_is_not_zero():
    s = fc.segment()
    honest = logup.table_fingerprint(s["table"], CHALLENGE[:4], CHALLENGE[4:])
    assert not np.array_equal(honest, logup.table_fingerprint(fc.altered(s["table"]), CHALLENGE[:4], CHALLENGE[4:]))      # the challenge tells them apart
    _, seg_total = fc.segment_total()
    assert f4_add(seg_total, *[out[TT.OUT_TOTAL:] for _, _, out in fc.tree_parts(True)]).any()
    assert f4_add(seg_total, *[out[T.OUT_TOTAL:] for _, _, out in fc.page_parts(True)]).any()


def test_check_accepts_the_tied_wide_segment_and_names_a_forged_flat_cell():
    s = fc.segment()
    accum, total = fc.segment_total()
    out = np.concatenate([np.zeros(4, dtype=np.uint32), CHALLENGE, total])
    mix = np.zeros(int(s["desc"][8]), dtype=np.uint32)
    rows = lambda data, o=out: check.first_failure(check.reference_check_rows(s["desc"], SEG_PO2, accum, s["code"], data, o, mix))
    assert rows(s["data"]) == (-1, check.NONE, 0)
    off = out.copy()
    off[sl.OUT_TOTAL] = (int(off[sl.OUT_TOTAL]) + ONE) % P
    assert rows(s["data"], off)[::2] == ((1 << SEG_PO2) - SEG_ZK - 1, 1)     # the `last` row closes on F, and only it
    # a flat cell off by one with the accum as it was: the term's constraint on that row, and the page constraint
    n = 1 << SEG_PO2
    d = s["data"].reshape(-1, n).copy()
    f1 = s["args"].pages.flats[1]
    d[f1, 7] = (int(d[f1, 7]) + ONE) % P
    f = check.reference_check_rows(s["desc"], SEG_PO2, accum, s["code"], d.reshape(-1), out, mix)
    assert check.first_failure(f)[0] == 7 and set(np.flatnonzero(f != check.NONE)) <= {7, 8}
    # ... and with the accum made again the bus closes on another total, but the page constraint still names row 7
    accum2, total2 = logup.reference_accumulate(s["args"], SEG_PO2, SEG_ZK, s["code"], d.reshape(-1), CHALLENGE)
    assert not np.array_equal(enc(total2), total)
    f = check.reference_check_rows(s["desc"], SEG_PO2, accum2, s["code"], d.reshape(-1), np.concatenate([out[:12], enc(total2)]), mix)
    row, step, failing = check.first_failure(f)
    assert (row, failing) == (7, 1)
    assert {(g, c) for g, c, _ in check.explain_step(s["desc"], step)["taps"]} == {(GROUP_DATA, s["args"].pages.p_on), (GROUP_DATA, f1), (GROUP_DATA, s["args"].pages.p_addr)}


# ------------------------------------------------------------------------------------------------ what is still refused
class _Circuit:
    def __init__(self, words, flats):
        self.words, self.flats = words, flats

    def page_words(self):
        return self.words

    def page_flats(self):
        return self.flats


class _Prover:
    hal = None

    def __init__(self, words, flats):
        self.circuit = _Circuit(words, flats)


def test_refuse_wide_refuses_only_a_wide_segment_without_flat_columns():
    msg = r"^{}: the segment's memory holds 2 value words per address \(ZKA1 version 10\): the tie of a wide memory is not built without flat-address columns"
    sp = _Prover(2, 0)
    with pytest.raises(HalError, match=msg.format("seal_tied")):
        page_seal.seal_tied(sp, None, None, None, None, None, [], None, 0, None, None)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree")):
        page_seal.seal_tied_tree(sp, None, None, None, None, None, [], None, 0, None, None)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree_from_proof")):
        page_seal.seal_tied_tree_from_proof(sp, None, None, None, None, None, [], None, None)
    with pytest.raises(HalError, match=msg.format("preflight_paged_run")):
        page_seal.preflight_paged_run(sp, [], [], None, None)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree_from_proof")):
        page_seal.seal_paged_step(page_seal.PagedStep(None, None, None, None, None, None), sp, None, None, [])
    for words, flats in ((2, 2), (1, 0), (0, 0)):                            # with flats, and narrow: not refused here
        page_seal._refuse_wide("seal_tied", _Prover(words, flats))
        assert page_seal.preflight_paged_run(_Prover(words, flats), [], [], None, None) == []
