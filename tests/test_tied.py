"""THE TIE on the host (zeth_amd/circuits/logup.py "THE OPEN BUS", syn_lookup.py SYN-LOOKUP-tied, p2_page_tied.py): a
paging segment's seal and the seals of its page-out chain on one bus.  The ZKA1 version-8 blob (the OPEN record) through the Python
parser and the library's, by message; the open totals of host-made witnesses against the plain-Python table_fingerprint, their sum
over a segment and its chain of parts, and a page-out side with one altered word; circuits/check.py on both tied witnesses; the shared
challenge (zkh_tie_challenge); the new exports.

The segment is SYN-LOOKUP-tied's tiny shape at po2 8 over an image of 64 words; its page table is sealed by P2-PAGE-tied parts at
page_ordered_cases' h = 3 shape (po2 12, 22 slots): three parts, the last with dead slots."""
import ctypes as C

import numpy as np
import pytest

import page_ordered_cases as oc
from tied_cases import CHALLENGE, ONE, P, PAGE_PO2, PAGE_ZK, SEG_PO2, SEG_ZK, W, enc, f4_add, parts, segment, segment_total
from zeth_amd import hal as zhal
from zeth_amd.circuits import check, logup, p2_page, p2_page_ordered, p2_page_tied as T, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_DATA


# ------------------------------------------------------------------------------------------------ the blob
def test_version_8_round_trips_and_the_builder_writes_it_only_for_an_open_bus():
    for desc, blob in (sl.syn_lookup_tiny_tied(), T.build_p2_page_tied()):
        args = logup.Arguments.parse(blob)
        assert blob[1] == 8 and args.version == 8 and args.open is not None and args.open.tag == logup.TIE_TAG
        assert blob[7] & logup.OPEN_BIT and int(blob[-16]) == logup.KIND_OPEN
        assert np.array_equal(args.blob(), blob)
        assert (args.open.alpha, args.open.beta) == (args.alpha, args.beta) and args.open.out_words == int(desc[7])
    tiny = logup.Arguments.parse(sl.syn_lookup_tiny_tied()[1]).open
    assert (tiny.alpha, tiny.beta, tiny.total, tiny.out_words) == (4, 8, 12, 16)
    page = logup.Arguments.parse(T.arguments())
    assert (page.open.alpha, page.open.beta, page.open.total, page.open.out_words) == (18, 22, 26, 30) and page.k == 1 and len(page.terms) == 1
    assert page.pages is None and not blob[7] & logup.PAGES_BIT                  # version 8 asks for neither a PAGES record nor READS
    # every earlier version is written exactly when it was
    kw = [({}, 1), ({"derive": True}, 2), ({"sort": True}, 3), ({"limbs": True}, 4), ({"link": True}, 5), ({"link": True, "reads": True}, 6),
          ({"link": True, "reads": True, "pages": True}, 7)]
    for k, version in kw:
        blob = sl.build_syn_lookup(sl.TINY, **k)[1]
        assert blob[1] == version and logup.Arguments.parse(blob).open is None


def test_the_tied_descriptions_are_their_own_and_the_others_are_untouched():
    paged, tied = sl.syn_lookup_tiny_paged(), sl.syn_lookup_tiny_tied()
    assert int(paged[0][7]) == 4 and int(tied[0][7]) == sl.TIED_OUT == 16 and int(tied[0][3]) == int(paged[0][3])      # one more term, the same 8 columns
    desc = T.p2_page_tied_circuit()
    assert [int(desc[i]) for i in (3, 4, 5, 7, 13)] == [T.WA, 42, 129, 30, T.KIND_P2_PAGE_TIED]
    p2_page_ordered.build_p2_page_ordered()
    assert [f[0] for f in T.FAMILIES] == [f[0] for f in p2_page_ordered.FAMILIES] and "order" in [f[0] for f in T.FAMILIES]
    assert max(p2_page.constraint_degrees(desc)) <= 4


def _refusals():
    blob = sl.syn_lookup_tiny_tied()[1]
    n = blob.size
    open_at, pages_at = n - 16, n - 48
    e = []
    b = np.concatenate([blob[:pages_at], blob[open_at:], blob[pages_at:open_at]])
    e.append((b, "record 2: a record after the OPEN record 1 (the OPEN record comes last)"))
    b = blob.copy(); b[open_at + 4] = 13
    e.append((b, "record 2: the total at out words 13..16, the circuit has 16"))
    b = blob.copy(); b[open_at + 2] = 14
    e.append((b, "record 2: alpha at out words 14..17, the circuit has 16"))
    b = np.concatenate([blob, blob[open_at:]]); b[6] += 1
    e.append((b, "record 3: a second OPEN record (record 2 is one: a seal closes on one total)"))
    b = blob.copy(); b[open_at + 3] = 6
    e.append((b, "record 2: alpha, beta and the total overlap in out (words 4, 6, 12: 4 words each)"))
    b = blob.copy(); b[open_at + 9] = 1
    e.append((b, "record 2: a reserved word of the OPEN record is not 0 (words 6..15)"))
    b = blob.copy(); b[open_at + 1] = 7
    e.append((b, "record 2: no term has the open tag 7"))
    b = blob.copy(); b[3] = 0
    e.append((b, "record 2: header words 3, 4 are 0, 8, the OPEN record's alpha, beta are 4, 8"))
    return e


def test_both_parsers_refuse_a_bad_open_record_with_the_same_words():
    desc, blob = sl.syn_lookup_tiny_tied()
    hc = zhal.HostCircuit(desc)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(blob), blob.size))
    where = np.zeros(4, dtype=np.uint32)
    assert zhal._lib.zkh_circuit_open_bus(hc.h, zhal._ptr(where)) == 1 and list(where) == [logup.TIE_TAG, 4, 8, 12]
    for bad, msg in _refusals():
        bad = np.ascontiguousarray(bad, dtype=np.uint32)
        with pytest.raises(ValueError) as py:
            logup.Arguments.parse(bad)
        assert str(py.value) == "ZKA1: " + msg
        with pytest.raises(zhal.HalError) as c:
            zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(bad), bad.size))
        assert str(c.value) == "set_arguments: " + msg
    for edit in ([(7, int(blob[7]) ^ logup.OPEN_BIT)], [(1, 9)]):                 # version 8 without bit 17; no version 9
        bad = blob.copy()
        for w, v in edit:
            bad[w] = v
        with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
            logup.Arguments.parse(bad)
        with pytest.raises(zhal.HalError, match="not a ZKA1"):
            zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(bad), bad.size))
    bad = blob[:-16].copy(); bad[6] -= 1
    with pytest.raises(ValueError, match=r"^ZKA1: header word 7 has bit 17 \(OPEN\), but the blob has no OPEN record$"):
        logup.Arguments.parse(bad)
    # the OPEN record is of ONE circuit: SYN-LOOKUP-paged has 4 out words
    paged = zhal.HostCircuit(sl.syn_lookup_tiny_paged()[0])
    with pytest.raises(zhal.HalError, match="accum Fp4 columns|the OPEN record is of a circuit with 16 out words, this one has 4"):
        zhal._check(zhal._lib.zkh_circuit_set_arguments(paged.h, zhal._ptr(blob), blob.size))


def test_the_builder_refuses_offsets_outside_out_and_a_derived_open_term():
    with pytest.raises(ValueError, match="the total at out words 14..17, the circuit has 16"):
        logup.LogupBuilder((4, 2, 4), (16, 8), alpha=4, beta=8, open_bus=(2, 14))
    b = logup.LogupBuilder((4, 2, 4), (16, 8), alpha=4, beta=8, open_bus=(2, 12))
    b.term(0, [(GROUP_DATA, 0)], tag=1)
    with pytest.raises(ValueError, match="no term has the open tag 2"):
        b.args()
    b.term(0, [(GROUP_DATA, 1)], sign=-1, mult=(GROUP_DATA, 2), tag=2, derive=True)
    with pytest.raises(ValueError, match="term 1 of the open tag 2 is derived or a sorted copy"):
        b.args()


# ------------------------------------------------------------------------------------------------ the totals
def test_the_segments_open_total_is_the_fingerprint_of_its_page_table():
    s = segment()
    _, total = segment_total()
    assert len(s["table"]) > 2 * oc.table(PAGE_PO2, PAGE_ZK, W, 0)["N"] and any(i == o for _, i, o in s["table"])
    assert np.array_equal(total, logup.table_fingerprint(s["table"], CHALLENGE[:4], CHALLENGE[4:])) and total.any()
    assert np.array_equal(logup.table_fingerprint([], CHALLENGE[:4], CHALLENGE[4:]), np.zeros(4, dtype=np.uint32))
    with pytest.raises(logup.ReferenceError, match="a challenge of 4 words"):
        logup.reference_accumulate(s["args"], SEG_PO2, SEG_ZK, s["code"], s["data"], CHALLENGE[:4])
    # every other term nets to zero inside the seal: the bus check passes with the open tag's keys skipped, and fails if they are not
    assert logup.reference_bus(s["args"], SEG_PO2, SEG_ZK, s["code"], s["data"])["row"] == -1
    closed = logup.Arguments(s["args"].k, 0, 4, s["args"].terms, [r for r in s["args"].records if not isinstance(r, logup.Open)])
    found = logup.reference_bus(closed, SEG_PO2, SEG_ZK, s["code"], s["data"])
    assert found["tag"] == logup.TIE_TAG and found["unbalanced_keys"] == len(s["table"])


def test_the_totals_of_a_segment_and_its_chain_of_parts_cancel():
    s = segment()
    _, seg_total = segment_total()
    chain = parts()
    assert len(chain) == 3
    totals = [out[T.OUT_TOTAL:] for _, _, out in chain]
    assert not f4_add(seg_total, *totals).any()
    assert f4_add(seg_total, *totals[:2]).any()
    # a part's total is minus the fingerprint of its own live rows, and a part without a live row would add nothing
    N = oc.table(PAGE_PO2, PAGE_ZK, W, 0)["N"]
    for p, total in enumerate(totals):
        rows = s["table"][p * N:(p + 1) * N]
        assert not f4_add(total, logup.table_fingerprint(rows, CHALLENGE[:4], CHALLENGE[4:])).any()
    for p, (data, _, out) in enumerate(chain):                                    # the rest of a part is P2-PAGE-ordered's, word for word
        want_data, want_out = p2_page_ordered.reference_ordered_part(PAGE_PO2, PAGE_ZK, W, s["table"], s["image"], p * N)
        assert np.array_equal(out[:T.PREFIX_WORDS], want_out) and np.array_equal(data, want_data)
    assert all(np.array_equal(out[T.OUT_ALPHA:T.OUT_TOTAL], CHALLENGE) for _, _, out in chain)


def test_the_fixed_challenge_separates_the_altered_table():
    s = segment()
    table = list(s["table"])
    a, w_in, w_out = table[1]
    table[1] = (a, w_in, (w_out + ONE) % P)
    honest = logup.table_fingerprint(s["table"], CHALLENGE[:4], CHALLENGE[4:])
    forged = logup.table_fingerprint(table, CHALLENGE[:4], CHALLENGE[4:])
    assert not np.array_equal(honest, forged)                                      # on the CPU, before anything rests on it


def test_one_altered_out_word_on_the_page_out_side_leaves_a_sum_that_is_not_zero():
    _, seg_total = segment_total()
    totals = [out[T.OUT_TOTAL:] for _, _, out in parts(altered=True)]
    assert f4_add(seg_total, *totals).any()


# ------------------------------------------------------------------------------------------------ circuits/check.py
def _check(desc, po2, accum, code, data, out):
    f = check.reference_check_rows(desc, po2, accum, code, data, out, np.zeros(int(desc[8]), dtype=np.uint32))
    return check.first_failure(f)


def test_check_accepts_the_tied_segment_and_names_the_closing_step_when_the_total_is_off_by_one():
    s = segment()
    accum, total = segment_total()
    out = np.concatenate([np.zeros(4, dtype=np.uint32), CHALLENGE, total])
    assert _check(s["desc"], SEG_PO2, accum, s["code"], s["data"], out) == (-1, check.NONE, 0)
    out[sl.OUT_TOTAL] = (int(out[sl.OUT_TOTAL]) + ONE) % P
    row, step, failing = _check(s["desc"], SEG_PO2, accum, s["code"], s["data"], out)
    assert (row, failing) == ((1 << SEG_PO2) - SEG_ZK - 1, 1)                       # the `last` row, and only it
    e = check.explain_step(s["desc"], step)
    assert (0, sl.OUT_TOTAL) in e["globals"] and {g for g, _, _ in e["taps"]} == {0} and len(e["taps"]) == s["args"].k      # sum_c S_c[0] - out[F]
    # with another challenge in `out` the first row's terms no longer match the accum
    out = np.concatenate([np.zeros(4, dtype=np.uint32), CHALLENGE[::-1], total])
    assert _check(s["desc"], SEG_PO2, accum, s["code"], s["data"], out)[0] == 0


def test_check_accepts_a_tied_part_and_names_the_closing_step_when_the_total_is_off_by_one():
    desc = T.p2_page_tied_circuit()
    t = oc.table(PAGE_PO2, PAGE_ZK, W, 0)
    code = oc.code_of(PAGE_PO2, PAGE_ZK, t["h"])
    n = 1 << PAGE_PO2
    for p, (active, accum, out) in enumerate(parts()):
        if p == 1:
            continue                                                              # the first part, and the last with its dead slots
        data = np.zeros((T.WD, n), dtype=np.uint32)
        data[:, :n - PAGE_ZK] = active
        assert _check(desc, PAGE_PO2, accum, code, data, out) == (-1, check.NONE, 0), p
        bad = out.copy()
        bad[T.OUT_TOTAL + 2] = (int(bad[T.OUT_TOTAL + 2]) + ONE) % P
        row, step, failing = _check(desc, PAGE_PO2, accum, code, data, bad)
        assert (row, failing) == (p2_page.BLOCK_ROWS * t["h"] * t["N"] - 1, 1) and T.family_of(step) == "accum"          # the last path's top row
        assert (0, T.OUT_TOTAL + 2) in check.explain_step(desc, step)["globals"]
    dead = parts()[2][0]
    live = dead[T.D_LIVE, ::p2_page.BLOCK_ROWS * t["h"]][:t["N"]]
    assert 0 < int((live == ONE).sum()) < t["N"]


# ------------------------------------------------------------------------------------------------ the challenge
def test_tie_challenge_is_a_function_of_the_roots_in_their_order():
    rng = np.random.default_rng(11)
    roots = rng.integers(0, P, (4, 8), dtype=np.uint64).astype(np.uint32)
    ch = zhal.tie_challenge(roots)
    assert ch.shape == (8,) and (ch < P).all() and len(set(ch.tolist())) == 8
    assert np.array_equal(ch, zhal.tie_challenge(roots.copy()))
    changed = roots.copy(); changed[2, 5] = (int(changed[2, 5]) + 1) % P
    swapped = roots[[0, 2, 1, 3]]
    seen = [ch, zhal.tie_challenge(changed), zhal.tie_challenge(swapped), zhal.tie_challenge(roots[:3]), zhal.tie_challenge(roots[:1])]
    assert len({tuple(c.tolist()) for c in seen}) == len(seen)
    with pytest.raises(zhal.HalError, match="tie_challenge: a root word is not a reduced element"):
        bad = roots.copy(); bad[1, 1] = P
        zhal.tie_challenge(bad)
    with pytest.raises(zhal.HalError, match="tie_challenge: roots of 12 words"):
        zhal.tie_challenge(roots.reshape(-1)[:12])


def test_the_new_exports_are_present_and_bound():
    lib = zhal.load_library()
    for name in ("zkh_accumulate_open", "zkh_circuit_open_bus", "zkh_table_fingerprint", "zkh_data_root", "zkh_seal_data_root", "zkh_tie_challenge"):
        assert hasattr(lib, name) and name in zhal.ABI, name
    assert isinstance(C.cast(lib.zkh_tie_challenge, C.c_void_p).value, int)
