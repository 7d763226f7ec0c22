"""Paging memory in from an image and out again (ZKA1 version 7, the PAGES record; zeth_amd/circuits/logup.py, csrc/arguments.hip's
validator): the version-7 blob round-trips and versions 1..6 stay what they were; every new rule is reached by an edited blob with the
same message from the parser and the C validator on a GPU-less circuit, and by the builder; a refused blob leaves the circuit's arguments
as they were; `reference_links` with an image against a walk over the rows with a dictionary (pages_cases.walk), two segments chained
through `reference_page_out` against one walk over both; SYN-LOOKUP-paged against the row checker and the bus: the honest witness
holds, a forked page fails the gap constraint on exactly its row although the bus balances, a wrong p_out and an unlinked load that
ignores the image unbalance the bus and `describe_bus` names the key.  No GPU."""
import re

import numpy as np
import pytest

import pages_cases as pc
from zeth_amd import hal as zhal
from zeth_amd.circuits import check, logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_ACCUM, GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError

P = 2013265921
ONE = (1 << 32) % P
TINY = syn_lookup.TINY
NONE = logup.NONE
SIZES = (8, 6, 48)
N_TERMS = 4
REC_AT = [logup.ARGS_HEADER + 16 * N_TERMS + off for off in (0, 16, 48, 80)]    # record 0: LIMBS; 1: the paged LINK; 2: a LINK; 3: PAGES
WORDS = REC_AT[3] + 32
PAGE_DSTS = list(range(30, 41))


def _rec(i, w):
    return REC_AT[i] + w


def _builder(pages=True):
    """record 0: LIMBS; record 1: a LINK with READS, a selector, a clock and one value (the paged one); record 2: a LINK without READS;
    record 3: the PAGES record of record 1, 3 limbs of 8 bits, its destinations data 30 .. 40"""
    b = logup.LogupBuilder(SIZES, (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1)
    b.term(0, [(GROUP_CODE, 1)], sign=-1, mult=(GROUP_DATA, 4), tag=0, derive=True)              # term 1: derived multiplicity 4
    r1 = b.derive_links(3, (GROUP_DATA, 8), [(GROUP_DATA, 9), (GROUP_DATA, 10)], [11, 12, 13, 14, 15, 16, 17], 8, write=(GROUP_DATA, 22))
    r2 = b.derive_links(None, (GROUP_CODE, 4), [(GROUP_DATA, 18)], [19, 20, 21], 4)
    r3 = b.derive_pages(r1, PAGE_DSTS, 8) if pages else None
    r0 = b.derive_limbs((GROUP_CODE, 2), [5, 6, 7], 5)                                           # added last: it goes first, the PAGES target moves
    b.term(1, [(GROUP_DATA, 31), (GROUP_DATA, 32)], mult=(GROUP_DATA, 30), tag=2)                # term 2: + p_on (p_addr, p_in)
    b.term(1, [(GROUP_DATA, 35)], tag=0)                                                         # term 3: a lookup reads an address limb
    return b, (r0, r1, r2, r3)


def _all(pages=True):
    b, _ = _builder(pages)
    return b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0)))


def test_builder_round_trips_version_7():
    b, (r0, r1, r2, _) = _builder()
    r3 = b.records[3]
    assert b.records[:3] == [r0, r1, r2] and isinstance(r3, logup.Pages) and r3.link == 1        # the LIMBS record came later and went first
    assert (r3.p_on, r3.p_addr, r3.p_in, r3.p_out, r3.p_time, r3.alimbs, r3.gaps) == (30, 31, 32, 33, 34, (35, 36, 37), (38, 39, 40))
    assert b.paged(r1) == r3 and b.paged(r2) is None
    a = b.args()
    blob = a.blob()
    assert blob[1] == 7 and blob[6] == 4 and blob[7] == 0x10001 and blob.size == WORDS and a.reads == 1 and a.pages == r3
    assert list(blob[_rec(3, 0):]) == [4, 8, 3, 1] + [0] * 12 + PAGE_DSTS + [0] * 5
    back = logup.Arguments.parse(blob)
    assert back.version == 7 and back.records == [r0, r1, r2, r3] and back.terms == a.terms and np.array_equal(back.blob(), blob)
    assert back.plain().version == 1
    # without the PAGES record the same records are the version-6 blob they were: the LINK's own words do not change
    _, blob6 = _all(pages=False)
    assert blob6[1] == 6 and blob6[7] == 1 and blob6[6] == 3 and blob6.size == WORDS - 32
    same = blob[:WORDS - 32].copy()
    same[[1, 6, 7]] = blob6[[1, 6, 7]]
    assert np.array_equal(same, blob6)
    assert np.array_equal(logup.Arguments.parse(blob6).blob(), blob6)


def test_earlier_versions_are_what_they_were():
    """SYN-LOOKUP's blobs and descriptions without pages= do not change (the digests pinned in test_logup_links.py and test_logup_reads.py
    say the same), and a version-5 or version-6 blob marked version 7 is no ZKA1 blob: its header word 7 lacks bit 16"""
    for kw in (dict(link=True), dict(link=True, reads=True), dict(sort=True), dict(order=True, sort=True)):
        blob = syn_lookup.build_syn_lookup(TINY, **kw)[1]
        assert int(blob[1]) < 7 and not int(blob[7]) & 0x10000
        bad = blob.copy()
        bad[1] = 7
        with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
            logup.Arguments.parse(bad)


PAGES_RANGE = r"a PAGES record of {} limbs of {} bits \(1\.\.4 limbs of 1\.\.16 bits, at most 29 bits in all\)"
PAGES_RESERVED = r"a reserved word of a PAGES record is not 0 \(words 4\.\.15 and the unused destination words\)"
PAGES_TARGET = r"a PAGES record pages record {}, which is no LINK record with READS and two carried columns \(a clock and one value\)"
# (edits of the blob of `_all()`, the message of the parser and of the C validator), in the order of the rules
BLOB_EDITS = [
    ([(7, 0x10002)], "header word 7 is 2, the blob has 1 LINK records with READS"),
    ([(7, 0x30001)], "header word 7 is 131073, the blob has 1 LINK records with READS"),
    ([(_rec(3, 0), 3)], r"header word 7 has bit 16 \(PAGES\), but the blob has no PAGES record"),  # the record reads as a LINK: no PAGES record is left
    ([(_rec(2, 0), 4)], r"record 3: a second PAGES record \(record 2 is one: a blob pages one memory\)"),
    ([(7, 0x10000), (_rec(1, 0), 4)], r"record 2: a record after the PAGES record 1 \(the PAGES record comes last\)"),
    ([(_rec(3, 1), 0)], "record 3: " + PAGES_RANGE.format(3, 0)),
    ([(_rec(3, 1), 17)], "record 3: " + PAGES_RANGE.format(3, 17)),
    ([(_rec(3, 1), 10)], "record 3: " + PAGES_RANGE.format(3, 10)),                              # 30 bits
    ([(_rec(3, 2), 0)], "record 3: " + PAGES_RANGE.format(0, 8)),
    ([(_rec(3, 2), 5)], "record 3: " + PAGES_RANGE.format(5, 8)),
    ([(_rec(3, 4), 1)], "record 3: " + PAGES_RESERVED),
    ([(_rec(3, 15), 9)], "record 3: " + PAGES_RESERVED),
    ([(_rec(3, 27), 41)], "record 3: " + PAGES_RESERVED),                                        # past the 11 destinations
    ([(_rec(3, 2), 2)], "record 3: " + PAGES_RESERVED),                                          # two limbs: 9 destinations, the last two words are set
    ([(_rec(3, 3), 0)], "record 3: " + PAGES_TARGET.format(0)),                                  # a LIMBS record
    ([(_rec(3, 3), 2)], "record 3: " + PAGES_TARGET.format(2)),                                  # a LINK without READS
    ([(_rec(3, 3), 3)], "record 3: " + PAGES_TARGET.format(3)),                                  # itself
    ([(_rec(3, 3), 9)], "record 3: " + PAGES_TARGET.format(9)),
    ([(_rec(3, 17), 30)], r"record 3: its destination \(data 30\) appears twice"),
    ([(_rec(3, 20), 8)], r"record 1: its source \(data 8\) is a destination of record 3 \(records never chain\)"),   # the LINK objects first
    ([(_rec(3, 20), 13)], r"record 1: its destination \(data 13\) is also written by record 3"),
    ([(_rec(3, 20), 5)], r"record 3: its destination \(data 5\) is also written by record 0"),
    ([(_rec(3, 20), 4)], r"record 3: its destination \(data 4\) is the derived multiplicity of term 1"),
    ([(_rec(3, 20), 18)], r"record 2: its source \(data 18\) is a destination of record 3"),
    ([(_rec(0, 4), GROUP_DATA), (_rec(0, 5), 33)], r"record 3: its destination \(data 33\) is read by record 0 \(the links run after the columns, and never chain\)"),
    ([(_rec(3, 16), 31), (_rec(3, 17), 30)], r"record 3: its destination \(data 30\) is the multiplicity of term 2 \(of a PAGES record's destinations only p_on may be\)"),
]
# ... and what only a validator that knows the circuit can refuse (the builder and the C validator)
SHAPE_EDITS = [
    ([(_rec(3, 20), 48)], "record 3: destination 48 is not a data column"),
]
# ... and what the rules allow
GOOD_EDITS = [
    [(_rec(3, 1), 7), (_rec(3, 2), 4)],                                                          # four limbs of 7 bits: 13 destinations
    [(_rec(3, 20), 47)],
]


def _edited(blob, edit):
    bad = blob.copy()
    for w, v in edit:
        bad[w] = v
    if edit == GOOD_EDITS[0]:
        bad[_rec(3, 27)], bad[_rec(3, 28)] = 41, 42
    return bad


def test_parser_refuses_every_rule():
    _, blob = _all()
    assert blob.size == WORDS and blob[1] == 7
    for edit in ([(7, 1)], [(7, 0)], [(7, 0x20001)], [(1, 8)]):                                  # version 7 without bit 16; no version 8
        with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
            logup.Arguments.parse(_edited(blob, edit))
    with pytest.raises(ValueError, match=r"^ZKA1: \d+ words for 4 terms and 4 records$"):           # version 6 knows no 32-word record of kind 4
        logup.Arguments.parse(_edited(blob, [(1, 6), (7, 1)]))
    for edit, msg in BLOB_EDITS:
        with pytest.raises(ValueError, match="ZKA1: " + msg):
            logup.Arguments.parse(_edited(blob, edit))
    for edit in GOOD_EDITS:
        a = logup.Arguments.parse(_edited(blob, edit))
        assert np.array_equal(a.blob(), _edited(blob, edit))
    for edit, msg in SHAPE_EDITS:
        a = logup.Arguments.parse(_edited(blob, edit))
        assert logup.check_pages(a.terms, a.records) is None
        assert re.search(msg, logup.check_pages(a.terms, a.records, SIZES))


def test_builder_refuses_and_keeps_its_state():
    b, (r0, r1, r2, _) = _builder()
    before = list(b.records)
    with pytest.raises(ValueError, match=r"record 4: a second PAGES record \(record 3 is one"):
        b.derive_pages(r1, list(range(41, 48)), 8)
    b2, (_, q1, q2, _) = _builder(pages=False)
    for rec, dsts, bits, msg in ((q2, PAGE_DSTS, 8, "record 3: " + PAGES_TARGET.format(2)),
                                 (q1, PAGE_DSTS, 10, "record 3: " + PAGES_RANGE.format(3, 10)),
                                 (q1, PAGE_DSTS[:-1] + [13], 8, r"record 1: its destination \(data 13\) is also written by record 3"),
                                 (q1, PAGE_DSTS[:-1] + [48], 8, "record 3: destination 48 is not a data column")):
        with pytest.raises(ValueError, match=msg):
            b2.derive_pages(rec, dsts, bits)
    with pytest.raises(ValueError, match="destinations"):
        b2.derive_pages(q1, PAGE_DSTS[:6], 8)
    assert b.records == before and b.args().version == 7 and b2.args().version == 6 and len(b2.records) == 3
    with pytest.raises(ValueError, match=r"record 3: its destination \(data 33\) is the multiplicity of term 4 \(of a PAGES record's destinations only p_on may be\)"):
        b.term(1, [(GROUP_DATA, 31)], sign=-1, mult=(GROUP_DATA, 33), tag=2)
    assert len(b.terms) == 4


def _c_set(hc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))


def _derived(hc):
    cols, n = np.zeros(64, dtype=np.uint32), zhal.C.c_size_t()
    zhal._check(zhal._lib.zkh_circuit_derived_data_columns(hc.h, zhal._ptr(cols), cols.size, zhal.C.byref(n)))
    return [int(x) for x in cols[:n.value]]


def test_c_validator_on_a_gpu_less_circuit_gives_the_same_messages():
    desc, blob = _all()
    hc = zhal.HostCircuit(desc)
    pages = lambda: zhal._lib.zkh_circuit_pages(hc.h)
    assert pages() == 0
    _c_set(hc, blob)
    assert pages() == 1 and zhal._lib.zkh_circuit_links_check_reads(hc.h) == 1 and zhal._lib.zkh_circuit_derives_links(hc.h) == 1
    want = [4, 5, 6, 7] + list(range(11, 18)) + [19, 20, 21] + PAGE_DSTS
    assert _derived(hc) == want                                               # the page table crosses PCIe on its blinding rows only
    for edit in ([(7, 1)], [(7, 0)], [(7, 0x20001)], [(1, 8)]):
        with pytest.raises(HalError, match=r"set_arguments: not a ZKA1 \(version 1\) argument blob$"):
            _c_set(hc, _edited(blob, edit))
    with pytest.raises(HalError, match=r"set_arguments: \d+ words for 4 terms and 4 records$"):
        _c_set(hc, _edited(blob, [(1, 6), (7, 1)]))
    for edit, msg in BLOB_EDITS + SHAPE_EDITS:
        with pytest.raises(HalError, match="set_arguments: " + msg):
            _c_set(hc, _edited(blob, edit))
    assert _derived(hc) == want and pages() == 1                             # a refused blob leaves the circuit's arguments as they were
    for edit in GOOD_EDITS:
        _c_set(hc, _edited(blob, edit))
        assert pages() == 1
    _, blob6 = _all(pages=False)
    _c_set(hc, blob6)
    assert pages() == 0 and _derived(hc) == want[:-11]
    with pytest.raises(HalError, match=r"set_arguments: not a ZKA1 \(version 1\) argument blob$"):
        _c_set(hc, _edited(blob6, [(1, 7)]))
    assert pages() == 0


# ---- the reference against a walk over the rows ----
@pytest.mark.parametrize("po2,zk", [(6, 3), (8, 40), (10, 300)])
def test_reference_links_with_an_image_equals_a_dictionary_walk(po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(pc.KINDS):
        desc, blob, code, data, image = pc.case(kind, 50 * po2 + i, po2, zk)
        args = logup.Arguments.parse(blob)
        assert args.version == 7 and args.pages.link == 0
        got = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
        out, mem = pc.walk(code, data, image, A, kind)
        want = data.copy()
        for c, v in out.items():
            want[c, :A] = v
        if kind == "two":                                                    # the record that is not paged is what it is alone
            alone = logup.Arguments(args.k, args.alpha, args.beta, args.terms, [args.records[1]])
            want[pc.SECOND + 3:pc.SECOND + 10] = logup.reference_links(alone, po2, zk, code.reshape(-1), data.reshape(-1)).reshape(-1, n)[pc.SECOND + 3:pc.SECOND + 10]
        assert np.array_equal(got, want), kind
        rows = pc.accesses(code, data, A, kind)
        D = len(mem)
        assert D == {"equal": 1, "distinct": A, "range5": 5, "edges": 4}.get(kind, D) and (got[pc.P_ON, :A] == ONE).sum() == D
        firsts = rows[got[pc.LINKED, rows] == 0]
        loads = firsts[(data[pc.WRITE, firsts] % P == 0) & (got[pc.PVALUE, firsts] % P != 0)]
        assert len(firsts) == D and 4 * len(loads) >= D, (kind, D, len(loads))      # first accesses that the image answers, with non-zero words
        # page-out: the image with what the last access of every address left
        after = logup.reference_page_out(args, po2, zk, got.reshape(-1), image)
        want_image = image.copy()
        for a, v in mem.items():
            want_image[a] = v
        assert np.array_equal(after, want_image)
        with pytest.raises(logup.ReferenceError, match=re.escape(logup.PAGES_NEED_IMAGE)):
            logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1))


@pytest.mark.parametrize("kind", ["sparse", "big", "two", "edges"])
def test_two_segments_chained_through_page_out_equal_one_walk(kind):
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code1, data1, image0 = pc.case(kind, 7, po2, zk)
    args = logup.Arguments.parse(blob)
    full1 = logup.reference_links(args, po2, zk, code1.reshape(-1), data1.reshape(-1), image=image0)
    image1 = logup.reference_page_out(args, po2, zk, full1, image0)
    assert not np.array_equal(image1, image0)
    _, blob2, code2, data2, same = pc.case(kind, 7, po2, zk, image=image1, trace_seed=8)          # the second segment's loads see the first one's stores
    assert np.array_equal(blob2, blob)
    image1 = same                                                            # (`big` writes some of its words as raw words >= P)
    full2 = logup.reference_links(args, po2, zk, code2.reshape(-1), data2.reshape(-1), image=image1).reshape(-1, n)
    image2 = logup.reference_page_out(args, po2, zk, full2.reshape(-1), image1)
    # one walk over both segments, the memory in one dictionary that starts from image0
    out1, mem1 = pc.walk(code1, data1, image0, A, kind)
    out2, mem2 = pc.walk(code2, data2, image0, A, kind, memory=mem1)
    for c, v in out2.items():
        assert np.array_equal(full2[c, :A] % P, v % P), c                    # residues: `big` rewrote words of image1 as raw words >= P
    assert set(mem1) & set(mem2)
    final = image0.copy()
    for a, v in list(mem1.items()) + list(mem2.items()):
        final[a] = v
    assert np.array_equal(image2 % P, final % P)


def _refuses(args, po2, zk, code, data, image, msg):
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image)


def test_reference_refuses_as_documented():
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = pc.case("two", 3, po2, zk)
    args = logup.Arguments.parse(blob)
    W = len(image)
    x = lambda v: int(pc.dec(v))
    first = {}
    for r in range(A):
        first.setdefault(x(data[pc.KEY, r]), r)
    r = sorted(first.values())[10]                                           # a first access
    a = x(data[pc.KEY, r])
    d = data.copy()
    d[pc.KEY, r] = pc.enc(W)
    _refuses(args, po2, zk, code, d, image, f"record 0 at row {r}: address {W} outside the image of {W} words")
    d[pc.WRITE, r] = pc.enc(2)                                               # the write flag comes first
    _refuses(args, po2, zk, code, d, image, f"record 0 at row {r}: write flag 2, not 0 or 1")
    d = data.copy()
    d[pc.CLOCK, r] = 0
    _refuses(args, po2, zk, code, d, image, f"record 0 at row {r}: clock 0 is the image's")
    d[pc.KEY, r] = pc.enc(W + 5)                                             # the address comes before the clock
    _refuses(args, po2, zk, code, d, image, f"record 0 at row {r}: address {W + 5} outside the image of {W} words")
    d = data.copy()
    d[pc.WRITE, r], d[pc.VALUE, r] = 0, pc.enc(x(image[a]) + 1)
    msg = f"record 0 at row {r}: a load of carried column 1 returns {(x(image[a]) + 1) % P}, but the image holds {x(image[a])} at its address {a}"
    _refuses(args, po2, zk, code, d, image, msg)
    d[pc.CLOCK, r] = pc.enc((1 << 24) + 1)                                   # the clock comes before the read rule
    _refuses(args, po2, zk, code, d, image, f"record 0 at row {r}: the clock difference {1 << 24} (after the image) does not fit 3 limbs of 8 bits")
    d = data.copy()
    d[pc.WRITE, r], d[pc.VALUE, r] = 0, np.uint32(int(image[a]) % P + P) if int(image[a]) % P + P < 1 << 32 else image[a]
    logup.reference_links(args, po2, zk, code.reshape(-1), d.reshape(-1), image=image)           # the same residue as a raw word >= P holds
    # the PAGES record's own refusal comes after every LINK's: an address that its limbs do not hold (here: a short PAGES record)
    short = logup.Arguments(args.k, args.alpha, args.beta, args.terms, args.records[:2] + [logup.Pages(2, 2, 0, args.pages.dsts[:9])])
    low = min(rr for aa, rr in first.items() if aa >= 16)
    _refuses(short, po2, zk, code, data, image, f"record 2 at row {low}: address {x(data[pc.KEY, low])} does not fit 2 limbs of 2 bits")
    d = data.copy()
    d[pc.SECOND, A - 1], d[pc.SECOND + 1, A - 1] = d[pc.SECOND, A - 2], d[pc.SECOND + 1, A - 2]
    t = x(d[pc.SECOND + 1, A - 2])
    _refuses(short, po2, zk, code, d, image, f"record 1 at row {A - 1}: clock not increasing ({t} after {t} at row {A - 2})")
    # page-out's own refusals, the image unchanged
    full = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
    for edit, msg in (((pc.P_ON, 3, pc.enc(2)), "record 2 at row 3: p_on 2, not 0 or 1"),
                      ((pc.P_ADDR, 3, pc.enc(W)), f"record 2 at row 3: address {W} outside the image of {W} words"),
                      ((pc.P_ADDR, 3, full[pc.P_ADDR, 2]), f"record 2 at row 3: page address {x(full[pc.P_ADDR, 2])} does not follow a smaller one "
                                                           f"(row 2: p_on 1, address {x(full[pc.P_ADDR, 2])})"),
                      ((pc.P_ON, 2, 0), f"record 2 at row 3: page address {x(full[pc.P_ADDR, 3])} does not follow a smaller one "
                                        f"(row 2: p_on 0, address {x(full[pc.P_ADDR, 2])})")):
        bad = full.copy()
        bad[edit[0], edit[1]] = edit[2]
        with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
            logup.reference_page_out(args, po2, zk, bad.reshape(-1), image)


# ---- SYN-LOOKUP-paged against the row checker and the bus ----
def _paged(po2=8, zk=40, W=64, seed=1):
    desc, blob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True, reads=True, pages=True)
    rng = np.random.default_rng(seed)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, full, out = syn_lookup.witness(TINY, po2, zk, seed=seed, addr_range=W, link=True, reads=True, pages=True, image=image)
    mix = rng.integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    return desc, blob, logup.Arguments.parse(blob), image, code, full, out, mix


def _recount(args, po2, zk, code, data):
    """the multiplicities counted again: a forger's limbs are looked up like any other"""
    n = 1 << po2
    m = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[2]
    d = np.array(data, dtype=np.uint32).reshape(-1, n)
    d[m, :n - zk] = 0
    return logup.reference_multiplicities(args, po2, zk, code, d.reshape(-1))


def test_syn_lookup_paged_shape_and_switches():
    desc, blob = syn_lookup.syn_lookup_tiny_paged()
    a = logup.Arguments.parse(blob)
    pcols = syn_lookup.pages_layout(2, 4)
    assert (int(desc[5]), len(a.terms), a.k, a.version, len(a.records), int(blob[7])) == (33, 22, 8, 7, 2, 0x10001) and pcols == list(range(22, 33))
    reads = logup.Arguments.parse(syn_lookup.syn_lookup_tiny_reads()[1])
    assert a.records[0] == reads.records[0] and a.pages == logup.Pages(4, 3, 0, tuple(pcols))   # the LINK's words are version 6's
    assert not any(t.mult in ((GROUP_DATA, 14), (GROUP_DATA, 15)) for t in a.terms)              # nothing uses linked or last as a multiplicity
    assert [t.tuple_cols for t in a.terms if t.mult == (GROUP_DATA, 22)] == [((GROUP_DATA, 23), (GROUP_DATA, 24)),
                                                                             ((GROUP_DATA, 23), (GROUP_DATA, 25), (GROUP_DATA, 26))]
    with pytest.raises(ValueError, match="pages=True pages the memory of a LINK record with the read rule"):
        syn_lookup.build_syn_lookup(TINY, link=True, pages=True)
    with pytest.raises(ValueError, match="pages=True pages one memory: n_mem is 3"):
        syn_lookup.build_syn_lookup(syn_lookup.MULTI, link=True, reads=True, pages=True)
    with pytest.raises(ValueError, match="it needs link=, reads=True and image="):
        syn_lookup.witness(TINY, 8, 40, link=True, reads=True, pages=True)
    assert logup.Arguments.parse(syn_lookup.syn_lookup_paged()[1]).version == 7


def test_the_honest_witness_satisfies_every_row_and_the_bus():
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, args, image, code, full, out, mix = _paged(po2, zk)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=1, addr_range=64, link=False, reads=True, pages=False, image=image, count=False, limbs=False)
    pcols = syn_lookup.pages_layout(2, 4)
    assert not bare.reshape(-1, n)[pcols, :A].any() and full.reshape(-1, n)[pcols[0], :A].sum() > 0
    chain = logup.reference_links(args, po2, zk, code, logup.reference_columns(args, po2, zk, code, bare), image=image)
    chain = logup.reference_multiplicities(args, po2, zk, code, chain)
    assert np.array_equal(chain, full)                                        # columns -> links (paged) -> multiplicities = the host-made witness
    accum, total = logup.reference_accumulate(args, po2, zk, code, full, mix)
    assert total == [0, 0, 0, 0]
    assert check.first_failure(check.reference_check_rows(desc, po2, accum, code, full, out, mix)) == (-1, NONE, 0)
    assert logup.reference_bus(args, po2, zk, code, full)["row"] == -1
    w = full.reshape(-1, n)
    first = w[14, :A] == 0                                                    # unlinked: the image answers
    assert (first & (w[21, :A] == 0) & (w[12, :A] != 0)).sum() * 4 >= first.sum() and np.array_equal(w[17, :A][first], np.zeros(first.sum()))
    assert np.array_equal(w[16, :A][first], image[logup._dec(w[11, :A][first]).astype(np.int64)])


def test_a_forked_page_fails_the_gap_constraint_on_exactly_its_row():
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, args, image, code, full, out, mix = _paged(po2, zk)
    forged, row = syn_lookup.fork_page(TINY, full, po2, zk, image)
    forged = _recount(args, po2, zk, code, forged)
    f, w = forged.reshape(-1, n), full.reshape(-1, n)
    pcols = syn_lookup.pages_layout(2, 4)
    assert f[pcols[1], row] == f[pcols[1], row - 1] and (f[pcols[0], :A] != 0).sum() == (w[pcols[0], :A] != 0).sum() + 1   # one address, two pages
    accum, total = logup.reference_accumulate(args, po2, zk, code, forged, mix)
    assert total == [0, 0, 0, 0] and logup.reference_bus(args, po2, zk, code, forged)["row"] == -1      # the bus still balances
    per_row = check.reference_check_rows(desc, po2, accum, code, forged, out, mix)
    bad_row, step, count = check.first_failure(per_row)
    assert (bad_row, count) == (row, 1)
    taps = check.explain_step(desc, step)["taps"]
    assert (GROUP_DATA, pcols[1], 1) in taps and all((GROUP_DATA, c, 0) in taps for c in pcols[8:])   # p_addr@1 and the gap limbs
    with pytest.raises(logup.ReferenceError, match="does not follow a smaller one"):
        logup.reference_page_out(args, po2, zk, forged, image)


def test_a_wrong_p_out_and_a_load_that_ignores_the_image_unbalance_the_bus():
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, args, image, code, full, out, mix = _paged(po2, zk)
    plain = args.plain()
    pcols = syn_lookup.pages_layout(2, 4)
    w = full.reshape(-1, n)
    bad = w.copy()
    bad[pcols[3], 5] = (int(bad[pcols[3], 5]) + ONE) % P                     # page 5 writes another value out
    bus = logup.reference_bus(plain, po2, zk, code, bad.reshape(-1))
    addr = int(logup._dec(w[pcols[1], 5]))
    assert bus["row"] >= 0 and bus["tag"] == 1 and bus["key"][0] == addr
    line = logup.describe_bus(bus, plain)
    assert f"key (tag 1; {addr}, " in line and "does not balance" in line
    with pytest.raises(logup.ReferenceError, match="the bus does not balance"):
        logup.reference_accumulate(plain, po2, zk, code, bad.reshape(-1), mix)
    # an unlinked load that returns 0 as if memory started zeroed: its own tuple (addr, 0, time) is never removed
    r = next(r for r in range(A) if w[14, r] == 0 and w[21, r] == 0 and w[12, r] != 0)
    bad = w.copy()
    bad[12, r] = 0
    a = int(logup._dec(w[11, r]))
    with pytest.raises(logup.ReferenceError, match=re.escape(f"at row {r}: a load of carried column 1 returns 0, but the image holds")):
        logup.reference_links(args, po2, zk, code, bad.reshape(-1), image=image)
    bus = logup.reference_bus(plain, po2, zk, code, bad.reshape(-1))
    assert bus["row"] >= 0 and bus["tag"] == 1 and bus["key"][0] == a
    assert f"key (tag 1; {a}, " in logup.describe_bus(bus, plain)
    accum, _ = logup.reference_accumulate(plain, po2, zk, code, bad.reshape(-1), mix, check_balance=False)
    assert check.first_failure(check.reference_check_rows(desc, po2, accum, code, bad.reshape(-1), out, mix))[0] == r   # (1 - w)(val - pval) on its row
