"""The FLAT-ADDRESS columns of a wide page table on the CPU (ZKA1 version 11, zeth_amd/circuits/logup.py FLAT): the format and its rules, in
Python and in csrc/arguments.hip message for message, from ONE table of edited blobs; every earlier builder blob byte for byte; the numpy
twin `reference_links` against the address column of wide_cases.walk's flat table, in image and in table mode, with one record and with
three ports; and `page_constraints`' two new constraints under circuits/check.py: the honest tiny witness, and three forgeries.  No GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

import flat_cases as fc
import pages_cases as narrow
import wide_cases as wc
from zeth_amd import hal as zhal
from zeth_amd.circuits import check, logup, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_DATA
from zeth_amd.hal import HalError

HERE = os.path.dirname(os.path.abspath(__file__))
P, ONE = fc.P, fc.ONE
FLAT7 = logup.PAGES_BIT | logup.WIDE_BIT | logup.FLAT_BIT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _blob(kind="two", k=1):
    """(desc, the version-11 blob, the version-10 blob of the same circuit) of a small case; `two` has a LINK that is not paged: record 1"""
    if kind == "two":                                                        # flat_cases keeps wide_cases' kinds that page; `two` is built here
        _, old, code, data, image = wc.case("two", 1, 6, 3)
        wd = data.shape[0] + 2
        a = logup.Arguments.parse(old)
        out = []
        for flats in ((wd - 2, wd - 1), None):
            b = logup.LogupBuilder((4, wc.WC, wd), (4, 8))
            for t in a.terms:
                b.term(t.col, list(t.tuple_cols), tag=t.tag)
            built = [b.derive_links(r.sel, r.key, r.carried, r.dsts, r.limb_bits, write=r.write) for r in a.records[:2]]
            b.derive_pages(built[0], a.pages.dsts, a.pages.limb_bits, flats=flats)
            out.append(b.finish_all(b.arguments(b.true(), b.get(1, 0), b.get(1, 1), b.get(1, 2))))
        assert np.array_equal(out[1][1], old)
        return out[0][0], out[0][1], out[1][1]
    return fc.case(kind, 1, 6, 3, k)[:3]


def _pages_at(blob):
    return blob.size - 32


# ------------------------------------------------------------------------------------------------ the format
def test_version_11_round_trips_and_earlier_blobs_do_not_move():
    desc, blob, blob10 = _blob()
    a = logup.Arguments.parse(blob)
    wd = int(desc[5])
    assert a.version == 11 and blob[1] == 11 and blob[7] == 1 | FLAT7 and a.flat and a.wide and np.array_equal(a.blob(), blob)
    at = _pages_at(blob)
    assert list(blob[at:at + 16]) == [4, 8, 3, 0, 1, 2, wd - 2, wd - 1] + [0] * 8                 # word 5 holds F, words 6 and 7 the columns
    assert np.array_equal(blob[at + 16:], blob10[at + 16:]) and a.pages.flats == (wd - 2, wd - 1)  # the 16 destination slots are version 10's
    # the version-10 blob of the same circuit: word for word what it was, and it differs in the version, bit 20 and words 5 .. 7 alone
    a10 = logup.Arguments.parse(blob10)
    assert blob10[1] == 10 and a10.version == 10 and not a10.flat and a10.pages.flats == () and not int(blob10[7]) & logup.FLAT_BIT
    assert [int(i) for i in np.nonzero(blob != blob10)[0]] == [1, 7, at + 5, at + 6, at + 7]
    # with ports: bit 18 stands beside bits 19 and 20
    _, ported, _ = _blob("big", k=3)
    ap = logup.Arguments.parse(ported)
    assert ap.version == 11 and ported[7] == 3 | FLAT7 | logup.PORTS_BIT and np.array_equal(ap.blob(), ported)
    # V = 2 with ng = 4 uses 15 of the 16 slots: the flats do not ask for room there
    b = logup.LogupBuilder((4, 4, 40), (4, 8))
    b.term(0, [(GROUP_DATA, 39)])
    link = b.derive_links(None, (GROUP_DATA, 0), [(GROUP_DATA, 1), (GROUP_DATA, 2), (GROUP_DATA, 3)], list(range(5, 13)), 7, write=(GROUP_DATA, 4))
    rec = b.derive_pages(link, list(range(13, 28)), 7, flats=(28, 29))
    assert rec.ng == 4 and rec.n_dsts() == 15 and rec.flats == (28, 29) and logup.Arguments.parse(b.args().blob()).pages == rec


def test_every_earlier_builder_blob_is_byte_identical_with_flats_unused():
    for name in ("make_golden_syn_lookup_blobs", "make_golden_syn_lookup_wide_blobs"):       # versions 1 .. 10 of build_syn_lookup, descriptions included
        gen = _load(name)
        with open(gen.PATH) as fh:
            assert gen.record() == json.load(fh), name
    # derive_pages with flats=None, and with an empty list, writes the version-10 and the version-7 blob it wrote
    for case, version in ((wc.case("two", 1, 6, 3), 10), (narrow.case("two", 1, 6, 3), 7)):
        old = case[1]
        a = logup.Arguments.parse(old)
        for flats in (None, ()):
            b = logup.LogupBuilder((4, 8, 64), (4, 8))
            for t in a.terms:
                b.term(t.col, list(t.tuple_cols), tag=t.tag)
            built = [b.derive_links(r.sel, r.key, r.carried, r.dsts, r.limb_bits, write=r.write) for r in a.records[:2]]
            b.derive_pages(built[0], a.pages.dsts, a.pages.limb_bits, flats=flats)
            assert old[1] == version and np.array_equal(b.args().blob(), old)
    # a record without flats emits the constraints it emitted: SYN-LOOKUP-paged-wide's description is the pinned one (above), and flat=True is another
    wide = sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, wide=True)
    flat = sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, wide=True, flat=True)
    assert int(flat[0][5]) == int(wide[0][5]) + 2 and flat[0].size > wide[0].size and wide[1][1] == 10 and flat[1][1] == 11


def _as_11(blob, bits):
    bad = blob.copy()
    bad[1], bad[7] = 11, int(blob[7]) | bits
    return bad


def _edits():
    """[(the case whose circuit the blob is of, the blob, the message after 'ZKA1: ' / 'set_arguments: ')], every rule of version 11 once;
    None: no ZKA1 blob.  The one table behind the Python parser and zkh_circuit_set_arguments"""
    _, blob, blob10 = _blob()
    _, ported, _ = _blob("big", k=3)
    _, old, *_ = narrow.case("two", 1, 6, 3)
    at, nat, out = _pages_at(blob), _pages_at(old), []
    f0, f1 = int(blob[at + 6]), int(blob[at + 7])

    def edited(src, *edits):
        bad = src.copy()
        for w, v in edits:
            bad[w] = v
        return bad
    no_flat_record = r"header word 7 has bit 20 \(FLAT\), but no PAGES record has flat-address destinations"
    reserved = r"record 2: a reserved word of a PAGES record is not 0 \(words 8\.\.15, words 6 and 7 without flat-address destinations, and the unused destination words\)"
    word5 = r"record 2: word 5 of a PAGES record is {} \(F, the flat-address destinations: 0 or 2\)"
    out.append(("flat", edited(blob, (7, 1 | logup.PAGES_BIT | logup.WIDE_BIT)), None))          # version 11 without bit 20
    out.append(("flat", edited(blob, (1, 10)), "header word 7 is 1048577, the blob has 1 LINK records with READS"))     # bit 20 means nothing before version 11
    out.append(("flat", edited(blob, (1, 10), (7, 1 | logup.PAGES_BIT | logup.WIDE_BIT)),        # ... and version 10 reserves word 5 with the text it has
                r"record 2: a reserved word of a PAGES record is not 0 \(words 5\.\.15 and the unused destination words\)"))
    out.append(("flat", _as_11(blob10, logup.FLAT_BIT), no_flat_record))                         # bit 20 with F = 0
    out.append(("flat", edited(blob, (at + 5, 0)), no_flat_record))
    out.append(("flat", edited(blob, (at + 5, 1)), word5.format(1)))
    out.append(("flat", edited(blob, (at + 5, 3)), word5.format(3)))
    out.append(("narrow", edited(_as_11(old, logup.FLAT_BIT), (nat + 5, 2), (nat + 6, 40), (nat + 7, 41)),       # F = 2 with V = 1
                r"record 2: a PAGES record of one value word per address has 2 flat-address destinations \(they are the flat addresses of two value words\)"))
    out.append(("flat", edited(blob, (at + 8, 7)), reserved))
    out.append(("flat", edited(blob, (at + 15, 7)), reserved))
    out.append(("flat", edited(blob, (at + 31, 7)), reserved))
    out.append(("flat", edited(blob, (7, 1 | logup.PAGES_BIT | logup.FLAT_BIT)), r"a PAGES record pages two value words per address, but header word 7 lacks bit 19 \(WIDE\)"))
    out.append(("narrow", edited(_as_11(old, logup.FLAT_BIT | logup.WIDE_BIT), (nat + 5, 2)), r"header word 7 has bit 19 \(WIDE\), but no PAGES record pages two value words per address"))
    out.append(("ported", edited(ported, (7, 3 | FLAT7)), r"a LINK record joins, but header word 7 lacks bit 18 \(PORTS\)"))
    # ownership: p_flat_j are destinations like the others
    out.append(("flat", edited(blob, (at + 7, f0)), rf"record 2: its destination \(data {f0}\) appears twice"))
    out.append(("flat", edited(blob, (at + 6, int(blob[at + 16 + 2]))), rf"record 2: its destination \(data {int(blob[at + 16 + 2])}\) appears twice"))      # p_flat_0 = p_in_0
    out.append(("flat", edited(blob, (at + 6, wc.V1)), rf"record 0: its source \(data {wc.V1}\) is a destination of record 2 \(records never chain\)"))      # a value column
    out.append(("flat", edited(blob, (at + 7, wc.PER + wc.TABLE_W + 3)), rf"record 1: its destination \(data {wc.PER + wc.TABLE_W + 3}\) is also written by record 2"))      # the other LINK's `linked`
    assert f1 == f0 + 1
    return out


def test_parser_refuses_every_rule():
    for _, bad, msg in _edits():
        with pytest.raises(ValueError, match="^not a ZKA1 argument blob$" if msg is None else "^ZKA1: " + msg):
            logup.Arguments.parse(bad)


def test_builder_rules():
    b = logup.LogupBuilder((4, 4, 40), (4, 8))
    b.term(0, [(GROUP_DATA, 39)])
    one = b.derive_links(None, (GROUP_DATA, 0), [(GROUP_DATA, 1), (GROUP_DATA, 2)], list(range(5, 12)), 8, write=(GROUP_DATA, 4))
    with pytest.raises(ValueError, match=r"derive_pages: flat-address columns on a LINK that carries one value"):
        b.derive_pages(one, list(range(13, 24)), 8, flats=(30, 31))
    assert b.args().version == 6
    b = logup.LogupBuilder((4, 4, 40), (4, 8))
    b.term(0, [(GROUP_DATA, 39)])
    link = b.derive_links(None, (GROUP_DATA, 0), [(GROUP_DATA, 1), (GROUP_DATA, 2), (GROUP_DATA, 3)], list(range(5, 13)), 8, write=(GROUP_DATA, 4))
    with pytest.raises(ValueError, match=r"derive_pages: 1 flat-address columns \(2: p_flat_0, p_flat_1\)"):
        b.derive_pages(link, list(range(13, 26)), 8, flats=(30,))
    with pytest.raises(ValueError, match=r"record 1: destination 40 is not a data column"):
        b.derive_pages(link, list(range(13, 26)), 8, flats=(30, 40))
    assert b.args().version == 6
    rec = b.derive_pages(link, list(range(13, 26)), 8, flats=(30, 31))
    assert b.args().version == 11 and rec.flats == (30, 31)
    # of a PAGES record's destinations still only p_on may be a multiplicity; a term may READ a flat column
    for col in rec.flats:
        with pytest.raises(ValueError, match=rf"record 1: its destination \(data {col}\) is the multiplicity of term 1 \(of a PAGES record's destinations only p_on may be\)"):
            b.term(0, [(GROUP_DATA, 38)], sign=-1, mult=(GROUP_DATA, col))
    b.term(0, [(GROUP_DATA, rec.flats[0]), (GROUP_DATA, rec.p_ins[0])], sign=-1, mult=(GROUP_DATA, rec.p_on))
    assert len(b.terms) == 2
    # build_syn_lookup: flat needs wide; tied with wide needs flat, and says how to get the columns
    with pytest.raises(ValueError, match="flat=True adds the flat-address columns of a memory of two value words per address: it needs wide=True"):
        sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, flat=True)
    with pytest.raises(ValueError, match=r"tied=True with wide=True: the tie of a memory of two value words per address is not built \(.* need flat-address columns in the trace\): flat=True"):
        sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, tied=True, wide=True)


def _c_set(hc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))


def test_c_validator_gives_the_same_messages_and_page_flats():
    desc, blob, blob10 = _blob()
    pdesc, ported, _ = _blob("big", k=3)
    circuits = {"flat": (desc, blob, 2), "ported": (pdesc, ported, 2), "narrow": (*narrow.case("two", 1, 6, 3)[:2], 0)}
    hcs = {}
    for name, (d, b, F) in circuits.items():
        hcs[name] = hc = zhal.HostCircuit(d)
        assert zhal._lib.zkh_circuit_page_flats(hc.h) == 0
        _c_set(hc, b)
        assert zhal._lib.zkh_circuit_page_flats(hc.h) == F and zhal._lib.zkh_circuit_pages(hc.h) == 1
    wide = zhal.HostCircuit(desc)                                            # narrow / wide / flat: 0 / 0 / 2
    _c_set(wide, blob10)
    assert (zhal._lib.zkh_circuit_page_words(wide.h), zhal._lib.zkh_circuit_page_flats(wide.h)) == (2, 0)
    assert (zhal._lib.zkh_circuit_page_words(hcs["flat"].h), zhal._lib.zkh_circuit_page_words(hcs["narrow"].h)) == (2, 1)
    for name, bad, msg in _edits():
        with pytest.raises(HalError, match=r"set_arguments: not a ZKA1 \(version 1\) argument blob$" if msg is None else "set_arguments: " + msg):
            _c_set(hcs[name], bad)
        assert zhal._lib.zkh_circuit_page_flats(hcs[name].h) == circuits[name][2]                  # a refused blob leaves the arguments as they were
    with pytest.raises(HalError, match=rf"set_arguments: record 2: destination {int(desc[5])} is not a data column"):
        bad = blob.copy()
        bad[_pages_at(blob) + 7] = int(desc[5])                              # only the library knows the circuit's columns
        _c_set(hcs["flat"], bad)
    assert zhal._lib.zkh_circuit_page_flats(None) == 0


# ------------------------------------------------------------------------------------------------ the twin against the walk
@pytest.mark.parametrize("po2,zk", [(6, 3), (8, 40)])
@pytest.mark.parametrize("k", [1, 3])
def test_the_twin_writes_the_walks_flat_addresses_in_image_and_table_mode(po2, zk, k):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(fc.KINDS if k == 1 else fc.PORTED_KINDS):
        desc, blob, blob10, code, data, image = fc.case(kind, 70 * po2 + i, po2, zk, k)
        args, W = logup.Arguments.parse(blob), image.size // 2
        full, D, flat = fc.want(code, data, image, A, kind, k)
        c0, c1 = fc.flat_columns(data.shape[0])
        assert D == {"equal": 1, "distinct": A, "edges": 4}.get(kind, D) and (kind != "distinct" or D == A)
        if kind == "edges":                                                  # addresses 0 and W - 1: the lowest and the highest flat address
            assert {0, 1, 2 * W - 2, 2 * W - 1} <= {int(a) for a in flat[:, 0]}
        got = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
        assert np.array_equal(got, full), kind
        assert np.array_equal(wc.dec(got[c0, :D]), flat[0::2, 0]) and np.array_equal(wc.dec(got[c1, :D]), flat[1::2, 0])
        assert (got[[c0, c1], :D] < P).all() and not got[[c0, c1], D:A].any() and np.array_equal(got[:, A:], data[:, A:])
        if kind == "big":                                                    # the key as raw words >= P: p_addr keeps them, the flat cells never
            assert (got[args.pages.p_addr, :D] >= P).any()
        tabled = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), table=flat, image_words=image.size).reshape(-1, n)
        assert np.array_equal(tabled, full), kind
        # the version-10 blob of the same circuit leaves the two columns alone and everything else the same
        old = logup.reference_links(logup.Arguments.parse(blob10), po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
        assert np.array_equal(old[:c0], full[:c0]) and np.array_equal(old[c0:], data[c0:])


# ------------------------------------------------------------------------------------------------ the constraints
PO2, ZK = 8, 40
A_ = (1 << PO2) - ZK


@pytest.fixture(scope="module")
def tiny():
    """SYN-LOOKUP-paged-wide with flats (a closed bus), its host-made witness over a flat image of 64 words, and its accum"""
    desc, blob = sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, wide=True, flat=True)
    args = logup.Arguments.parse(blob)
    image = fc.flat_image()
    code, data, out = sl.witness(sl.TINY, PO2, ZK, seed=3, link=True, reads=True, pages=True, image=image, wide=True, flat=True)
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    accum, total = logup.reference_accumulate(logup.Arguments.parse(args.plain().blob()), PO2, ZK, code, data, mix)
    assert total == [0, 0, 0, 0]
    return {"desc": desc, "args": args, "code": code, "data": data, "out": out, "mix": mix, "accum": accum, "image": image}


def _check(t, data):
    f = check.reference_check_rows(t["desc"], PO2, t["accum"], t["code"], data, t["out"], t["mix"])
    return check.first_failure(f)


def test_the_witness_is_the_derive_and_draws_what_the_wide_witness_draws(tiny):
    n = 1 << PO2
    args, image = tiny["args"], tiny["image"]
    kw = dict(seed=3, reads=True, image=image, wide=True)
    _, bare, _ = sl.witness(sl.TINY, PO2, ZK, count=False, limbs=False, link=False, pages=False, flat=True, **kw)
    assert not bare.reshape(-1, n)[list(args.pages.flats), :A_].any()          # pages=False: the two columns are left to the library
    stages = logup.Arguments.parse(sl.build_syn_lookup(sl.TINY, derive=True, limbs=True, link=True, reads=True, pages=True, wide=True, flat=True)[1])
    assert (stages.pages.dsts, stages.pages.flats) == (args.pages.dsts, args.pages.flats)
    d = logup.reference_links(stages, PO2, ZK, tiny["code"], logup.reference_columns(stages, PO2, ZK, tiny["code"], bare), image=image)
    assert np.array_equal(logup.reference_multiplicities(stages, PO2, ZK, tiny["code"], d), tiny["data"])      # the stages make the host-made witness
    _, wide, _ = sl.witness(sl.TINY, PO2, ZK, link=True, pages=True, **kw)     # nothing new is drawn: the active rows of every shared column
    f, w = tiny["data"].reshape(-1, n), wide.reshape(-1, n)
    assert f.shape[0] == w.shape[0] + 2 and np.array_equal(f[:-2, :A_], w[:, :A_]) and sl.pages_layout(2, 4, wide=True, flat=True)[-2:] == list(args.pages.flats)


def test_check_accepts_the_honest_witness_and_names_the_row_and_the_constraint_of_each_forgery(tiny):
    n = 1 << PO2
    args = tiny["args"]
    f0, f1 = args.pages.flats
    assert _check(tiny, tiny["data"]) == (-1, check.NONE, 0)
    d = tiny["data"].reshape(-1, n)
    D = int((d[args.pages.p_on, :A_] == ONE).sum())
    assert D == 32 and D < A_
    row = 5
    # one p_flat_0 cell off by one: that row, the constraint p_on (p_flat_0 - 2 p_addr) = 0
    bad = d.copy()
    bad[f0, row] = (int(bad[f0, row]) + ONE) % P
    got_row, step0, failing = _check(tiny, bad.reshape(-1))
    assert (got_row, failing) == (row, 1)
    assert {(g, c) for g, c, back in check.explain_step(tiny["desc"], step0)["taps"]} == {(GROUP_DATA, args.pages.p_on), (GROUP_DATA, f0), (GROUP_DATA, args.pages.p_addr)}
    assert check.reference_value(tiny["desc"], PO2, tiny["accum"], tiny["code"], bad.reshape(-1), tiny["out"], tiny["mix"], row, step0) == (1, 0, 0, 0)
    # the two flat cells of one row swapped: both constraints fail on that row, the first of them named, the other by its own step
    bad = d.copy()
    bad[f0, row], bad[f1, row] = d[f1, row], d[f0, row]
    got_row, step, failing = _check(tiny, bad.reshape(-1))
    assert (got_row, step, failing) == (row, step0, 1)
    bad[f0, row] = d[f0, row]                                                # p_flat_0 put right: p_flat_1 = 2 a is named by the second constraint
    got_row, step1, failing = _check(tiny, bad.reshape(-1))
    assert (got_row, failing) == (row, 1) and step1 > step0
    assert {(g, c) for g, c, back in check.explain_step(tiny["desc"], step1)["taps"]} == {(GROUP_DATA, args.pages.p_on), (GROUP_DATA, f1), (GROUP_DATA, args.pages.p_addr)}
    assert check.reference_value(tiny["desc"], PO2, tiny["accum"], tiny["code"], bad.reshape(-1), tiny["out"], tiny["mix"], row, step1) == (P - 1, 0, 0, 0)
    # a flat cell that is not 0 on a row with p_on = 0 violates nothing: the constraint is gated by p_on ...
    bad = d.copy()
    bad[f0, D + 3] = ONE
    assert _check(tiny, bad.reshape(-1)) == (-1, check.NONE, 0)


def test_a_flat_cell_below_the_table_changes_nothing_on_the_bus_and_the_derive_never_writes_one():
    """Both halves of the answer: every term that reads p_flat_j has the multiplicity p_on, so with p_on = 0 the cell adds nothing to any
    accum column or to the open total; and the derive writes 0 there (the twin, against the walk, above)"""
    s = fc.segment()
    n = 1 << fc.SEG_PO2
    args = s["args"]
    reads = [t for t in args.terms if any((GROUP_DATA, c) in t.tuple_cols for c in args.pages.flats)]
    assert len(reads) == 2 and all(t.mult == (GROUP_DATA, args.pages.p_on) and t.tag == logup.TIE_TAG for t in reads)
    accum, total = fc.segment_total()
    d = s["data"].reshape(-1, n).copy()
    D = len(s["table"]) // 2
    assert not d[list(args.pages.flats), D:n - fc.SEG_ZK].any()
    d[args.pages.flats[0], D + 3], d[args.pages.flats[1], D + 7] = ONE, 12345
    accum2, total2 = logup.reference_accumulate(args, fc.SEG_PO2, fc.SEG_ZK, s["code"], d.reshape(-1), fc.CHALLENGE)
    assert np.array_equal(accum2, accum) and np.array_equal(fc.tied_cases.enc(total2), total)
