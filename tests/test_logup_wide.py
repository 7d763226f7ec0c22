"""WIDE paging on the CPU (ZKA1 version 10, zeth_amd/circuits/logup.py): a paged memory of two value words per address.  The format and its
rules, in Python and in csrc/arguments.hip message for message; the blobs of every earlier builder call byte for byte
(tests/golden/syn_lookup_blobs.json through its own maker) and the wide builder calls pinned (tests/golden/syn_lookup_wide_blobs.json); the numpy
twin `reference_links` against an independent dictionary walk (wide_cases.walk) in image and table mode and with ports;
`reference_page_out` and a second segment against one walk over both; `reference_page_out_proof`, whose table is the FLAT one, walked by
`check_page_out_proof` from root_before to the root of a fresh commit of the new image; the refusals of a wide circuit by what ties a segment to
its page-out.  No GPU.

The cases keep three conditions (wide_cases.check_conditions, asserted here against the walk alone): the two halves of every image address differ,
at least a quarter of the first accesses are loads answered by an image address whose two words are both non-zero, and in `big` at least a
sixth of the image's words are >= P."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import pages_cases as narrow
import wide_cases as wc
from zeth_amd import hal as zhal, page_seal
from zeth_amd.circuits import logup, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_DATA
from zeth_amd.hal import HalError

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen, gen_wide = _load("make_golden_syn_lookup_blobs"), _load("make_golden_syn_lookup_wide_blobs")
P, ONE = wc.P, wc.ONE
H = logup.ARGS_HEADER
WIDE7 = logup.PAGES_BIT | logup.WIDE_BIT


def _blob(kind="two", k=1):
    desc, blob, *_ = wc.case(kind, 1, 6, 3, k=k)
    return desc, blob


def _pages_at(blob):
    """the first word of the PAGES record: the last 32 words"""
    return blob.size - 32


# ------------------------------------------------------------------------------------------------ the format
def test_version_10_round_trips():
    desc, blob = _blob()
    a = logup.Arguments.parse(blob)
    assert a.version == 10 and blob[1] == 10 and blob[7] == 1 | WIDE7 and a.wide and np.array_equal(a.blob(), blob)
    at = _pages_at(blob)
    assert list(blob[at:at + 16]) == [4, 8, 3, 0, 1] + [0] * 11                                  # word 4 holds V - 1
    assert list(blob[at + 16:]) == list(range(wc.PER, wc.PER + 13)) + [0] * 3                  # 3 + 2 V + 2 ng destinations
    pg = a.pages
    assert pg.nv == 2 and (pg.p_on, pg.p_addr, pg.p_ins, pg.p_outs, pg.p_time) == (13, 14, (15, 16), (17, 18), 19)
    assert pg.alimbs == (20, 21, 22) and pg.gaps == (23, 24, 25) and a.records[0].nc == 3
    # V = 2 and ng = 4 take 15 of the 16 destination slots
    b = logup.LogupBuilder((4, 4, 40), (4, 8))
    b.term(0, [(GROUP_DATA, 39)])
    link = b.derive_links(None, (GROUP_DATA, 0), [(GROUP_DATA, 1), (GROUP_DATA, 2), (GROUP_DATA, 3)], list(range(5, 13)), 7, write=(GROUP_DATA, 4))
    rec = b.derive_pages(link, list(range(13, 28)), 7)
    assert rec.ng == 4 and rec.nv == 2 and rec.n_dsts() == 15 and logup.Arguments.parse(b.args().blob()).pages == rec
    # with ports: every port carries nc = 3, and bit 18 stands beside bit 19
    _, ported = _blob("range5", k=3)
    ap = logup.Arguments.parse(ported)
    assert ap.version == 10 and ported[7] == 3 | WIDE7 | logup.PORTS_BIT and [r.joins for r in ap.records[:3]] == [None, 0, 0] and ap.pages.link == 0
    assert np.array_equal(ap.blob(), ported)
    # nothing about V = 1 moves: a narrow paged blob is the version-7 blob it was, word 4 of its PAGES record 0
    _, old, *_ = narrow.case("two", 1, 6, 3)
    assert old[1] == 7 and old[7] == 0x10001 and old[_pages_at(old) + 4] == 0 and logup.Arguments.parse(old).pages.nv == 1


def _narrow_as_10():
    """a narrow paged blob marked version 10 with bit 19"""
    _, old, *_ = narrow.case("two", 1, 6, 3)
    bad = old.copy()
    bad[1], bad[7] = 10, int(old[7]) | logup.WIDE_BIT
    return bad


def _edits():
    """[(the case whose circuit the blob is of, the blob, the message after 'ZKA1: ' / 'set_arguments: ')], every rule of the wide format once;
    None: no ZKA1 blob"""
    _, blob = _blob()
    _, ported = _blob("range5", k=3)
    narrow10 = _narrow_as_10()
    at, nat, out = _pages_at(blob), _pages_at(narrow10), []

    def edited(src, *edits):
        bad = src.copy()
        for w, v in edits:
            bad[w] = v
        return bad
    no_wide_record = r"header word 7 has bit 19 \(WIDE\), but no PAGES record pages two value words per address"
    reserved = r"record 2: a reserved word of a PAGES record is not 0 \(words 5\.\.15 and the unused destination words\)"
    no_target = r"record 2: a PAGES record of two value words per address pages record {}, which is no LINK record with READS and three carried columns \(a clock and two values\)"
    out.append(("wide", edited(blob, (7, 1 | logup.PAGES_BIT)), None))                           # version 10 without bit 19
    out.append(("wide", edited(blob, (1, 9)), None))                                             # version 9 without bit 18
    out.append(("wide", edited(blob, (1, 7)), "header word 7 is 524289, the blob has 1 LINK records with READS"))    # bit 19 means nothing before version 10
    out.append(("narrow", narrow10, no_wide_record))                                             # bit 19 with V = 1
    out.append(("wide", edited(blob, (at + 4, 0)), no_wide_record))
    out.append(("wide", edited(blob, (at + 4, 2)), r"record 2: word 4 of a PAGES record is 2 \(V - 1: 0 = one value word per address, 1 = two\)"))
    out.append(("wide", edited(blob, (at + 5, 7)), reserved))
    out.append(("wide", edited(blob, (at + 31, 7)), reserved))
    out.append(("narrow", edited(narrow10, (nat + 4, 1), (nat + 27, 40), (nat + 28, 41)), no_target.format(0)))     # V - 1 is not the LINK's nc - 2
    out.append(("wide", edited(blob, (at + 3, 1)), no_target.format(1)))                         # the LINK that is not paged: no READS, two carried columns
    out.append(("ported", edited(ported, (7, 3 | WIDE7)), r"a LINK record joins, but header word 7 lacks bit 18 \(PORTS\)"))
    out.append(("wide", edited(blob, (7, 1 | WIDE7 | logup.PORTS_BIT)), r"header word 7 has bit 18 \(PORTS\), but no LINK record joins"))
    out.append(("wide", edited(blob, (at + 16 + 3, 15)), r"record 2: its destination \(data 15\) appears twice"))                  # p_in_1 = p_in_0
    out.append(("wide", edited(blob, (at + 16 + 5, 2)), r"record 0: its source \(data 2\) is a destination of record 2 \(records never chain\)"))   # p_out_1 = a value column
    return out


def test_parser_refuses_every_rule():
    for _, bad, msg in _edits():
        with pytest.raises(ValueError, match="^not a ZKA1 argument blob$" if msg is None else "^ZKA1: " + msg):
            logup.Arguments.parse(bad)
    # a V = 1 record that names a LINK of two values is what every version refused: the text it always had
    _, blob = _blob()
    a = logup.Arguments.parse(blob)
    old = logup.Arguments(a.k, a.alpha, a.beta, a.terms, a.records[:2] + [logup.Pages(8, 3, 0, a.pages.dsts[:11])]).blob()
    assert old[1] == 7
    with pytest.raises(ValueError, match=r"^ZKA1: record 2: a PAGES record pages record 0, which is no LINK record with READS and two carried columns \(a clock and one value\)$"):
        logup.Arguments.parse(old)


def test_builder_rules():
    b = logup.LogupBuilder((4, 4, 40), (4, 8))
    b.term(0, [(GROUP_DATA, 39)])
    link = b.derive_links(None, (GROUP_DATA, 0), [(GROUP_DATA, 1), (GROUP_DATA, 2), (GROUP_DATA, 3)], list(range(5, 13)), 8, write=(GROUP_DATA, 4))
    with pytest.raises(ValueError, match=r"derive_pages: 12 destinations \(7 \+ 2 ng for a LINK that carries two values: .*; 5 \+ 2 ng for one value\)"):
        b.derive_pages(link, list(range(13, 25)), 8)                                             # an even count: no 7 + 2 ng
    assert b.args().version == 6
    rec = b.derive_pages(link, list(range(13, 26)), 8)
    assert b.args().version == 10 and rec.nv == 2
    # the ownership rule covers the new destinations: of them only p_on may be a multiplicity
    for col, name in ((rec.p_ins[1], "p_in_1"), (rec.p_outs[0], "p_out_0"), (rec.p_outs[1], "p_out_1"), (rec.p_time, "p_time")):
        with pytest.raises(ValueError, match=rf"record 1: its destination \(data {col}\) is the multiplicity of term 1 \(of a PAGES record's destinations only p_on may be\)"):
            b.term(0, [(GROUP_DATA, 38)], sign=-1, mult=(GROUP_DATA, col))
    b.term(0, [(GROUP_DATA, 38)], sign=-1, mult=(GROUP_DATA, rec.p_on))
    assert len(b.terms) == 2


def _c_set(hc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))


def test_c_validator_gives_the_same_messages_and_page_words():
    circuits = {"wide": (_blob(), 2), "ported": (_blob("range5", k=3), 2), "narrow": (narrow.case("two", 1, 6, 3)[:2], 1)}
    hcs = {}
    for name, ((desc, blob), V) in circuits.items():
        hcs[name] = hc = zhal.HostCircuit(desc)
        assert zhal._lib.zkh_circuit_page_words(hc.h) == 0
        _c_set(hc, blob)
        assert zhal._lib.zkh_circuit_page_words(hc.h) == V and zhal._lib.zkh_circuit_pages(hc.h) == 1
    for name, bad, msg in _edits():
        with pytest.raises(HalError, match=r"set_arguments: not a ZKA1 \(version 1\) argument blob$" if msg is None else "set_arguments: " + msg):
            _c_set(hcs[name], bad)
        assert zhal._lib.zkh_circuit_page_words(hcs[name].h) == circuits[name][1]                  # a refused blob leaves the arguments as they were
    (desc, blob), _ = circuits["wide"]
    a = logup.Arguments.parse(blob)
    old = logup.Arguments(a.k, a.alpha, a.beta, a.terms, a.records[:2] + [logup.Pages(8, 3, 0, a.pages.dsts[:11])]).blob()
    with pytest.raises(HalError, match=r"set_arguments: record 2: a PAGES record pages record 0, which is no LINK record with READS and two carried columns \(a clock and one value\)$"):
        _c_set(hcs["wide"], old)


# ------------------------------------------------------------------------------------------------ the builders
def test_every_earlier_builder_blob_is_reproduced_unchanged():
    with open(gen.PATH) as fh:
        assert gen.record() == json.load(fh)


def test_the_wide_builder_calls_are_pinned():
    with open(gen_wide.PATH) as fh:
        assert gen_wide.record() == json.load(fh)
    for shape, kw, *_ in gen_wide.record():
        desc, blob = sl.build_syn_lookup(getattr(sl, shape), **kw)
        a = logup.Arguments.parse(blob)
        assert a.version == 10 and a.wide and int(blob[7]) & logup.WIDE_BIT and bool(int(blob[7]) & logup.PORTS_BIT) == bool(kw.get("ports"))
        narrow_kw = {k: v for k, v in kw.items() if k != "wide"}
        ndesc, nblob = sl.build_syn_lookup(getattr(sl, shape), **narrow_kw)
        assert int(nblob[1]) in (7, 9) and len(a.terms) == len(logup.Arguments.parse(nblob).terms)
        widths = sorted(len(t.tuple_cols) for t in a.terms if t.tag == 1)
        assert widths[-1] == 4 and widths.count(3) == 1                                          # (addr, v0, v1, time); the page-in's (p_addr, p_in_0, p_in_1)


def test_the_wide_witness_balances_and_shares_its_addresses_with_the_narrow_one():
    po2, zk, W = 8, 40, 64
    n, A = 1 << po2, (1 << po2) - zk
    for shape, ports in ((sl.TINY, False), (sl.MULTI, True)):
        desc, blob = sl.build_syn_lookup(shape, derive=True, limbs=True, link=True, reads=True, pages=True, wide=True, ports=ports)
        args = logup.Arguments.parse(blob)
        image = np.random.default_rng(3).integers(1, P, 2 * W, dtype=np.uint64).astype(np.uint32)
        kw = dict(seed=5, addr_range=W, reads=True, image=image, wide=True, ports=ports)
        code, full, _ = sl.witness(shape, po2, zk, link=True, pages=True, **kw)
        _, bare, _ = sl.witness(shape, po2, zk, count=False, limbs=False, link=False, pages=False, **kw)
        d = logup.reference_links(args, po2, zk, code, logup.reference_columns(args, po2, zk, code, bare), image=image)
        assert np.array_equal(logup.reference_multiplicities(args, po2, zk, code, d), full)      # the stages make the host-made witness
        mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
        assert logup.reference_accumulate(logup.Arguments.parse(args.plain().blob()), po2, zk, code, full, mix)[1] == [0, 0, 0, 0]
        _, one, _ = sl.witness(shape, po2, zk, link=True, pages=True, seed=5, addr_range=W, reads=True, image=image[:W], ports=ports)
        l1, l2 = sl.link_layout(shape.n_words, shape.n_limbs, shape.n_mem)[0], sl.link_layout(shape.n_words, shape.n_limbs, shape.n_mem, wide=True)[0]
        f1, f2 = one.reshape(-1, n), full.reshape(-1, n)
        assert np.array_equal(f1[l1[0], :A], f2[l2[0], :A]) and np.array_equal(f1[l1[2], :A], f2[l2[2], :A])     # the same addresses and clocks


# ------------------------------------------------------------------------------------------------ the twin against the walk
def _want(code, data, image, A, kind, k=1, memory=None):
    out, mem, flat = wc.walk(code, data, image, A, kind, memory=memory, k=k)
    want = data.copy()
    for c, v in out.items():
        want[c, :A] = v
    return want, mem, flat


@pytest.mark.parametrize("po2,zk", [(6, 3), (8, 40)])
def test_the_twin_equals_the_walk_in_image_and_table_mode(po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(wc.KINDS):
        desc, blob, code, data, image = wc.case(kind, 70 * po2 + i, po2, zk)
        firsts = wc.check_conditions(kind, code, data, image, A)
        args = logup.Arguments.parse(blob)
        got = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
        want, mem, flat = _want(code, data, image, A, kind)
        if kind == "two":                                                    # the record that is not paged is what it is alone
            alone = logup.Arguments(args.k, args.alpha, args.beta, args.terms, [args.records[1]])
            s = wc.table_base() + wc.TABLE_W + 3
            want[s:s + 7] = logup.reference_links(alone, po2, zk, code.reshape(-1), data.reshape(-1)).reshape(-1, n)[s:s + 7]
        assert np.array_equal(got, want), kind
        assert len(mem) == firsts == {"equal": 1, "distinct": A, "range5": 5, "edges": 4}.get(kind, firsts) and flat.shape == (2 * firsts, 3)
        assert (np.diff(flat[:, 0].astype(np.int64)) > 0).all()             # i major, j minor: strictly increasing flat addresses
        tabled = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), table=flat, image_words=image.size).reshape(-1, n)
        assert np.array_equal(tabled, want), kind


def test_the_twin_equals_the_walk_with_ports():
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(["range5", "big", "edges"]):
        desc, blob, code, data, image = wc.case(kind, 11 + i, po2, zk, k=3)
        wc.check_conditions(kind, code, data, image, A, k=3)
        args = logup.Arguments.parse(blob)
        assert args.ports and args.wide
        want, mem, flat = _want(code, data, image, A, kind, k=3)
        got = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
        assert np.array_equal(got, want), kind
        tabled = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), table=flat, image_words=image.size).reshape(-1, n)
        assert np.array_equal(tabled, want), kind
        # p_out_j is the TAIL access's own record's: some address is first touched through one port and last through another
        acc = wc.accesses(code, data, A, kind, 3)
        first, last = {}, {}
        for r, q in acc:
            a = int(wc.dec(data[wc.PER * q + wc.KEY, r]))
            first.setdefault(a, q)
            last[a] = q
        assert any(first[a] != last[a] for a in first)


def test_page_out_and_a_second_segment_equal_one_walk_over_both():
    po2, zk, kind = 8, 40, "big"
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code1, data1, image0 = wc.case(kind, 31, po2, zk)
    args = logup.Arguments.parse(blob)
    full1 = logup.reference_links(args, po2, zk, code1.reshape(-1), data1.reshape(-1), image=image0)
    image1 = logup.reference_page_out(args, po2, zk, full1, image0)
    assert not np.array_equal(image1, image0) and image1.size == image0.size
    _, _, code2, data2, image1b = wc.case(kind, 31, po2, zk, image=image1, trace_seed=32)
    full2 = logup.reference_links(args, po2, zk, code2.reshape(-1), data2.reshape(-1), image=image1b)
    image2 = logup.reference_page_out(args, po2, zk, full2, image1b)
    _, mem1, _ = wc.walk(code1, data1, image0, A, kind)
    out2, mem2, _ = wc.walk(code2, data2, image0, A, kind, memory=mem1)
    f2 = full2.reshape(-1, n)
    for col, v in out2.items():
        assert np.array_equal(f2[col, :A] % P, v % P), col
    assert set(mem1) & set(mem2)
    final = image0.copy()
    for a, (v0, v1) in list(mem1.items()) + list(mem2.items()):
        final[2 * a], final[2 * a + 1] = v0, v1
    assert np.array_equal(image2 % P, final % P)


@pytest.mark.parametrize("kind,k", [("sparse", 1), ("big", 1), ("range5", 3)])
def test_the_proofs_table_is_the_flat_one_and_walks_to_the_new_root(kind, k):
    po2, zk = 8, 40
    A = (1 << po2) - zk
    desc, blob, code, data, image = wc.case(kind, 5, po2, zk, k=k)
    args = logup.Arguments.parse(blob)
    full = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image)
    nodes = logup.reference_image_tree(image)
    proof = logup.reference_page_out_proof(args, po2, zk, full, image.size, nodes)
    _, mem, flat = wc.walk(code, data, image, A, kind, k=k)
    D, h = len(mem), int(proof[4])
    assert int(proof[1]) == image.size and int(proof[2]) == 2 * D                                # (V W, V D)
    table = proof[5 + h:5 + h + 6 * D].reshape(-1, 3)
    assert np.array_equal(table[:, 0], flat[:, 0]) and np.array_equal(table[:, 1:], flat[:, 1:] % np.uint32(P))
    assert proof.size <= logup.image_proof_words(image.size, 2 * D)
    after = logup.reference_page_out(args, po2, zk, full, image)
    assert np.array_equal(logup.check_page_out_proof(proof, nodes[1]), logup.reference_image_root(after))
    # the fourth rule names the word: p_in_1 forged on one row, then p_in_0 as well (the lowest j first)
    n = 1 << po2
    bad = full.reshape(-1, n).copy()
    pg = args.pages
    row = D // 2
    a = int(wc.dec(bad[pg.p_addr, row]))
    bad[pg.p_ins[1], row] = wc.enc(int(wc.dec(image[2 * a + 1])) + 1)
    with pytest.raises(logup.ReferenceError, match=rf"record {k} at row {row}: p_in word 1 {(int(wc.dec(image[2 * a + 1])) + 1) % P} at address {a}, the tree holds {int(wc.dec(image[2 * a + 1]))}$"):
        logup.reference_page_out_proof(args, po2, zk, bad.reshape(-1), image.size, nodes)
    bad[pg.p_ins[0], row] = wc.enc(int(wc.dec(image[2 * a])) + 1)
    with pytest.raises(logup.ReferenceError, match=rf"record {k} at row {row}: p_in word 0 "):
        logup.reference_page_out_proof(args, po2, zk, bad.reshape(-1), image.size, nodes)


def test_the_twins_refusals():
    po2, zk = 8, 40
    desc, blob, code, data, image = wc.case("two", 21, po2, zk)
    args = logup.Arguments.parse(blob)
    flat = lambda d: d.reshape(-1)
    with pytest.raises(logup.ReferenceError, match="^an image of 1999 words is not a whole number of addresses of 2 value words$"):
        logup.reference_links(args, po2, zk, flat(code), flat(data), image=image[:-1])
    with pytest.raises(logup.ReferenceError, match="^an image of 1999 words is not a whole number of addresses of 2 value words$"):
        logup.reference_page_out(args, po2, zk, flat(data), image[:-1])
    with pytest.raises(logup.ReferenceError, match="address 50 outside the image of 50 words"):  # W is counted in addresses
        d = data.copy()
        d[wc.KEY, 0] = wc.enc(50)
        logup.reference_links(args, po2, zk, flat(code), flat(d), image=image[:100])


# ------------------------------------------------------------------------------------------------ what is left out
class _WideCircuit:
    def page_words(self):
        return 2


class _WideProver:
    circuit, hal = _WideCircuit(), None


def test_the_tie_of_a_wide_memory_is_refused_before_anything_is_sealed():
    with pytest.raises(ValueError, match="tied=True with wide=True: the tie of a memory of two value words per address is not built"):
        sl.build_syn_lookup(sl.TINY, link=True, reads=True, pages=True, tied=True, wide=True)
    with pytest.raises(ValueError, match="wide=True gives the paged memory two value words per address: it needs pages=True"):
        sl.build_syn_lookup(sl.TINY, link=True, reads=True, wide=True)
    sp = _WideProver()                                                       # its hal is None: a call that went on would fail on it, not with this sentence
    msg = "{}: the segment's memory holds 2 value words per address \\(ZKA1 version 10\\): the tie of a wide memory is not built"
    with pytest.raises(HalError, match=msg.format("seal_tied")):
        page_seal.seal_tied(sp, None, None, None, None, None, [], None, 0, None, None)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree")):
        page_seal.seal_tied_tree(sp, None, None, None, None, None, [], None, 0, None, None)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree_from_proof")):
        page_seal.seal_tied_tree_from_proof(sp, None, None, None, None, None, [], None, None)
    with pytest.raises(HalError, match=msg.format("preflight_paged_run")):
        page_seal.preflight_paged_run(sp, [], [], None, None)
    step = page_seal.PagedStep(None, None, None, None, None, None)
    with pytest.raises(HalError, match=msg.format("seal_tied_tree_from_proof")):
        page_seal.seal_paged_step(step, sp, None, None, [])
