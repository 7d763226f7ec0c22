"""PORTS on the CPU (ZKA1 version 9, zeth_amd/circuits/logup.py): a LINK record that joins the memory of a head.  The format and its rules, in
Python and in csrc/arguments.hip message for message; the blobs of every earlier builder call byte for byte (tests/golden/syn_lookup_blobs.json,
recorded on the commit before); SYN-LOOKUP-reads-ported's description, which is SYN-LOOKUP-reads'; the numpy twin `reference_links` against the
host's sequential walk over (row, port), plain and paged (image and table modes); and the refusals of the twin.  No GPU.

The ported witness under the version-6 blob of separate memories must be refused by the read rule exactly when some load reads what another
port left: at addresses below 8 that happens in every trace, at addresses below 2^20 it is decided from the witness, not assumed."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import ports_cases as pc
from zeth_amd import hal as zhal
from zeth_amd.circuits import check, logup, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_syn_lookup_blobs", os.path.join(HERE, "golden", "make_golden_syn_lookup_blobs.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
P, ONE, MULTI = pc.P, pc.ONE, pc.MULTI
H = logup.ARGS_HEADER


# ------------------------------------------------------------------------------------------------ the format
def _base(tied=False):
    """-> (builder, desc, blob): records 0 LIMBS, 1 a head, 2 and 3 its joiners, 4 a LINK of its own, 5 the PAGES record of the head (, 6 OPEN)"""
    b = logup.LogupBuilder((4, 6, 60), (16, 8), alpha=4, beta=8, open_bus=(2, 12)) if tied else logup.LogupBuilder((4, 6, 60), (4, 8))
    b.term(0, [(GROUP_DATA, 0)], tag=2 if tied else 1)
    link = lambda base, **kw: b.derive_links(3, (GROUP_DATA, base), [(GROUP_DATA, base + 1), (GROUP_DATA, base + 2)], list(range(base + 4, base + 11)), 8,
                                             write=(GROUP_DATA, base + 3), **kw)
    head = link(1)
    link(12, joins=head)
    b.derive_links(None, (GROUP_DATA, 34), [(GROUP_DATA, 35)], [36, 37, 38], 4)
    link(23, joins=head)                                                     # it goes after the memory's last port, before the LINK of its own
    b.derive_pages(head, list(range(40, 51)), 8)
    b.derive_limbs((GROUP_CODE, 2), [52, 53], 16)                            # ... and this one before all of them: every index moves by one
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0)))
    return b, desc, blob


def _at(blob, record):
    """the first word of record `record` of _base's blob (one term, one 16-word LIMBS record, then 32-word records)"""
    return H + 16 * int(blob[5]) + 16 + 32 * (record - 1)


def test_version_9_round_trips_and_the_builder_keeps_a_memory_one_run():
    b, desc, blob = _base()
    a = logup.Arguments.parse(blob)
    assert a.version == 9 and blob[1] == 9 and blob[7] == 3 | logup.PAGES_BIT | logup.PORTS_BIT and np.array_equal(a.blob(), blob)
    assert [type(r).__name__ for r in a.records] == ["Record", "Link", "Link", "Link", "Link", "Pages"]
    assert [r.joins for r in a.records[1:5]] == [None, 1, 1, None] and a.pages.link == 1
    assert [r.key[1] for r in a.records[1:5]] == [1, 12, 23, 34]
    assert logup.memory_ports(a.records, 1) == [1, 2, 3] and logup.memory_ports(a.records, 4) == [4]
    for rec in (2, 3):
        at = _at(blob, rec)
        assert blob[at + 5] == 3 and blob[at + 31] == 1                      # READS | JOINS, and the head in word 31
    assert blob[_at(blob, 1) + 5] == 1 and blob[_at(blob, 1) + 31] == 0
    assert all(b.paged(r) == a.pages for r in b.records[1:4]) and b.paged(b.records[4]) is None     # every port of the paged memory
    _, _, tied = _base(tied=True)
    t = logup.Arguments.parse(tied)
    assert t.version == 9 and tied[7] == 3 | logup.PAGES_BIT | logup.OPEN_BIT | logup.PORTS_BIT and np.array_equal(t.blob(), tied)
    # without a joiner the builder writes what it wrote: the version is the highest feature in use
    assert [int(sl.build_syn_lookup(sl.TINY, link=True, reads=True, **kw)[1][1]) for kw in ({}, {"pages": True}, {"pages": True, "tied": True})] == [6, 7, 8]
    assert int(sl.build_syn_lookup(sl.TINY, link=True, reads=True, ports=True)[1][1]) == 6      # one pair: nothing joins


def test_every_earlier_builder_call_gives_the_blob_it_gave():
    with open(gen.PATH) as fh:
        recorded = json.load(fh)
    assert len(recorded) == len(gen.CALLS) == 49 and sorted({r[4] for r in recorded}) == [1, 2, 3, 4, 5, 6, 7, 8]
    assert gen.record() == recorded


def _messages(desc, blob):
    """-> (the Python message: the parser's, else the rules' with the circuit's widths; the message of zkh_circuit_set_arguments)"""
    hc = zhal.HostCircuit(desc)
    py = c_msg = None
    try:
        a = logup.Arguments.parse(blob)
        py = logup.check_sorted(a.terms) or logup.check_derived(a.terms) or logup._check_records(a.terms, a.records, (4, 6, 60))
    except ValueError as e:
        py = str(e)
    try:
        zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(blob), blob.size))
    except zhal.HalError as e:
        c_msg = str(e)
    return py, c_msg


def _edited(blob, edits):
    out = blob.copy()
    for w, v in edits:
        out[w] = v
    return out


def _rule_cases():
    _, desc, blob = _base()
    r = lambda rec, word: _at(blob, rec) + word
    unjoin = lambda rec: [(r(rec, 5), 1), (r(rec, 31), 0)]
    cases = [
        ("joins a joiner", [(r(3, 31), 2)], "record 3: a LINK joins record 2, which is no LINK record without JOINS before it (a port joins the head of its memory)"),
        ("joins a LIMBS record", [(r(2, 31), 0)], "record 2: a LINK joins record 0, which is no LINK record without JOINS before it (a port joins the head of its memory)"),
        ("joins itself", [(r(2, 31), 2)], "record 2: a LINK joins record 2, which is no LINK record without JOINS before it (a port joins the head of its memory)"),
        ("joins a later record", [(r(3, 31), 4)], "record 3: a LINK joins record 4, which is no LINK record without JOINS before it (a port joins the head of its memory)"),
        ("a record between does not join", unjoin(2), "record 3: a LINK joins record 1, but record 2 between them does not (a memory is a run of consecutive LINK records)"),
        ("another L", [(r(2, 1), 7)], "record 2: a LINK joins record 1 with another nc, L, nl or READS (the ports of a memory have their head's)"),
        ("no READS", [(r(3, 5), 2), (r(3, 14), 0), (r(3, 15), 0), (7, 2 | logup.PAGES_BIT | logup.PORTS_BIT)],
         "record 3: a LINK joins record 1 with another nc, L, nl or READS (the ports of a memory have their head's)"),
        ("the PAGES record names a joiner", [(r(5, 3), 2)], "record 5: a PAGES record pages record 2, which joins record 1 (a PAGES record names the head of a memory)"),
        ("word 5 bit 2", [(r(2, 5), 7)], "record 2: word 5 of a LINK is 0x7 (bit 0: READS, the read rule; bit 1: JOINS, a port of its head's memory; the other bits are reserved)"),
        ("word 31 without JOINS", [(r(4, 31), 1)],
         "record 4: a reserved word of a LINK is not 0 (words 5, 14, 15, the unused carried pairs and the unused destination words)"),
        ("bit 18 and no joiner", unjoin(2) + unjoin(3), "header word 7 has bit 18 (PORTS), but no LINK record joins"),
        ("bit 17 and no OPEN record", [(7, int(blob[7]) | logup.OPEN_BIT)], "header word 7 has bit 17 (OPEN), but the blob has no OPEN record"),
        ("no bit 16 and a PAGES record", [(7, int(blob[7]) ^ logup.PAGES_BIT)], "the blob has a PAGES record, but header word 7 lacks bit 16 (PAGES)"),
    ]
    return desc, blob, cases


def test_the_rules_refuse_with_one_text_in_python_and_in_the_c_decoder():
    desc, blob, cases = _rule_cases()
    assert _messages(desc, blob) == (None, None)
    for what, edits, want in cases:
        py, c_msg = _messages(desc, _edited(blob, edits))
        assert py in (want, "ZKA1: " + want), (what, py)
        assert c_msg == "set_arguments: " + want, (what, c_msg)
    # an OPEN record without bit 17 (version 9 no longer implies it)
    _, tdesc, tied = _base(tied=True)
    assert _messages(tdesc, tied) == (None, None)
    py, c_msg = _messages(tdesc, _edited(tied, [(7, int(tied[7]) ^ logup.OPEN_BIT)]))
    assert py == "ZKA1: the blob has an OPEN record, but header word 7 lacks bit 17 (OPEN)" and c_msg == "set_arguments: " + py[6:]
    # version 9 without bit 18 is no ZKA1 blob, and so is JOINS in a blob of an earlier version: word 5 keeps its text there
    for edits in ([(7, int(blob[7]) ^ logup.PORTS_BIT)], [(1, 9)]):
        src = blob if edits[0][0] == 7 else sl.build_syn_lookup(sl.TINY, link=True, reads=True)[1]
        with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
            logup.Arguments.parse(_edited(src, edits))
    assert _messages(desc, _edited(blob, [(7, int(blob[7]) ^ logup.PORTS_BIT)]))[1] == "set_arguments: not a ZKA1 (version 1) argument blob"
    d6, b6 = sl.build_syn_lookup(MULTI, link=True, reads=True)
    at = H + 16 * int(b6[5]) + 32
    old = "record 1: word 5 of a LINK is 0x3 (bit 0: READS, the read rule; the other bits are reserved)"
    with pytest.raises(ValueError, match="^" + re.escape("ZKA1: " + old) + "$"):
        logup.Arguments.parse(_edited(b6, [(at + 5, 3), (at + 31, 0)]))
    hc = zhal.HostCircuit(d6)
    with pytest.raises(zhal.HalError, match="^" + re.escape("set_arguments: " + old) + "$"):
        bad = _edited(b6, [(at + 5, 3), (at + 31, 0)])
        zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(bad), bad.size))


def test_a_memory_has_at_most_eight_records():
    b = logup.LogupBuilder((4, 6, 12 * 9 + 1), (4, 8))
    b.term(0, [(GROUP_DATA, 0)], tag=1)
    link = lambda q, **kw: b.derive_links(None, (GROUP_DATA, 1 + 12 * q), [(GROUP_DATA, 2 + 12 * q)], [3 + 12 * q, 4 + 12 * q, 5 + 12 * q], 4, **kw)
    head = link(0)
    for q in range(1, logup.MAX_PORTS):
        link(q, joins=head)
    want = "record 8: port 8 of the memory of record 0 (a memory has at most 8 records)"
    with pytest.raises(ValueError, match="^" + re.escape(want) + "$"):
        link(8, joins=head)
    assert len(b.records) == 8
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0)))
    ninth = logup.Link(None, (GROUP_DATA, 97), ((GROUP_DATA, 98),), 4, 0, (99, 100, 101), joins=0)
    a = logup.Arguments.parse(blob)
    long = logup.Arguments(a.k, a.alpha, a.beta, a.terms, a.records + [ninth]).blob()
    py, c_msg = _messages(desc, long)
    assert py == "ZKA1: " + want and c_msg == "set_arguments: " + want
    with pytest.raises(ValueError, match="not one of this builder's"):
        link(8, joins=ninth)


# ------------------------------------------------------------------------------------------------ the description
@pytest.mark.parametrize("shape", [sl.TINY, MULTI], ids=["TINY", "MULTI"])
def test_the_ported_description_is_the_unported_one(shape):
    for kw in ({}, {"derive": True, "limbs": True}):
        desc, blob = sl.build_syn_lookup(shape, link=True, reads=True, **kw)
        pdesc, pblob = sl.build_syn_lookup(shape, link=True, reads=True, ports=True, **kw)
        assert np.array_equal(desc, pdesc)
        assert np.array_equal(blob, pblob) == (shape.n_mem == 1)
    with pytest.raises(ValueError, match="ports=True makes the memory pairs the ports of one memory"):
        sl.build_syn_lookup(shape, link=True, ports=True)
    with pytest.raises(ValueError, match="pages=True pages one memory: n_mem is 3"):
        sl.build_syn_lookup(MULTI, link=True, reads=True, pages=True)


# ------------------------------------------------------------------------------------------------ the twin against the walk
@pytest.mark.parametrize("po2,zk,addr_range", pc.SYN)
def test_the_twin_derives_the_host_made_ported_witness(po2, zk, addr_range):
    s = pc.syn(po2, zk, addr_range)
    args = s["args"]
    assert args.version == 9 and np.array_equal(s["desc"], s["same"]) and logup.Arguments.parse(s["apart"]).version == 6
    got = logup.reference_multiplicities(args, po2, zk, s["code"], logup.reference_links(args, po2, zk, s["code"], logup.reference_columns(args, po2, zk, s["code"], s["bare"])))
    assert np.array_equal(got, s["full"])
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    accum, total = logup.reference_accumulate(args, po2, zk, s["code"], s["full"], mix)
    assert total == [0, 0, 0, 0]
    assert (check.reference_check_rows(s["desc"], po2, accum, s["code"], s["full"], s["out"], mix, 0, (1 << po2) - zk) == check.NONE).all()
    # the same traces as three memories that know nothing of each other: a load that reads another port's store is a misread there
    acc = pc.accesses(s["full"], po2, zk)
    seen, crossed = {}, False
    for r, q, a, store, *_ in acc:
        crossed |= not store and a in seen and seen[a] != q
        seen[a] = q
    assert crossed or addr_range > 8
    apart = logup.Arguments.parse(s["apart"])
    if crossed:
        with pytest.raises(logup.ReferenceError, match=r"^record \d at row \d+: a load of carried column 1 returns \d+, but "):
            logup.reference_links(apart, po2, zk, s["code"], s["bare"])
    else:
        logup.reference_links(apart, po2, zk, s["code"], s["bare"])


def test_the_direct_cases_are_version_9_and_the_twin_takes_them():
    for kind, (po2, zk, memories) in pc.DIRECT.items():
        desc, blob, code, data, _, _ = pc.direct(kind)
        args = logup.Arguments.parse(blob)
        links = [i for i, r in enumerate(args.records) if isinstance(r, logup.Link)]
        assert args.version == 9 and len(links) == sum(memories)
        heads = [i for i in links if args.records[i].joins is None]
        assert [len(logup.memory_ports(args.records, h)) for h in heads] == memories
        n, A = 1 << po2, (1 << po2) - zk
        want = logup.reference_links(args, po2, zk, code, data).reshape(-1, n)
        assert np.array_equal(want[:, A:], data.reshape(-1, n)[:, A:])
        on = sum(int((want[args.records[i].last, :A] == ONE).sum()) for i in links)
        assert on == (1 if kind in ("one", "equal") else on) and on >= 1
    # `disjoint`: some access of port 1 links to port 0's access of the same row
    desc, blob, code, data, po2, zk = pc.direct("disjoint")
    args = logup.Arguments.parse(blob)
    w = logup.reference_links(args, po2, zk, code, data).reshape(-1, 1 << po2)
    d = data.reshape(-1, 1 << po2)
    r1 = args.records[1]
    both = [r for r in range((1 << po2) - zk) if w[r1.linked, r] == ONE and w[r1.prevs[0], r] == d[pc.CLOCK, r] and d[pc.KEY, r] % P == d[pc.PER + pc.KEY, r] % P]
    assert len(both) > 5


# ------------------------------------------------------------------------------------------------ paged
def test_the_paged_twin_in_both_modes_is_the_host_walk():
    s = pc.paged()
    args, po2, zk = s["args"], 8, 40
    assert args.version == 9 and args.pages.link == [i for i, r in enumerate(args.records) if isinstance(r, logup.Link)][0]
    chain = lambda **kw: logup.reference_multiplicities(args, po2, zk, s["code"], logup.reference_links(args, po2, zk, s["code"],
                                                        logup.reference_columns(args, po2, zk, s["code"], s["bare"]), **kw))
    by_image, by_table = chain(image=s["image"]), chain(table=s["table"], image_words=pc.W)
    assert np.array_equal(by_image, s["full"]) and np.array_equal(by_table, s["full"])
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    accum, total = logup.reference_accumulate(args, po2, zk, s["code"], s["full"], mix)
    assert total == [0, 0, 0, 0]
    assert (check.reference_check_rows(s["desc"], po2, accum, s["code"], s["full"], s["out"], mix, 0, (1 << po2) - zk) == check.NONE).all()
    assert np.array_equal(logup.reference_page_out(args, po2, zk, s["full"], s["image"]), s["after"])
    first, last = {}, {}
    for r, q, a, *_ in pc.accesses(s["full"], po2, zk):
        first.setdefault(a, q)
        last[a] = q
    assert any(first[a] == 2 and last[a] == 0 for a in first), "no address is first touched through port 2 and last through port 0"
    with pytest.raises(logup.ReferenceError, match="an image is required"):
        logup.reference_links(args, po2, zk, s["code"], s["bare"])


def test_more_pages_than_rows_is_refused():
    """2 ports over 6 active rows touch 12 addresses: the table has 6 rows"""
    desc, blob, code, data, image, po2, zk = pc.overfull()
    args = logup.Arguments.parse(blob)
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(pc.OVERFULL) + "$"):
        logup.reference_links(args, po2, zk, code, data, image=image)
    _, _, code, data, image, _, _ = pc.overfull(spread=False)                # port 1 at port 0's addresses: 6 pages
    out = logup.reference_links(args, po2, zk, code, data, image=image).reshape(-1, 8)
    assert (out[22, :6] == ONE).all() and (out[15, :6] == ONE).all() and (out[4, :6] == 0).all()      # every port-1 access links to port 0's of its row


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["clock", "load", "range"])
def test_the_twin_refuses_across_ports_and_names_the_other_record(what):
    po2, zk = 8, 40
    s = pc.syn(po2, zk, 8)
    forged, want = pc.forge(what, s, po2, zk)
    assert " of record " in want
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(want) + "$"):
        logup.reference_links(s["args"], po2, zk, s["code"], forged)


@pytest.mark.parametrize("what", ["clock0", "outside"])
def test_the_paged_twin_refuses_on_a_joiner(what):
    po2, zk = 8, 40
    s = pc.paged()
    forged, want = pc.forge(what, s, po2, zk)
    assert not want.startswith(f"record {pc._record(s['args'], 0)} ")
    for kw in (dict(image=s["image"]), dict(table=s["table"], image_words=pc.W)):
        if what == "outside" and "table" in kw:                              # the address left the trace: the table then has a row too many, or another address in its row
            continue
        with pytest.raises(logup.ReferenceError, match="^" + re.escape(want) + "$"):
            logup.reference_links(s["args"], po2, zk, s["code"], forged, **kw)


def test_the_lowest_record_then_row_is_the_one_named():
    po2, zk = 8, 40
    s = pc.syn(po2, zk, 8)
    n = 1 << po2
    lcols, wcols = pc.columns()
    d = np.array(s["full"], dtype=np.uint32).reshape(-1, n)
    d[wcols[2], 3] = pc.enc(2)                                               # port 2 at row 3 ...
    d[wcols[1], 100] = pc.enc(5)                                             # ... and port 1 at row 100: the lower record is named
    rec = lambda q: pc._record(s["args"], q)
    with pytest.raises(logup.ReferenceError, match=f"^record {rec(1)} at row 100: write flag 5, not 0 or 1$"):
        logup.reference_links(s["args"], po2, zk, s["code"], d.reshape(-1))
    d[wcols[1], 100] = s["full"].reshape(-1, n)[wcols[1], 100]
    with pytest.raises(logup.ReferenceError, match=f"^record {rec(2)} at row 3: write flag 2, not 0 or 1$"):
        logup.reference_links(s["args"], po2, zk, s["code"], d.reshape(-1))
