"""The FLAT-ADDRESS columns on the GPU (ZKA1 version 11; csrc/links.hip k_links<true, .., kV = 2, kFlat = true>): the head lane of page i
stores fp_encode(2 a_i + j) to p_flat_j next to p_in_j, the rows below the table zero the two columns with the rest.  flat_cases' traces
(wide_cases' with two more poisoned data columns) at wide_cases' three sizes (A = 216: no multiple of a wave; 2102; 6198: past one sort tile
and one scan workgroup): the whole data group after derive_links_paged, derive_all_paged and derive_links_paged_table equals the numpy twin
bit for bit, and the two flat columns equal the address column of the independent walk's flat table; with one record and with three ports.
A refused witness leaves `data`, the flat columns included, as it was; a version-11 derive runs the profile scopes of the version-10
derive of the same trace.  Then `zkh_accumulate_open` on the tiny tied-wide segment against the reference.

Mutants these cases are meant to catch:
  * 2 a + j stored raw, not encoded: every kind (the twin's cells are Montgomery words);
  * the flat address taken from the raw key word (2 * keycol[row]): `big`, whose keys are raw words >= P;
  * p_flat_1 = 2 a (j dropped) or the two columns swapped: every kind, against the walk's odd and even flat addresses;
  * the store made by the tail lane, or indexed by the row and not the page: every kind but `distinct` / `equal`;
  * the rows below the table not zeroed: every kind but `distinct` (D = A has no such row: it shows that nothing past A is written);
  * the flats written by a check pass, or before the verdict: the refused witness."""
import re

import numpy as np
import pytest

import flat_cases as fc
import wide_cases as wc
from args_gpu import circuit as _circuit, image_buf as _image, profiled, upload as _upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup as sl
from zeth_amd.hal import HalError

pytestmark = pytest.mark.gpu
P, ONE = fc.P, fc.ONE
AT = 7                                                                        # the flat table's first word in its buffer: non-zero and odd
NOISE = 0x0F1A


def _table_buf(hal, table, at=AT, fill=0xdeadbeef):
    words = np.concatenate([np.full(at, fill, dtype=np.uint32), np.asarray(table, dtype=np.uint32).reshape(-1), np.full(3, fill, dtype=np.uint32)])
    return hal.copy_from("page_table", words)


def _same(got, want, n, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"


def _derives(hal, kind, seed, po2, zk, k):
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, blob10, code, data, image = fc.case(kind, seed, po2, zk, k)
    args = logup.Arguments.parse(blob)
    assert args.version == 11 and int(blob[7]) & logup.FLAT_BIT
    full, D, flat = fc.want(code, data, image, A, kind, k)                    # the walk's answer, the flat columns from its flat table
    c0, c1 = fc.flat_columns(data.shape[0])
    code, data = code.reshape(-1), data.reshape(-1)
    want = logup.reference_links(args, po2, zk, code, data, image=image)
    assert np.array_equal(want.reshape(-1, n), full), "the twin is not the walk"
    assert D == {"equal": 1, "distinct": A, "edges": 4}.get(kind, D)
    c = _circuit(hal, desc, blob)
    assert c.pages() and c.page_words() == 2 and c.page_flats() == 2
    assert c.derived_data_columns() == sorted([x for r in args.records for x in r.dsts] + [c0, c1])
    dcode, ddata = _upload(hal, code, data)                                   # the destinations and the blinding rows are poisoned: random words
    dimage = _image(hal, image)
    prof = profiled(hal, lambda: hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage))
    got = ddata.to_vec()
    _same(got, want, n, f"{kind} k {k} po2 {po2}")
    g = got.reshape(-1, n)
    assert np.array_equal(wc.dec(g[c0, :D]), flat[0::2, 0]) and np.array_equal(wc.dec(g[c1, :D]), flat[1::2, 0]), "the flat columns are not the walk's flat addresses"
    assert (g[[c0, c1], :D] < P).all() and not g[[c0, c1], D:A].any()
    assert np.array_equal(g[:, A:], data.reshape(-1, n)[:, A:]), "a blinding row was written"
    assert np.array_equal(dcode.to_vec(), code) and np.array_equal(dimage.to_vec(), image)
    if kind == "big":
        assert (g[args.pages.p_addr, :D] >= P).any()                         # p_addr keeps the raw key word; the flat cells are canonical
    ddata.write(data)
    hal.derive_all_paged(c, po2, zk, dcode, ddata, dimage)
    _same(ddata.to_vec(), want, n, f"{kind} k {k} po2 {po2} (derive_all_paged)")
    ddata.write(data)
    dtable = _table_buf(hal, flat)
    hal.derive_links_paged_table(c, po2, zk, dcode, ddata, dtable, image.size, table_at=AT, D=len(flat))
    _same(ddata.to_vec(), want, n, f"{kind} k {k} po2 {po2} (table)")
    # the version-10 blob of the same circuit: the same scopes (no new launch), the two columns left alone, every other word the same
    c10 = _circuit(hal, desc, blob10)
    assert c10.page_words() == 2 and c10.page_flats() == 0
    ddata.write(data)
    prof10 = profiled(hal, lambda: hal.derive_links_paged(c10, po2, zk, dcode, ddata, dimage))
    assert set(prof) == set(prof10) and {n_: r["calls"] for n_, r in prof.items()} == {n_: r["calls"] for n_, r in prof10.items()}, (set(prof), set(prof10))
    assert {"sort_keys", "sort_pack", "pages_scan", "links_check", "links_write"} <= set(prof)
    old = ddata.to_vec().reshape(-1, n)
    assert np.array_equal(old[:c0], want.reshape(-1, n)[:c0]) and np.array_equal(old[c0:], data.reshape(-1, n)[c0:])


@pytest.mark.parametrize("po2,zk", fc.SIZES)
def test_flat_columns_match_the_twin_and_the_walk(hal, po2, zk):
    for i, kind in enumerate(fc.KINDS):
        _derives(hal, kind, 100 * po2 + i, po2, zk, 1)


@pytest.mark.parametrize("po2,zk", fc.SIZES)
def test_flat_columns_match_the_twin_and_the_walk_with_three_ports(hal, po2, zk):
    for i, kind in enumerate(fc.PORTED_KINDS):
        _derives(hal, kind, 100 * po2 + 50 + i, po2, zk, 3)


@pytest.mark.parametrize("k", [1, 3])
def test_a_refused_witness_leaves_the_flat_columns_as_they_were(hal, k):
    """one load with a wrong SECOND word: the twin's text, from the image and from the flat table, and `data` unchanged"""
    po2, zk, kind = 8, 40, "sparse"
    A = (1 << po2) - zk
    desc, blob, _, code, data, image = fc.case(kind, 21, po2, zk, k)
    args = logup.Arguments.parse(blob)
    _, _, flat = fc.want(code, data, image, A, kind, k)
    data = data.copy()
    acc = wc.accesses(code, data, A, kind, k)
    seen = set()
    for r, q in acc:                                                         # a first access that is a load: the image answers it
        a = int(wc.dec(data[wc.PER * q + wc.KEY, r]))
        if a not in seen and len(seen) >= 5 and data[wc.PER * q + wc.WRITE, r] == 0:
            break
        seen.add(a)
    x = int(wc.dec(image[2 * a + 1]))
    data[wc.PER * q + wc.V1, r] = wc.enc(x + 1)
    for r2, q2 in acc[acc.index((r, q)) + 1:]:                               # the loads that follow return what it returned: one row breaks the rule
        if int(wc.dec(data[wc.PER * q2 + wc.KEY, r2])) == a:
            if data[wc.PER * q2 + wc.WRITE, r2] != 0:
                break
            data[wc.PER * q2 + wc.V1, r2] = wc.enc(x + 1)
    said = f"record {q} at row {r}: a load of carried column 2 returns {(x + 1) % P}, but the image holds {x} at its address {a}"
    c = _circuit(hal, desc, blob)
    dimage = _image(hal, image)
    calls = [(dict(image=image), lambda dcode, ddata: hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)),
             (dict(image=image), lambda dcode, ddata: hal.derive_all_paged(c, po2, zk, dcode, ddata, dimage)),
             (dict(table=flat, image_words=image.size), lambda dcode, ddata: hal.derive_links_paged_table(c, po2, zk, dcode, ddata, _table_buf(hal, flat), image.size, table_at=AT, D=len(flat)))]
    for kw, call in calls:
        with pytest.raises(logup.ReferenceError, match="^" + re.escape(said) + "$"):
            logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), **kw)
        dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
        with pytest.raises(HalError, match=re.escape(said + ": the witness is refused")):
            call(dcode, ddata)
        assert np.array_equal(ddata.to_vec(), data.reshape(-1)), "a refused witness changed `data`"


def test_accumulate_open_on_the_tied_wide_segment_is_the_reference(hal):
    s = fc.segment()
    want_accum, want_total = fc.segment_total()
    po2, zk = fc.SEG_PO2, fc.SEG_ZK
    n, A = 1 << po2, (1 << po2) - zk
    c = _circuit(hal, s["desc"], s["blob"])
    assert c.page_flats() == 2 and c.open_bus() is not None
    dcode, ddata = _upload(hal, s["code"], s["data"])
    k4 = 4 * s["args"].k
    accum = hal.alloc_elem("accum", k4 << po2)
    total = hal.accumulate_open(c, po2, zk, NOISE, dcode, ddata, fc.CHALLENGE, accum)
    got = accum.to_vec().reshape(k4, n)
    bad = np.argwhere(got[:, :A] != np.asarray(want_accum).reshape(k4, n)[:, :A])
    assert bad.size == 0, f"{len(bad)} accum words differ, the first at (column, row) {tuple(bad[0])}"
    assert np.array_equal(total, want_total) and total.any()
    out = np.concatenate([np.zeros(4, dtype=np.uint32), fc.CHALLENGE, total])
    assert hal.check_rows(c, po2, accum, dcode, ddata, out, np.zeros(int(s["desc"][8]), dtype=np.uint32))["row"] == -1
    assert hal.check_bus(c, po2, zk, dcode, ddata)["row"] == -1
    # the derive makes that witness: the underived traces through derive_all_paged give the host-made data group on the active rows
    _, bare, _ = sl.witness(sl.TINY, po2, zk, seed=3, link=False, reads=True, pages=False, image=s["image"], wide=True, flat=True)
    dcode2, ddata2 = _upload(hal, s["code"], bare)
    hal.derive_all_paged(c, po2, zk, dcode2, ddata2, _image(hal, s["image"]))
    assert np.array_equal(ddata2.to_vec().reshape(-1, n)[:, :A], s["data"].reshape(-1, n)[:, :A])
