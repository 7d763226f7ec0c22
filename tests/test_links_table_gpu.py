"""Paging in from a page table on the GPU (zkh_derive_links_paged_table, zkh_derive_all_paged_table; csrc/links.hip, the PAGED_TABLE mode of
k_links): the table stands for the image.  Every kind of pages_cases at its three sizes (A = 216: no multiple of a wave; 2102: nine
workgroups; 6198: past one sort tile) against zkh_derive_links_paged on the same trace, the table read off the image variant's own output
and lying at an offset in its buffer; the refusals with the twin's text, the lowest refused row in a later workgroup; and a table that
overruns its buffer.

Mutants these cases are meant to catch:
  * the page of a head without the workgroup's carry: `distinct`, `sparse`, `big`, `two` at (12, 1994) and (13, 1994) (a head of a later
    workgroup reads a row of the first 256: refused, or another word);
  * the word read at the address (`table[3 a + 1]`) instead of at the page: every kind but a table of one row at address 0;
  * table_at dropped: every case (the table lies 7 words into its buffer);
  * the address comparison dropped: the `changed` refusal is accepted;
  * the count of pages not compared: the `added` refusal is accepted."""
import re

import numpy as np
import pytest

import links_table_cases as lt
import pages_cases as pc
from args_gpu import circuit as _circuit, image_buf as _image, upload as _upload
from zeth_amd.circuits import logup
from zeth_amd.hal import HalError

pytestmark = pytest.mark.gpu
P = pc.P
AT = 7                                                                        # the table's first word in its buffer


def _table_buf(hal, table, at=AT, fill=0xdeadbeef):
    words = np.concatenate([np.full(at, fill, dtype=np.uint32), np.asarray(table, dtype=np.uint32).reshape(-1), np.full(3, fill, dtype=np.uint32)])
    return hal.copy_from("page_table", words), words


@pytest.mark.parametrize("po2,zk", lt.SIZES)
def test_the_table_variant_equals_the_image_variant(hal, po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(pc.KINDS):
        desc, blob, code, data, image = pc.case(kind, 100 * po2 + i, po2, zk)
        code, data = code.reshape(-1), data.reshape(-1)
        c = _circuit(hal, desc, blob)
        dcode, ddata = _upload(hal, code, data)
        hal.derive_links_paged(c, po2, zk, dcode, ddata, _image(hal, image))
        want = ddata.to_vec()
        table = lt.table_of(want, po2, zk)
        D, m = len(table), pc.accesses(code.reshape(-1, n), data.reshape(-1, n), A, kind).size
        assert D == {"equal": 1, "distinct": A, "range5": 5, "edges": 4}.get(kind, D) and (kind != "sparse" or D < m < A), (kind, D, m)
        assert kind != "edges" or (table[0, 0], table[-1, 0]) == (0, len(image) - 1)
        assert (po2, kind) != (12, "distinct") or D == A == 2102
        dtable, words = _table_buf(hal, table)
        ddata.write(data)                                                    # the destinations are poisoned again
        hal.derive_links_paged_table(c, po2, zk, dcode, ddata, dtable, len(image), table_at=AT, D=D)
        got = ddata.to_vec()
        bad = np.nonzero(got % P != want % P)[0]
        assert bad.size == 0, f"{kind} po2 {po2}: {bad.size} residues differ, first at column {bad[0] // n}, row {bad[0] % n}"
        if kind == "big":
            assert (got != want).any()                                       # raw image words >= P came through the table as residues
        else:
            assert np.array_equal(got, want), f"{kind} po2 {po2}"
        assert not np.array_equal(got, data)
        assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])
        assert np.array_equal(dcode.to_vec(), code) and np.array_equal(dtable.to_vec(), words)
        if i == po2 % len(pc.KINDS):                                         # one kind per size: the stage table hands the table to the links stage
            ddata.write(data)
            hal.derive_all_paged_table(c, po2, zk, dcode, ddata, table, len(image))     # rows given as an array are uploaded
            assert np.array_equal(ddata.to_vec(), got), kind


def _refused(hal, desc, blob, po2, zk, code, data, table, W, msg, at=AT):
    """the twin and the device refuse with `msg`; data, code and the table are left as they were"""
    code, data = np.ascontiguousarray(code).reshape(-1), np.ascontiguousarray(data).reshape(-1)
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(logup.Arguments.parse(blob), po2, zk, code, data, table=table, image_words=W)
    c = _circuit(hal, desc, blob)
    dcode, ddata = _upload(hal, code, data)
    dtable, words = _table_buf(hal, table, at)
    for call in (hal.derive_links_paged_table, hal.derive_all_paged_table):
        with pytest.raises(HalError, match="^" + re.escape("derive_links: " + msg + ": the witness is refused") + "$"):
            call(c, po2, zk, dcode, ddata, dtable, W, table_at=at, D=len(table))
        assert np.array_equal(ddata.to_vec(), data) and np.array_equal(dtable.to_vec(), words) and np.array_equal(dcode.to_vec(), code)


@pytest.mark.parametrize("what", ["changed", "cut", "added"])
@pytest.mark.parametrize("po2,zk,kind,page", [(8, 40, "two", 17), (13, 1994, "distinct", 4101)])
def test_a_table_of_other_pages_is_refused_with_the_twins_text(hal, po2, zk, kind, page, what):
    """(13, 1994) `distinct`: page 4101 is sorted position 4101, lane 5 of workgroup 16 and past the first sort tile; `cut` refuses the
    last head, in workgroup 24"""
    A = (1 << po2) - zk
    desc, blob, code, data, image = pc.case(kind, 21, po2, zk)
    table = lt.table_for(code, data, image, A, kind)
    assert page < len(table) and (kind != "distinct" or len(table) == A)
    bad, msg = lt.own_refusals(table, data, A, 2 if kind == "two" else 1, page)[what]
    _refused(hal, desc, blob, po2, zk, code, data, bad, len(image), msg)


@pytest.mark.parametrize("what", ["address", "clock", "load", "tile", "range", "limbs", "lowest"])
def test_the_image_variants_refusals_come_through_a_table(hal, what):
    """test_a_paged_refusal_carries_the_reference_text's cases with the table of the refused trace's own pages in the image's place: the
    same text.  `address` is measured against image_words; `lowest`: a clock 0 on a row below a head that the table does not list"""
    po2, zk = (13, 1994) if what == "tile" else (8, 40)
    n, A = 1 << po2, (1 << po2) - zk
    kind = "distinct" if what == "tile" else "two"
    desc, blob, code, data, image = pc.case(kind, 21, po2, zk)
    W = len(image)
    x = lambda v: int(pc.dec(v))
    firsts = sorted(lt.first_access(data, A, int(a)) for a in np.unique(pc.dec(data[pc.KEY, :A])))
    if what == "tile":
        a = 3 * 4096 + 1
        r = lt.first_access(data, A, a)
    else:
        r = firsts[12]
        a = x(data[pc.KEY, r])
    edit = None
    if what == "address":
        data[pc.KEY, r] = pc.enc(W)
        msg = f"record 0 at row {r}: address {W} outside the image of {W} words"
    elif what == "clock":
        data[pc.CLOCK, r] = np.uint32(P)
        msg = f"record 0 at row {r}: clock 0 is the image's"
    elif what in ("load", "tile"):
        data[pc.WRITE, r], data[pc.VALUE, r] = 0, pc.enc(x(image[a]) + 1)
        msg = f"record 0 at row {r}: a load of carried column 1 returns {(x(image[a]) + 1) % P}, but the image holds {x(image[a])} at its address {a}"
    elif what == "range":
        later = [q for q in range(r + 1, A) if x(data[pc.KEY, q]) == a]
        data[pc.CLOCK, r] = pc.enc((1 << 24) + 1)
        for j, q in enumerate(later):
            data[pc.CLOCK, q] = pc.enc((1 << 24) + 2 + j)
        msg = f"record 0 at row {r}: the clock difference {1 << 24} (after the image) does not fit 3 limbs of 8 bits"
    elif what == "limbs":
        a0 = logup.Arguments.parse(blob)
        blob = logup.Arguments(a0.k, a0.alpha, a0.beta, a0.terms, a0.records[:2] + [logup.Pages(2, 2, 0, a0.pages.dsts[:9])]).blob()
        r = min(q for q in range(A) if x(data[pc.KEY, q]) >= 16)
        msg = f"record 2 at row {r}: address {x(data[pc.KEY, r])} does not fit 2 limbs of 2 bits"
    else:                                                                    # the lowest (record, row) wins, whichever rule it breaks
        data[pc.CLOCK, r] = np.uint32(P)
        later = firsts[20]
        edit = x(data[pc.KEY, later])
        msg = f"record 0 at row {r}: clock 0 is the image's"
    table = lt.table_for(code, data, image, A, kind)
    if edit is not None:
        table[int(np.nonzero(table[:, 0] == edit)[0][0]), 0] += 1000
    _refused(hal, desc, blob, po2, zk, code, data, table, W, msg)


def test_a_table_that_overruns_its_buffer_is_refused_before_a_launch(hal):
    po2, zk = 8, 40
    A = (1 << po2) - zk
    desc, blob, code, data, image = pc.case("range5", 2, po2, zk)
    table = lt.table_for(code, data, image, A, "range5")
    c = _circuit(hal, desc, blob)
    dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
    dtable, words = _table_buf(hal, table)
    hal.prof_enable(True)
    hal.prof_reset()
    for at, D, msg in ((AT, 7, f"a table of 7 rows of 3 words at word {AT} does not fit a buffer of {words.size} words"),
                       (words.size + 1, 0, f"a table of 0 rows of 3 words at word {words.size + 1} does not fit a buffer of {words.size} words")):
        with pytest.raises(HalError, match="^" + re.escape("derive_links: " + msg) + "$"):
            hal.derive_links_paged_table(c, po2, zk, dcode, ddata, dtable, len(image), table_at=at, D=D)
    for W in (0, 1 << 32):
        with pytest.raises(HalError, match="^" + re.escape(f"derive_links: an image of {W} words (1 .. 2^32 - 1)") + "$"):
            hal.derive_links_paged_table(c, po2, zk, dcode, ddata, dtable, W, table_at=AT, D=5)
    with pytest.raises(HalError, match=re.escape("a page table is required (zkh_derive_all_paged_table)")):
        hal.derive_all_paged_table(c, po2, zk, dcode, ddata, None, len(image))
    assert not [r for r in hal.prof_get() if r["calls"]], "a refused call launched"
    hal.prof_enable(False)
    assert np.array_equal(ddata.to_vec(), data.reshape(-1))
    hal.derive_links_paged_table(c, po2, zk, dcode, ddata, dtable, len(image), table_at=AT, D=5)       # and the table as it is is accepted
    assert np.array_equal(ddata.to_vec(), logup.reference_links(logup.Arguments.parse(blob), po2, zk, code.reshape(-1), data.reshape(-1), image=image))


def test_without_a_pages_record_the_table_is_ignored(hal):
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = pc.case("two", 4, po2, zk)
    a = logup.Arguments.parse(blob)
    blob6 = logup.Arguments(a.k, a.alpha, a.beta, a.terms, a.records[:2]).blob()
    data[pc.WRITE, :A] = pc.ONE                                              # all stores: version 6 has nothing to object to
    code, data = code.reshape(-1), data.reshape(-1)
    c = _circuit(hal, desc, blob6)
    want = logup.reference_links(logup.Arguments.parse(blob6), po2, zk, code, data)
    for table in (None, np.zeros((3, 3), dtype=np.uint32)):
        dcode, ddata = _upload(hal, code, data)
        hal.derive_links_paged_table(c, po2, zk, dcode, ddata, table, 0)
        assert np.array_equal(ddata.to_vec(), want)
        ddata.write(data)
        hal.derive_all_paged_table(c, po2, zk, dcode, ddata, table, 0)
        assert np.array_equal(ddata.to_vec(), want)
