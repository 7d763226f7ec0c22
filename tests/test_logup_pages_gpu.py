"""Paging on the GPU (zkh_derive_links_paged, zkh_page_out, zkh_derive_all_paged; csrc/links.hip, the page-out in csrc/page_out.hip): the memory of a LINK record starts
from an image and goes back into it.  Hand-built load / store traces (pages_cases.case) at three sizes (A = 216: no multiple of a wave;
2102; 6198: past one 4096-item sort tile and past one scan workgroup) over the key patterns that can break the page scan and the table —
one address for every access (D = 1, head and tail 6197 positions apart), all distinct (D = m: every position both head and tail, every
load answered by the image), five addresses, a sparse selector (D < m < A: both zeroing paths), the addresses 0 and W - 1, raw words >= P
in key, clock, value and image next to their residues, and a second LINK record that is not paged: the data equals the host reference
word for word, and so does a derive at po2 19, the smallest size at which a thread of the carry scan owns two counters.
The refusals carry the reference's text and leave `data` unchanged; page-out equals `reference_page_out`, a second segment
derived from that image equals the walk over both segments, and a refused page-out leaves the image unchanged.  SYN-LOOKUP-paged seals
byte-identically to the host-made witness under the plain blob, and a forked page yields no accepted seal.

Mutants these cases are meant to catch (the case named is the one whose reference words the mutant cannot produce):
  * the page index from an exclusive instead of an inclusive scan: every kind of test_pages_match_the_reference (the table moves up by one
    row; `equal` writes row -1);
  * the second-level carry dropped at a workgroup boundary: `distinct`, `sparse`, `big`, `two` of test_pages_match_the_reference at every
    size (D > 256 or heads in a later workgroup: pages of a later workgroup land on the first one's rows);
  * p_out taken at the head: every kind but `distinct` (where head = tail) of test_pages_match_the_reference;
  * the previous address taken from the packed key: `range5`, `edges`, `sparse` (keys whose constant bits the packed key drops: the gaps differ);
  * image residues compared as raw words: `big` of test_pages_match_the_reference is refused (a load v of an image word P + v);
  * rows [D, A) not zeroed: every kind but `distinct` at A = m (the poisoned table rows stay)."""
import re

import numpy as np
import pytest

import pages_cases as pc
from args_gpu import circuit as _circuit, image_buf as _image, links_refused, profiled, seal_host as _seal_host, upload as _upload
import zko
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x0C06
ONE = (1 << 32) % P
TINY = syn_lookup.TINY
SIZES = [(8, 40), (12, 1994), (13, 1994)]


@pytest.mark.parametrize("po2,zk", SIZES)
def test_pages_match_the_reference(hal, po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(pc.KINDS):
        desc, blob, code, data, image = pc.case(kind, 100 * po2 + i, po2, zk)
        args = logup.Arguments.parse(blob)
        assert args.version == 7 and int(blob[7]) == 0x10001 and len(args.records) == (3 if kind == "two" else 2)
        code, data = code.reshape(-1), data.reshape(-1)
        c = _circuit(hal, desc, blob)
        assert c.pages() and c.derives_links() and c.links_check_reads() == 1
        assert c.derived_data_columns() == sorted(x for r in args.records for x in r.dsts)
        want = logup.reference_links(args, po2, zk, code, data, image=image)
        w, d0 = want.reshape(-1, n), data.reshape(-1, n)
        # the input exercises the path: D is what the kind is meant to have, and the image answers first accesses with non-zero words
        rows = pc.accesses(code.reshape(-1, n), d0, A, kind)
        D = int((w[pc.P_ON, :A] == ONE).sum())
        assert D == np.unique(pc.dec(d0[pc.KEY, rows])).size == {"equal": 1, "distinct": A, "range5": 5, "edges": 4}.get(kind, D) and D <= rows.size, (kind, D)
        assert not w[pc.P_ON:pc.P_ON + 11, D:A].any() and (kind != "sparse" or D < rows.size < A)
        firsts = rows[w[pc.LINKED, rows] == 0]
        loads = firsts[(d0[pc.WRITE, firsts] % P == 0) & (w[pc.PVALUE, firsts] % P != 0)]
        assert firsts.size == D and 4 * loads.size >= D, (kind, D, loads.size)
        if kind == "big":
            assert (image >= P).sum() > image.size // 6 and (d0[pc.KEY, :A] >= P).any() and (d0[pc.CLOCK, :A] >= P).any() and (d0[pc.VALUE, :A] >= P).any()
        dcode, ddata = _upload(hal, code, data)
        dimage = _image(hal, image)
        prof = profiled(hal, lambda: hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage))
        assert {"sort_keys", "sort_pack", "pages_scan", "links_check", "links_write"} <= set(prof), set(prof)
        got = ddata.to_vec()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{kind} po2 {po2}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
        assert not np.array_equal(got, data)                                 # the (poisoned) destinations were written
        assert np.array_equal(got.reshape(-1, n)[:, A:], d0[:, A:])          # the blinding rows were not
        assert np.array_equal(dcode.to_vec(), code) and np.array_equal(dimage.to_vec(), image)
        ddata.write(data)                                                    # the stage table hands the image to the links stage
        hal.derive_all_paged(c, po2, zk, dcode, ddata, dimage)
        assert np.array_equal(ddata.to_vec(), want)


@pytest.mark.parametrize("kind", ["distinct", "sparse"])
def test_the_carry_scan_with_two_counters_per_thread(hal, kind):
    """po2 19 is the smallest size at which a thread of the carry scan owns more than one counter: 2041 workgroups of 256 positions
    under 1024 threads.  `distinct`: every workgroup's total is 256, so a dropped or shifted carry moves every page; `sparse`: 40
    pages, most totals 0"""
    po2, zk = 19, 1994
    n, A = 1 << po2, (1 << po2) - zk
    assert (A + 255) // 256 == 2041 > 1024
    desc, blob, code, data, image = pc.case(kind, 19, po2, zk)
    args = logup.Arguments.parse(blob)
    code, data = code.reshape(-1), data.reshape(-1)
    want = logup.reference_links(args, po2, zk, code, data, image=image)
    D, m = int((want.reshape(-1, n)[pc.P_ON, :A] == ONE).sum()), pc.accesses(code.reshape(-1, n), data.reshape(-1, n), A, kind).size
    assert (D, m) == (A, A) if kind == "distinct" else D == 40 and A // 4 < m < A // 3, (D, m)
    dcode, ddata = _upload(hal, code, data)
    dimage = _image(hal, image)
    hal.derive_links_paged(_circuit(hal, desc, blob), po2, zk, dcode, ddata, dimage)
    got = ddata.to_vec()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{kind}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
    assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])                 # the blinding rows were not written
    assert np.array_equal(dimage.to_vec(), image)


def test_without_a_pages_record_the_paged_calls_are_the_plain_ones(hal):
    po2, zk = 8, 40
    desc, blob, code, data, image = pc.case("two", 4, po2, zk)
    a = logup.Arguments.parse(blob)
    blob6 = logup.Arguments(a.k, a.alpha, a.beta, a.terms, a.records[:2]).blob()
    assert int(blob6[1]) == 6
    code, data = code.reshape(-1), data.reshape(-1)
    c = _circuit(hal, desc, blob6)
    assert not c.pages()
    # under version 6 memory starts zeroed: the first loads of this trace return the image's words, and are refused
    with pytest.raises(logup.ReferenceError, match="its address was never accessed: the value must be 0") as e:
        logup.reference_links(logup.Arguments.parse(blob6), po2, zk, code, data)
    n, A = 1 << po2, (1 << po2) - zk
    d = data.reshape(-1, n).copy()
    d[pc.WRITE, :A] = ONE                                                    # all stores: the version-6 rule has nothing to object to
    d = d.reshape(-1)
    want = logup.reference_links(logup.Arguments.parse(blob6), po2, zk, code, d)
    for image_buf in (None, _image(hal, image)):
        dcode, ddata = _upload(hal, code, d)
        hal.derive_links_paged(c, po2, zk, dcode, ddata, image_buf)
        assert np.array_equal(ddata.to_vec(), want)
        ddata.write(d)
        hal.derive_all_paged(c, po2, zk, dcode, ddata, image_buf)
        assert np.array_equal(ddata.to_vec(), want)
        ddata.write(data)
        with pytest.raises(HalError, match=re.escape("derive_links: " + str(e.value))):
            hal.derive_links_paged(c, po2, zk, dcode, ddata, image_buf)


# ---- refusals ----
def _first_access(data, A, nth):
    """the row of the nth first access (in row order) of the paged record of a case without a selector, and its address"""
    seen, found = set(), []
    keys = pc.dec(data[pc.KEY, :A])
    for r in range(A):
        if int(keys[r]) not in seen:
            seen.add(int(keys[r]))
            found.append(r)
    return found[nth], int(keys[found[nth]])


@pytest.mark.parametrize("what", ["address", "clock", "load", "tile", "range", "limbs"])
def test_a_paged_refusal_carries_the_reference_text(hal, what):
    po2, zk = (13, 1994) if what == "tile" else (8, 40)
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = pc.case("distinct" if what == "tile" else "two", 21, po2, zk)
    W = len(image)
    x = lambda v: int(pc.dec(v))
    if what == "tile":                                                       # the unlinked load at sorted position 4096: the address of rank 4096
        r = int(np.nonzero(pc.dec(data[pc.KEY, :A]) == 3 * 4096 + 1)[0][0])
        a = 3 * 4096 + 1
    else:
        r, a = _first_access(data, A, 12)
    if what == "address":
        data[pc.KEY, r] = pc.enc(W)
        msg = f"record 0 at row {r}: address {W} outside the image of {W} words"
    elif what == "clock":
        data[pc.CLOCK, r] = np.uint32(P)                                     # clock 0 as the raw word P
        msg = f"record 0 at row {r}: clock 0 is the image's"
    elif what in ("load", "tile"):
        data[pc.WRITE, r], data[pc.VALUE, r] = 0, pc.enc(x(image[a]) + 1)
        msg = f"record 0 at row {r}: a load of carried column 1 returns {(x(image[a]) + 1) % P}, but the image holds {x(image[a])} at its address {a}"
    elif what == "range":
        later = [q for q in range(r + 1, A) if x(data[pc.KEY, q]) == a]
        data[pc.CLOCK, r] = pc.enc((1 << 24) + 1)
        for j, q in enumerate(later):                                        # the later accesses follow, so that only the first one is out of range
            data[pc.CLOCK, q] = pc.enc((1 << 24) + 2 + j)
        msg = f"record 0 at row {r}: the clock difference {1 << 24} (after the image) does not fit 3 limbs of 8 bits"
    else:                                                                    # a PAGES record of 2 limbs of 2 bits: the addresses from 16 on do not fit
        a0 = logup.Arguments.parse(blob)
        short = logup.Arguments(a0.k, a0.alpha, a0.beta, a0.terms, a0.records[:2] + [logup.Pages(2, 2, 0, a0.pages.dsts[:9])])
        blob = short.blob()
        r = min(q for q in range(A) if x(data[pc.KEY, q]) >= 16)
        msg = f"record 2 at row {r}: address {x(data[pc.KEY, r])} does not fit 2 limbs of 2 bits"
    links_refused(hal, desc, blob, po2, zk, code, data, msg, image=image)


def test_a_paging_circuit_needs_an_image(hal):
    po2, zk = 8, 40
    desc, blob, code, data, image = pc.case("range5", 2, po2, zk)
    c = _circuit(hal, desc, blob)
    dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
    for call in (hal.derive_links, hal.derive_all, lambda *a: hal.derive_links_paged(*a, None), lambda *a: hal.derive_all_paged(*a, None)):
        with pytest.raises(HalError, match=re.escape(logup.PAGES_NEED_IMAGE)):
            call(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), data.reshape(-1))
    with pytest.raises(HalError, match=re.escape(logup.PAGES_NEED_IMAGE)):  # and so does a seal that was given none
        _seal_host(hal, SegmentProver(hal, desc, arguments=blob), Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE), code.reshape(-1),
                   data.reshape(-1), np.zeros(4, dtype=np.uint32))


# ---- page-out ----
@pytest.mark.parametrize("po2,zk,kind", [(8, 40, "sparse"), (13, 1994, "big"), (12, 1994, "two")])
def test_page_out_and_a_second_segment(hal, po2, zk, kind):
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code1, data1, image0 = pc.case(kind, 31, po2, zk)
    args = logup.Arguments.parse(blob)
    c = _circuit(hal, desc, blob)
    dimage = _image(hal, image0)
    dcode, ddata = _upload(hal, code1.reshape(-1), data1.reshape(-1))
    hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    full1 = ddata.to_vec()
    hal.page_out(c, po2, zk, ddata, dimage)
    image1 = dimage.to_vec()
    assert np.array_equal(image1, logup.reference_page_out(args, po2, zk, full1, image0)) and not np.array_equal(image1, image0)
    assert np.array_equal(ddata.to_vec(), full1)
    # the second segment's loads see the first one's stores; `big` rewrites words of the image as raw words >= P on the way
    _, _, code2, data2, image1b = pc.case(kind, 31, po2, zk, image=image1, trace_seed=32)
    dimage.write(image1b)
    dcode, ddata = _upload(hal, code2.reshape(-1), data2.reshape(-1))
    hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    full2 = ddata.to_vec()
    assert np.array_equal(full2, logup.reference_links(args, po2, zk, code2.reshape(-1), data2.reshape(-1), image=image1b))
    hal.page_out(c, po2, zk, ddata, dimage)
    image2 = dimage.to_vec()
    # ... and equal one walk over both segments with the memory in one dictionary that starts from the first image
    _, mem1 = pc.walk(code1, data1, image0, A, kind)
    out2, mem2 = pc.walk(code2, data2, image0, A, kind, memory=mem1)
    f2 = full2.reshape(-1, n)
    for col, v in out2.items():
        assert np.array_equal(f2[col, :A] % P, v % P), col
    assert set(mem1) & set(mem2)
    final = image0.copy()
    for a, v in list(mem1.items()) + list(mem2.items()):
        final[a] = v
    assert np.array_equal(image2 % P, final % P)


def test_a_refused_page_out_leaves_the_image_unchanged(hal):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = pc.case("two", 41, po2, zk)
    args = logup.Arguments.parse(blob)
    c = _circuit(hal, desc, blob)
    W = len(image)
    full = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
    x = lambda v: int(pc.dec(v))
    dimage = _image(hal, image)
    for edits in ([(pc.P_ON, 30, pc.enc(2) + np.uint32(P))], [(pc.P_ADDR, 49, pc.enc(W))], [(pc.P_ADDR, 30, full[pc.P_ADDR, 29])], [(pc.P_ON, 29, 0)],
                  [(pc.P_ON, 40, pc.enc(7)), (pc.P_ADDR, 20, pc.enc(W + 3))]):     # of two bad rows the lower
        bad = full.copy()
        for col, row, v in edits:
            bad[col, row] = v
        with pytest.raises(logup.ReferenceError) as e:
            logup.reference_page_out(args, po2, zk, bad.reshape(-1), image)
        ddata = hal.alloc_elem("data", bad.size)
        ddata.write(bad.reshape(-1))
        with pytest.raises(HalError, match=re.escape("page_out: " + str(e.value) + ": the image is unchanged")):
            hal.page_out(c, po2, zk, ddata, dimage)
        assert np.array_equal(dimage.to_vec(), image)
    assert "row 20: address" in str(e.value)
    plain = _circuit(hal, desc, args.plain().blob())
    with pytest.raises(HalError, match="page_out: the circuit's arguments hold no PAGES record"):
        hal.page_out(plain, po2, zk, ddata, dimage)


# ---- SYN-LOOKUP-paged: seals ----
def _paged(po2, zk, W, seed):
    desc, blob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True, reads=True, pages=True)
    image = np.random.default_rng(seed).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, full, out = syn_lookup.witness(TINY, po2, zk, seed=seed, addr_range=W, link=True, reads=True, pages=True, image=image)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=seed, addr_range=W, count=False, limbs=False, link=False, reads=True, pages=False, image=image)
    return desc, blob, logup.Arguments.parse(blob).plain().blob(), image, code, full, bare, out


@pytest.mark.parametrize("po2,zk,W", [(8, 40, 64), (12, 1994, 300)])
def test_the_chain_equals_the_host_made_witness_and_seals_alike(hal, oracle, po2, zk, W):
    desc, blob, plain, image, code, full, bare, out = _paged(po2, zk, W, po2)
    assert not np.array_equal(bare, full) and logup.Arguments.parse(blob).version == 7
    c = _circuit(hal, desc, blob)
    assert c.pages() and set(syn_lookup.pages_layout(TINY.n_words, TINY.n_limbs)) <= set(c.derived_data_columns())
    dcode, ddata = _upload(hal, code, bare)
    dimage = _image(hal, image)
    hal.derive_all_paged(c, po2, zk, dcode, ddata, dimage)
    assert np.array_equal(ddata.to_vec(), full)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out, image=dimage)
    again = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out, image=dimage, page_out=True)
    host = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    assert np.array_equal(receipt.seal, host.seal) and np.array_equal(again.seal, host.seal)     # run to run, and as the host-made columns
    assert np.array_equal(dimage.to_vec(), logup.reference_page_out(logup.Arguments.parse(blob), po2, zk, full, image))
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


def test_a_forked_page_yields_no_accepted_seal(hal, oracle):
    po2, zk, W = 8, 40, 64
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, plain, image, code, full, bare, out = _paged(po2, zk, W, 5)
    args = logup.Arguments.parse(blob)
    forged, row = syn_lookup.fork_page(TINY, full, po2, zk, image)
    m = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[2]
    d = forged.reshape(-1, n).copy()
    d[m, :A] = 0
    forged = logup.reference_multiplicities(args, po2, zk, code, d.reshape(-1))                   # the multiplicities counted again
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    _, total = logup.reference_accumulate(logup.Arguments.parse(plain), po2, zk, code, forged, mix)
    assert total == [0, 0, 0, 0]                                             # every lookup is answered and the bus balances
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    honest = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    honest.verify(desc, root)
    with pytest.raises(HalError, match=f"witness: row {row} fails constraint step"):             # check=True names its row
        _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, forged, out, check=True)
    try:
        receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, forged, out)
    except HalError:
        return                                                               # no seal at all
    with pytest.raises(HalError):
        receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is not None
