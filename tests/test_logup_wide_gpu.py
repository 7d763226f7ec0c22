"""WIDE paging on the GPU (ZKA1 version 10; csrc/links.hip k_links<.., kV = 2>, csrc/page_out.hip k_page_out<.., 2> and k_page_flat): a paged
memory of two value words per address.  Hand-built load / store traces with two value columns (wide_cases.case) at three sizes (A = 216: no
multiple of a wave; 2102; 6198: past one 4096-item sort tile and one scan workgroup) over the key patterns of the narrow paging tests: the data
after derive_links_paged and derive_all_paged equals the numpy twin word for word (blinding rows, code and image untouched), and so does
derive_links_paged_table on the FLAT table at a non-zero, odd table_at; the ported case (three LINK records of one memory) at (12, 1994).
The refusals carry the twin's text and leave `data` unchanged.  page_out / page_out_tree equal the twin and a fresh image_commit, a refused
page-out leaves the image unchanged, page_out(proof=True, walk=True) agrees with the host verifier and the twin's proof.
SYN-LOOKUP-paged-wide seals from the derive byte-identically to the host-made witness, the oracle's verifier accepts, a forged p_in_1
yields no accepted seal; and one seal_page_out_tree(dirty=...) over the flat table verifies from root_before to root_after.

Mutants these cases are meant to catch (the case named is the one whose twin words the mutant cannot produce):
  * the low word used for both halves (word1 = word): every kind of test_wide_pages_match_the_twin (the two halves of every image address
    differ: prev_2 and p_in_1 differ, and a first load of both halves is refused);
  * the halves swapped in the image index (word 0 at 2 a + 1): the same cases, and test_page_out_equals_the_twin (the scatter);
  * the image indexed at a + j instead of V a + j: every kind but `equal` at address 0 (another address's words; `edges` reads past W);
  * p_out_1 taken at the head: every kind but `distinct` (where head = tail) of test_wide_pages_match_the_twin;
  * the flat order j-major (row j D + i): test_page_out_tree_and_the_proof (the flat addresses do not increase: the tree update and the
    proof differ from the twin's) and test_the_flat_table_pages_in (the table variant refuses the walk's table);
  * residues compared as raw words: `big` of test_wide_pages_match_the_twin is refused (a load v of an image word P + v, in either half)."""
import re

import numpy as np
import pytest

import wide_cases as wc
from args_gpu import circuit as _circuit, image_buf as _image, profiled, seal_host as _seal_host, upload as _upload
import zko
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_tree, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, verify_page_tree_chain

pytestmark = pytest.mark.gpu
P, ONE = wc.P, wc.ONE
NOISE = 0x0C0A
TINY = syn_lookup.TINY
AT = 7                                                                        # the flat table's first word in its buffer: non-zero and odd
PG0 = wc.table_base()


def _table_buf(hal, table, at=AT, fill=0xdeadbeef):
    words = np.concatenate([np.full(at, fill, dtype=np.uint32), np.asarray(table, dtype=np.uint32).reshape(-1), np.full(3, fill, dtype=np.uint32)])
    return hal.copy_from("page_table", words)


def _same(got, want, n, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"


@pytest.mark.parametrize("po2,zk", wc.SIZES)
def test_wide_pages_match_the_twin(hal, po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(wc.KINDS):
        desc, blob, code, data, image = wc.case(kind, 100 * po2 + i, po2, zk)
        firsts = wc.check_conditions(kind, code, data, image, A)
        args = logup.Arguments.parse(blob)
        assert args.version == 10 and int(blob[7]) == 0x90001 and args.pages.nv == 2
        code, data = code.reshape(-1), data.reshape(-1)
        c = _circuit(hal, desc, blob)
        assert c.pages() and c.page_words() == 2 and c.derives_links() and c.links_check_reads() == 1
        assert c.derived_data_columns() == sorted(x for r in args.records for x in r.dsts)
        want = logup.reference_links(args, po2, zk, code, data, image=image)
        w, d0 = want.reshape(-1, n), data.reshape(-1, n)
        D = int((w[PG0 + wc.P_ON, :A] == ONE).sum())
        assert D == firsts == {"equal": 1, "distinct": A, "range5": 5, "edges": 4}.get(kind, D) and not w[PG0:PG0 + wc.TABLE_W, D:A].any()
        dcode, ddata = _upload(hal, code, data)
        dimage = _image(hal, image)
        prof = profiled(hal, lambda: hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage))
        assert {"sort_keys", "sort_pack", "pages_scan", "links_check", "links_write"} <= set(prof), set(prof)
        got = ddata.to_vec()
        _same(got, want, n, f"{kind} po2 {po2}")
        assert not np.array_equal(got, data)                                 # the (poisoned) destinations were written
        assert np.array_equal(got.reshape(-1, n)[:, A:], d0[:, A:])          # the blinding rows were not
        assert np.array_equal(dcode.to_vec(), code) and np.array_equal(dimage.to_vec(), image)
        ddata.write(data)                                                    # the stage table hands the image to the links stage
        hal.derive_all_paged(c, po2, zk, dcode, ddata, dimage)
        _same(ddata.to_vec(), want, n, f"{kind} po2 {po2} (derive_all_paged)")


@pytest.mark.parametrize("po2,zk", wc.SIZES)
def test_the_flat_table_pages_in(hal, po2, zk):
    """derive_links_paged_table on the FLAT table of the independent walk, 2 D rows (2 a + j, in_j, out_j) at an odd table_at: the twin's
    words.  The in words are the image's raw words, so the result is the image variant's word for word, `big` included"""
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(wc.KINDS):
        desc, blob, code, data, image = wc.case(kind, 100 * po2 + i, po2, zk)
        args = logup.Arguments.parse(blob)
        _, mem, flat = wc.walk(code, data, image, A, kind)
        assert flat.shape == (2 * len(mem), 3) and (np.diff(flat[:, 0].astype(np.int64)) > 0).all()
        code, data = code.reshape(-1), data.reshape(-1)
        want = logup.reference_links(args, po2, zk, code, data, table=flat, image_words=image.size)
        assert np.array_equal(want, logup.reference_links(args, po2, zk, code, data, image=image))
        c = _circuit(hal, desc, blob)
        dcode, ddata = _upload(hal, code, data)
        dtable = _table_buf(hal, flat)
        hal.derive_links_paged_table(c, po2, zk, dcode, ddata, dtable, image.size, table_at=AT, D=len(flat))
        _same(ddata.to_vec(), want, n, f"{kind} po2 {po2}")
        ddata.write(data)
        hal.derive_all_paged_table(c, po2, zk, dcode, ddata, dtable, image.size, table_at=AT, D=len(flat))
        _same(ddata.to_vec(), want, n, f"{kind} po2 {po2} (derive_all_paged_table)")


@pytest.mark.parametrize("kind", ["big", "range5", "edges"])
def test_the_ported_case(hal, kind):
    """three LINK records of one wide memory, every port with its own selector: the twin's words from the image and from the flat table;
    p_in_j comes from the head access's record, p_out_j from the tail access's own"""
    po2, zk, k = 12, 1994, 3
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = wc.case(kind, 12, po2, zk, k=k)
    wc.check_conditions(kind, code, data, image, A, k=k)
    args = logup.Arguments.parse(blob)
    assert args.version == 10 and int(blob[7]) == 0xd0003
    out, mem, flat = wc.walk(code, data, image, A, kind, k=k)
    code, data = code.reshape(-1), data.reshape(-1)
    want = logup.reference_links(args, po2, zk, code, data, image=image)
    for col, v in out.items():                                               # ... which is the walk's
        assert np.array_equal(want.reshape(-1, n)[col, :A], v), col
    c = _circuit(hal, desc, blob)
    assert c.page_words() == 2
    dcode, ddata = _upload(hal, code, data)
    dimage = _image(hal, image)
    hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    _same(ddata.to_vec(), want, n, kind)
    assert np.array_equal(dimage.to_vec(), image)
    ddata.write(data)
    hal.derive_links_paged_table(c, po2, zk, dcode, ddata, _table_buf(hal, flat), image.size, table_at=AT, D=len(flat))
    _same(ddata.to_vec(), want, n, kind + " (table)")


# ---- refusals ----
def _first_access(data, A, nth):
    """the row of the nth first access (in row order) of a case without a selector, and its address"""
    seen, found = set(), []
    keys = wc.dec(data[wc.KEY, :A])
    for r in range(A):
        if int(keys[r]) not in seen:
            seen.add(int(keys[r]))
            found.append(r)
    return found[nth], int(keys[found[nth]])


def _refused(hal, c, po2, zk, code, data, twin, call, suffix=": the witness is refused"):
    """`twin()` raises the twin's text, `call(dcode, ddata)` the same after "derive_links: ", and `data` stays as it was"""
    with pytest.raises(logup.ReferenceError) as e:
        twin()
    dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
    with pytest.raises(HalError, match=re.escape("derive_links: " + str(e.value) + suffix)):
        call(dcode, ddata)
    assert np.array_equal(ddata.to_vec(), data.reshape(-1))
    return str(e.value)


@pytest.mark.parametrize("what", ["high", "low", "both"])
def test_a_load_wrong_in_one_half_is_refused_with_the_twins_text(hal, what):
    po2, zk = 8, 40
    A = (1 << po2) - zk
    desc, blob, code, data, image = wc.case("two", 21, po2, zk)
    args = logup.Arguments.parse(blob)
    x = lambda v: int(wc.dec(v))
    r, a = _first_access(data, A, 12)
    data[wc.WRITE, r], data[wc.V0, r], data[wc.V1, r] = 0, image[2 * a], image[2 * a + 1]
    if what in ("high", "both"):
        data[wc.V1, r] = wc.enc(x(image[2 * a + 1]) + 1)
    if what in ("low", "both"):
        data[wc.V0, r] = wc.enc(x(image[2 * a]) + 1)
    j = 2 if what == "high" else 1                                           # the lowest j is named first
    want = f"record 0 at row {r}: a load of carried column {j} returns {(x(image[2 * a + j - 1]) + 1) % P}, but the image holds {x(image[2 * a + j - 1])} at its address {a}"
    c = _circuit(hal, desc, blob)
    dimage = _image(hal, image)
    msg = _refused(hal, c, po2, zk, code, data, lambda: logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image),
                   lambda dcode, ddata: hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage))
    assert msg == want and np.array_equal(dimage.to_vec(), image)
    # ... and the same from the flat table
    _, _, flat = wc.walk(*wc.case("two", 21, po2, zk)[2:], A, "two")
    _refused(hal, c, po2, zk, code, data, lambda: logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), table=flat, image_words=image.size),
             lambda dcode, ddata: hal.derive_links_paged_table(c, po2, zk, dcode, ddata, _table_buf(hal, flat), image.size, table_at=AT, D=len(flat)))


def test_an_odd_image_and_a_bad_flat_table_are_refused(hal):
    po2, zk = 12, 1994
    A = (1 << po2) - zk
    desc, blob, code, data, image = wc.case("two", 22, po2, zk)
    args = logup.Arguments.parse(blob)
    c = _circuit(hal, desc, blob)
    flat_code, flat_data = code.reshape(-1), data.reshape(-1)
    odd = image[:-1]
    msg = _refused(hal, c, po2, zk, code, data, lambda: logup.reference_links(args, po2, zk, flat_code, flat_data, image=odd),
                   lambda dcode, ddata: hal.derive_links_paged(c, po2, zk, dcode, ddata, _image(hal, odd)), suffix="")
    assert msg == f"an image of {image.size - 1} words is not a whole number of addresses of 2 value words"
    _, mem, flat = wc.walk(code, data, image, A, "two")
    D = len(mem)
    table_call = lambda table, words=image.size: (lambda dcode, ddata: hal.derive_links_paged_table(c, po2, zk, dcode, ddata, _table_buf(hal, table), words, table_at=AT, D=len(table)))
    twin = lambda table, words=image.size: (lambda: logup.reference_links(args, po2, zk, flat_code, flat_data, table=table, image_words=words))
    _refused(hal, c, po2, zk, code, data, twin(flat, image.size - 1), table_call(flat, image.size - 1), suffix="")
    # the second row of a page holds another address: the head of that page names the flat row
    page = D // 2
    other = flat.copy()
    other[2 * page + 1, 0] += 2
    a = int(flat[2 * page, 0]) // 2
    msg = _refused(hal, c, po2, zk, code, data, twin(other), table_call(other))
    assert re.fullmatch(rf"record 2 at row \d+: address {a} is page {page} of the trace, but row {2 * page + 1} of the page table holds address {2 * a + 3}", msg), msg
    # a table of D rows instead of 2 D: the head of the first page it does not hold in full
    msg = _refused(hal, c, po2, zk, code, data, twin(flat[:D]), table_call(flat[:D]))
    assert re.fullmatch(rf"record 2 at row \d+: address \d+ is page \d+ of the trace, but the page table has {D} rows", msg), msg
    # ... and of two rows more than the trace pages: no row is refused, the count is
    more = np.concatenate([flat, [[flat[-1, 0] + 1, 5, 5], [flat[-1, 0] + 2, 6, 6]]]).astype(np.uint32)
    msg = _refused(hal, c, po2, zk, code, data, twin(more), table_call(more))
    assert msg == f"record 2: the trace pages {D} addresses, but the page table has {2 * D + 2} rows"


# ---- page-out ----
@pytest.mark.parametrize("po2,zk,kind", [(8, 40, "sparse"), (13, 1994, "big"), (12, 1994, "two")])
def test_page_out_equals_the_twin(hal, po2, zk, kind):
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code1, data1, image0 = wc.case(kind, 31, po2, zk)
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
    # the second segment's loads see both halves of the first one's stores
    _, _, code2, data2, image1b = wc.case(kind, 31, po2, zk, image=image1, trace_seed=32)
    dimage.write(image1b)
    dcode, ddata = _upload(hal, code2.reshape(-1), data2.reshape(-1))
    hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    full2 = ddata.to_vec()
    assert np.array_equal(full2, logup.reference_links(args, po2, zk, code2.reshape(-1), data2.reshape(-1), image=image1b))
    hal.page_out(c, po2, zk, ddata, dimage)
    _, mem1, _ = wc.walk(code1, data1, image0, A, kind)
    _, mem2, _ = wc.walk(code2, data2, image0, A, kind, memory=mem1)
    final = image0.copy()
    for a, (v0, v1) in list(mem1.items()) + list(mem2.items()):
        final[2 * a], final[2 * a + 1] = v0, v1
    assert set(mem1) & set(mem2) and np.array_equal(dimage.to_vec() % P, final % P)


@pytest.mark.parametrize("po2,zk,kind,k", [(8, 40, "range5", 1), (13, 1994, "distinct", 1), (12, 1994, "big", 1), (12, 1994, "edges", 3)])
def test_page_out_tree_and_the_proof(hal, po2, zk, kind, k):
    """page_out_tree leaves the image of the twin and the nodes of a fresh image_commit; the proof is the twin's word for word (its table the
    flat one) and page_out(proof=True, walk=True) walks it on the device to the root the host verifier reaches"""
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = wc.case(kind, 7, po2, zk, k=k)
    args = logup.Arguments.parse(blob)
    full = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image)
    after = logup.reference_page_out(args, po2, zk, full, image)
    c = _circuit(hal, desc, blob)
    ddata = hal.alloc_elem("data", full.size)
    ddata.write(full)
    dimage = _image(hal, image)
    tree = hal.image_commit(dimage)
    before = tree.to_vec()
    want_proof = logup.reference_page_out_proof(args, po2, zk, full, image.size, before)
    D = int((full.reshape(-1, n)[args.pages.p_on, :A] == ONE).sum())
    assert int(want_proof[1]) == image.size and int(want_proof[2]) == 2 * D
    got_proof = hal.page_out_proof(c, po2, zk, ddata, dimage, tree)
    assert np.array_equal(got_proof, want_proof)
    prof = profiled(hal, lambda: hal.page_out_tree(c, po2, zk, ddata, dimage, tree))
    assert {"page_out_check", "page_out_write", "page_out_flat"} <= set(prof), set(prof)
    assert np.array_equal(dimage.to_vec(), after)
    fresh = hal.image_commit(_image(hal, after))
    assert np.array_equal(tree.to_vec(), fresh.to_vec())
    assert np.array_equal(zhal.image_proof_verify(got_proof, before[8:16]), hal.image_root(tree))
    # the prover's call: proof, walk on the device, page-out, and the roots compared
    dimage2 = _image(hal, image)
    tree2 = hal.image_commit(dimage2)
    prover = SegmentProver(hal, desc, arguments=blob)
    words = prover.page_out(Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE), ddata, dimage2, tree=tree2, proof=True, walk=True)
    assert np.array_equal(words, want_proof) and np.array_equal(dimage2.to_vec(), after) and np.array_equal(tree2.to_vec(), fresh.to_vec())


def test_a_refused_wide_page_out_leaves_the_image_unchanged(hal):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = wc.case("two", 41, po2, zk)
    args = logup.Arguments.parse(blob)
    c = _circuit(hal, desc, blob)
    W = len(image) // 2
    full = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
    dimage = _image(hal, image)
    tree = hal.image_commit(dimage)
    nodes = tree.to_vec()
    pg = args.pages
    for edits in ([(pg.p_on, 30, wc.enc(2) + np.uint32(P))], [(pg.p_addr, 49, wc.enc(W))], [(pg.p_addr, 30, full[pg.p_addr, 29])], [(pg.p_on, 29, 0)]):
        bad = full.copy()
        for col, row, v in edits:
            bad[col, row] = v
        with pytest.raises(logup.ReferenceError) as e:
            logup.reference_page_out(args, po2, zk, bad.reshape(-1), image)
        ddata = hal.alloc_elem("data", bad.size)
        ddata.write(bad.reshape(-1))
        for call in (lambda: hal.page_out(c, po2, zk, ddata, dimage), lambda: hal.page_out_tree(c, po2, zk, ddata, dimage, tree)):
            with pytest.raises(HalError, match=re.escape("page_out: " + str(e.value) + ": the image is unchanged")):
                call()
        assert np.array_equal(dimage.to_vec(), image) and np.array_equal(tree.to_vec(), nodes)
    # the proof's fourth rule names the word: p_in_1 alone, then both (the lowest first)
    for cols, j in (((pg.p_ins[1],), 1), (pg.p_ins, 0)):
        bad = full.copy()
        for col in cols:
            bad[col, 17] = wc.enc(int(wc.dec(bad[col, 17])) + 1)
        with pytest.raises(logup.ReferenceError, match=f"p_in word {j} ") as e:
            logup.reference_page_out_proof(args, po2, zk, bad.reshape(-1), image.size, nodes)
        ddata.write(bad.reshape(-1))
        with pytest.raises(HalError, match=re.escape("page_out_proof: " + str(e.value))):
            hal.page_out_proof(c, po2, zk, ddata, dimage, tree)
    odd = _image(hal, image[:-1])
    with pytest.raises(HalError, match=re.escape(f"page_out: an image of {image.size - 1} words is not a whole number of addresses of 2 value words: the image is unchanged")):
        hal.page_out(c, po2, zk, ddata, odd)


# ---- SYN-LOOKUP-paged-wide: seals ----
def _paged_wide(po2, zk, W, seed):
    desc, blob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True, reads=True, pages=True, wide=True)
    image = np.random.default_rng(seed).integers(1, P, 2 * W, dtype=np.uint64).astype(np.uint32)
    kw = dict(seed=seed, addr_range=W, reads=True, image=image, wide=True)
    code, full, out = syn_lookup.witness(TINY, po2, zk, link=True, pages=True, **kw)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, count=False, limbs=False, link=False, pages=False, **kw)
    return desc, blob, logup.Arguments.parse(blob).plain().blob(), image, code, full, bare, out


def test_paged_wide_seals_as_the_host_made_witness_and_a_forged_p_in_1_is_not_accepted(hal, oracle):
    po2, zk, W = 8, 40, 64
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, plain, image, code, full, bare, out = _paged_wide(po2, zk, W, po2)
    args = logup.Arguments.parse(blob)
    assert not np.array_equal(bare, full) and args.version == 10
    c = _circuit(hal, desc, blob)
    assert c.page_words() == 2 and set(syn_lookup.pages_layout(TINY.n_words, TINY.n_limbs, wide=True)) <= set(c.derived_data_columns())
    dcode, ddata = _upload(hal, code, bare)
    dimage = _image(hal, image)
    hal.derive_all_paged(c, po2, zk, dcode, ddata, dimage)
    assert np.array_equal(ddata.to_vec(), full)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out, image=dimage, page_out=True)
    host = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    assert np.array_equal(receipt.seal, host.seal)                           # byte-identical to the host-made columns
    assert np.array_equal(dimage.to_vec(), logup.reference_page_out(args, po2, zk, full, image))
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None
    # a witness whose p_in_1 is forged on one page: the page-in no longer answers the first access's removal
    d = full.reshape(-1, n).copy()
    d[args.pages.p_ins[1], 3] = (int(d[args.pages.p_ins[1], 3]) + ONE) % P
    forged = d.reshape(-1)
    try:
        bad = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, forged, out)
    except HalError:
        return                                                               # no seal at all
    with pytest.raises(HalError):
        bad.verify(desc, root)
    assert oc.verify(bad.seal, root) is not None


def test_one_page_out_tree_seal_over_the_flat_table_from_the_dirty_nodes(hal):
    """P2-TREE knows nothing of V: the proof of a wide page-out holds the flat table over the flat image, and seal_page_out_tree(dirty=...)
    seals it from root_before to root_after"""
    po2, zk, W = 8, 40, 64
    desc, blob, plain, image, code, full, bare, out = _paged_wide(po2, zk, W, 9)
    seg_prover = SegmentProver(hal, desc, arguments=blob)
    ddata = hal.alloc_elem("data", full.size)
    ddata.write(full)
    dimage = _image(hal, image)
    tree = hal.image_commit(dimage)
    root_before = hal.image_root(tree)
    proof, dirty = seg_prover.page_out(Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE), ddata, dimage, tree=tree, proof=True, dirty=True)
    root_after = hal.image_root(tree)
    h = int(proof[4])
    assert int(proof[1]) == 2 * W and int(proof[2]) % 2 == 0 and h == 4 and not np.array_equal(root_before, root_after)
    shape = (10, 500)
    parts = hal.page_tree_plan(shape[0], shape[1], 2 * W, proof[5 + h:5 + h + 3 * int(proof[2])][::3])
    prover = SegmentProver(hal, p2_tree.p2_tree_circuit(), arguments=p2_tree.arguments())
    segs = [Segment(index=p, po2=shape[0], zk_cycles=shape[1], noise_seed=NOISE + 1 + p) for p in range(len(parts))]
    recs = prover.seal_page_out_tree(segs, proof, proof.size, None, None, check=True, dirty=dirty)
    root = prover.code_root(hal.page_tree_code(prover.circuit, *shape), shape[0])
    rb, ra, hi = verify_page_tree_chain(recs, root, h, root_before)
    assert np.array_equal(rb, root_before) and np.array_equal(ra, root_after) and hi == 1 << h
