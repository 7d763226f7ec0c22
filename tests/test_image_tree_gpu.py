"""The image's commitment on the GPU (zkh_image_commit, zkh_page_out_tree; csrc/image.hip, the listed fold of csrc/hash.hip): the tree of
a memory image built on the device equals logup.reference_image_tree word for word, and a page-out that goes through the tree leaves the
nodes that a fresh commit of the new image writes.

Commit: W = 1, 7, 8, 9 (one leaf, a partial leaf, two leaves), 650 and 1000 (partial last leaf and padding leaves), 1024 / 1025 (L = 128 /
256), the `big` image (raw words >= P), and W = 2^22 - 3 (L = 2^19: every fold kernel, the leaf layer against numpy, three paths up to
the root).  Page-out through the real derive: every kind of pages_cases at two sizes, and a second segment from the paged-out image.
The listed route: hand-made page tables (zkh_page_out reads p_on, p_addr and p_out alone) over the image of 2^22 - 3 words, whose
parent layers of 2^18, 2^17 and 2^16 nodes lie above the width the 8-lane kernels rebuild densely; po2 13 with 1994 blinding rows gives
6198 table rows, past one 4096-item tile and past 24 scan workgroups.  The seam tables of pages_cases put rows 255 and 256, the two
sides of the seam between two scan workgroups, into one leaf, into sibling leaves and under different parents.

Mutants these cases are meant to catch (the case named is the one whose reference words the mutant cannot produce):
  * raw words hashed instead of residues: `big` of test_commit_matches_the_reference; `spread` and `twins` (a third of the image and of
    p_out are raw words >= P: the leaves must hold their residues);
  * only the paged word of a leaf refreshed: `twins` (words 0 and 7 of one leaf are paged and the leaf's first row alone rewrites it:
    all eight words, or word 7 stays what it was);
  * a carry dropped at a scan-workgroup boundary: `spread`, `twins` and `all` (more than 256 dirty parents: the parents of a later
    workgroup land on the first one's ranks, and nodes stay stale);
  * duplicates not merged (a parent hashed from a stale sibling when both children are dirty, or hashed twice): `twins` has them on the
    leaf layer (8 j and 8 j + 7) and on the first parent layer (leaves 2 j and 2 j + 1); `edges` only at the root;
  * the dense top started one level too high: every table but `none` (the first layer that is not listed keeps stale nodes);
  * padding not zero: W = 1, 7, 9, 650, 1000, 1025 of test_commit_matches_the_reference (the device buffer is not zeroed by the
    allocator: the tests poison it), and `edges`, whose last leaf is the partial one."""
import re

import numpy as np
import pytest

import pages_cases as pc
from args_gpu import circuit as _circuit, image_buf as _image, profiled, seal_host as _seal_host, upload as _upload
from zeth_amd import host
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
ONE = (1 << 32) % P
NOISE = 0x0C07
TINY = syn_lookup.TINY
BIG_W = (1 << 22) - 3                                                        # L = 2^19: three parent layers above the dense top of 2^15


def _words(rng, size, big=True):
    """random non-zero residues, a third of them as the raw word >= P of the same residue"""
    w = rng.integers(1, P, size, dtype=np.uint64).astype(np.uint32)
    if big:
        w[rng.random(size) < 0.33] += np.uint32(P)
    return w


# ---- commit ----
@pytest.mark.parametrize("W", [1, 7, 8, 9, 650, 1000, 1024, 1025])
def test_commit_matches_the_reference(hal, W):
    image = _words(np.random.default_rng(W), W, big=W in (1000, 1025))
    want = logup.reference_image_tree(image)
    assert hal.image_tree_words(W) == want.size == 16 * logup.image_tree_leaves(W) and hal.image_tree_words(0) == 0
    nodes = hal.copy_from("nodes", np.full(want.size, 0xdeadbeef, dtype=np.uint32))      # poisoned: digest 0 and the padding are written
    assert hal.image_commit(_image(hal, image), nodes) is nodes
    assert np.array_equal(nodes.to_vec().reshape(-1, 8), want)
    fresh = hal.image_commit(_image(hal, image))
    assert np.array_equal(fresh.to_vec(), want.reshape(-1)) and np.array_equal(hal.image_root(fresh), want[1])
    assert np.array_equal(hal.image_root(fresh), logup.reference_image_root(image))


def test_commit_of_the_distinct_and_the_big_image(hal):
    for kind in ("distinct", "big"):
        image = pc.case(kind, 7, 8, 40)[4]
        assert image.size == (650 if kind == "distinct" else 1000) and (kind != "big" or (image >= P).sum() > image.size // 6)
        want = logup.reference_image_tree(image)
        assert np.array_equal(hal.image_commit(_image(hal, image)).to_vec(), want.reshape(-1))
        assert np.array_equal(want, logup.reference_image_tree(image % P))


@pytest.fixture(scope="module")
def big(hal):
    """the image of 2^22 - 3 words (a third of them raw words >= P) and its committed nodes, read back once: (image, nodes); unchanged by
    the tests, which upload their own copies"""
    image = _words(np.random.default_rng(22), BIG_W)
    nodes = hal.image_commit(_image(hal, image)).to_vec()
    return image, nodes


def test_commit_of_a_large_image(hal, big):
    image, flat = big
    L = 1 << 19
    assert flat.size == hal.image_tree_words(BIG_W) == 16 * L
    nodes = flat.reshape(-1, 8)
    leaves = np.zeros(8 * L, dtype=np.uint32)
    leaves[:BIG_W] = image % P
    assert not nodes[0].any() and np.array_equal(nodes[L:].reshape(-1), leaves)
    for leaf in (0, L - 1, 300001):                                          # the first, the partial last one, one in the middle
        i = L + leaf
        while i > 1:
            i >>= 1
            assert np.array_equal(nodes[i], host.hash_pair(nodes[2 * i], nodes[2 * i + 1])), (leaf, i)


def test_commit_refuses_an_empty_image_and_wrong_sized_nodes(hal):
    image = _image(hal, _words(np.random.default_rng(1), 100))
    for size in (16 * 16 - 8, 16 * 16 + 8, 16 * 8, 16 * 32):
        with pytest.raises(HalError, match="image_commit: nodes of .* words; an image of 100 words has a tree of 256"):
            hal.image_commit(image, hal.alloc_elem("nodes", size))
    with pytest.raises(HalError, match="image_commit: an image of 0 words"):
        hal.image_commit(image.slice(0, 0), hal.alloc_elem("nodes", 16))
    with pytest.raises(HalError, match="image_commit: an image of 0 words"):
        hal.image_commit(image.slice(0, 0))


# ---- page-out through the real derive ----
@pytest.mark.parametrize("po2,zk", [(8, 40), (12, 1994)])
def test_page_out_through_the_derive_keeps_the_tree(hal, po2, zk):
    for i, kind in enumerate(pc.KINDS):
        desc, blob, code, data, image0 = pc.case(kind, 200 * po2 + i, po2, zk)
        args = logup.Arguments.parse(blob)
        c = _circuit(hal, desc, blob)
        dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
        dimage = _image(hal, image0)
        nodes = hal.image_commit(dimage)
        before = nodes.to_vec()
        assert np.array_equal(before, logup.reference_image_tree(image0).reshape(-1))
        hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
        full = ddata.to_vec()
        hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)
        image1 = dimage.to_vec()
        assert np.array_equal(image1, logup.reference_page_out(args, po2, zk, full, image0)), kind
        got = nodes.to_vec()
        assert np.array_equal(got, hal.image_commit(dimage).to_vec()), kind
        assert not np.array_equal(got, before) and not np.array_equal(got[8:16], before[8:16]), kind
        assert np.array_equal(hal.image_root(nodes), logup.reference_image_root(image1)), kind
        assert np.array_equal(ddata.to_vec(), full)


@pytest.mark.parametrize("po2,zk,kind", [(8, 40, "sparse"), (12, 1994, "big")])
def test_a_second_segment_ends_at_the_root_the_walk_predicts(hal, po2, zk, kind):
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code1, data1, image0 = pc.case(kind, 31, po2, zk)
    c = _circuit(hal, desc, blob)
    dimage = _image(hal, image0)
    nodes = hal.image_commit(dimage)
    dcode, ddata = _upload(hal, code1.reshape(-1), data1.reshape(-1))
    hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)
    image1 = dimage.to_vec()
    # `big` hands the second segment raw words >= P for some residues of the first one's image: one memory, one root, the nodes stay
    _, _, code2, data2, image1b = pc.case(kind, 31, po2, zk, image=image1, trace_seed=32)
    assert np.array_equal(image1b % P, image1 % P)
    dimage.write(image1b)
    dcode, ddata = _upload(hal, code2.reshape(-1), data2.reshape(-1))
    hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
    hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)
    _, mem1 = pc.walk(code1, data1, image0, A, kind)
    _, mem2 = pc.walk(code2, data2, image0, A, kind, memory=mem1)
    final = image0.copy()
    for a, v in list(mem1.items()) + list(mem2.items()):
        final[a] = v
    assert np.array_equal(dimage.to_vec() % P, final % P)
    assert np.array_equal(hal.image_root(nodes), logup.reference_image_root(final))
    assert np.array_equal(nodes.to_vec(), logup.reference_image_tree(final).reshape(-1))


# ---- the listed route: hand-made tables ----
def _small_case():
    """desc and blob of a small case: they do not depend on po2"""
    desc, blob = pc.case("range5", 3, 8, 40)[:2]
    other = pc.case("range5", 3, 9, 40)[:2]
    assert np.array_equal(desc, other[0]) and np.array_equal(blob, other[1])
    return desc, blob


def _table(po2, addrs, out):
    """a data trace of zeros but for the page table's p_on, p_addr and p_out on its first len(addrs) rows"""
    data = np.zeros((pc.PAGED_W + 1, 1 << po2), dtype=np.uint32)
    D = len(addrs)
    data[pc.P_ON, :D], data[pc.P_ADDR, :D], data[pc.P_OUT, :D] = ONE, pc.enc(addrs), out
    return data.reshape(-1)


def _addresses(what, A, rng, rows=None):
    L = 1 << 19
    if what in pc.SEAM_TABLES:
        return pc.seam_table(what, rows, BIG_W, rng)
    if what == "spread":
        return np.sort(rng.choice(BIG_W, A, replace=False)).astype(np.int64)
    if what == "twins":                                                      # 8 j and 8 j + 7 of the leaves 2 q and 2 q + 1, A // 4 pairs of leaves
        q = np.sort(rng.choice(L // 2 - 1, A // 4, replace=False)).astype(np.int64)
        leaves = np.stack([2 * q, 2 * q + 1], axis=1).reshape(-1)
        return np.stack([8 * leaves, 8 * leaves + 7], axis=1).reshape(-1)
    if what == "edges":
        return np.array([0, BIG_W - 1], dtype=np.int64)
    if what == "one":
        return np.array([1234567], dtype=np.int64)
    if what == "none":
        return np.zeros(0, dtype=np.int64)
    assert what == "all"
    return 8 * np.arange(L, dtype=np.int64)


def _run_table(hal, big, what, po2, zk, seed=5, rows=None):
    image0, nodes0 = big
    A = (1 << po2) - zk
    rng = np.random.default_rng(seed)
    addrs = _addresses(what, A, rng, rows)
    D = len(addrs)
    assert D <= A and (D < 2 or (np.diff(addrs) > 0).all()) and (D == 0 or addrs[-1] < BIG_W)
    out = _words(rng, D)
    desc, blob = _small_case()
    c = _circuit(hal, desc, blob)
    ddata = hal.copy_from("data", _table(po2, addrs, out))
    dimage, nodes = _image(hal, image0), hal.copy_from("nodes", nodes0)
    prof = profiled(hal, lambda: hal.page_out_tree(c, po2, zk, ddata, dimage, nodes))
    want = image0.copy()
    want[addrs] = out
    assert np.array_equal(dimage.to_vec(), want)
    got = nodes.to_vec()
    fresh = hal.image_commit(dimage).to_vec()
    bad = np.nonzero(got != fresh)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, the first in digest {bad[0] // 8}"
    return prof, got, D


@pytest.mark.parametrize("what", ["spread", "twins", "edges", "one", "none"])
def test_a_hand_made_table_leaves_the_nodes_of_a_fresh_commit(hal, big, what):
    prof, got, D = _run_table(hal, big, what, 13, 1994)
    assert {"page_out_check", "page_out_write"} <= set(prof)
    if what == "none":
        assert D == 0 and np.array_equal(got, big[1]) and not {"image_leaves", "image_list", "image_sparse", "hash_fold_wide", "hash_fold_tail"} & set(prof)
        return
    assert not np.array_equal(got[8:16], big[1][8:16])                       # the root moved
    assert {"image_leaves", "hash_fold_wide", "hash_fold_tail"} <= set(prof), set(prof)
    if what in ("spread", "edges"):                                          # no threshold sends these to the dense path
        assert "image_list" in prof and prof["image_sparse"]["calls"] >= 2, prof
        assert D == {"spread": 6198, "edges": 2}[what]


@pytest.mark.parametrize("D", pc.SEAM_ROWS)
@pytest.mark.parametrize("what", pc.SEAM_TABLES)
def test_a_head_on_the_seam_of_two_workgroups(hal, big, what, D):
    """lane 0 of the second scan workgroup is no head of the first list of dirty parents (rows 255 and 256 in one leaf or in sibling
    leaves), or it is one (different parents): the listed route still leaves the nodes of a fresh commit"""
    prof, got, rows = _run_table(hal, big, what, 10, 40, seed=D, rows=D)
    assert rows == D and "image_list" in prof and not np.array_equal(got[8:16], big[1][8:16])


def test_every_leaf_dirty(hal, big):
    """D = L = 2^19: whichever route the rule picks for a table as wide as the leaf layer, the nodes agree"""
    prof, got, D = _run_table(hal, big, "all", 20, 1994)
    assert D == 1 << 19 and "image_leaves" in prof


# ---- refusals ----
def test_a_refused_page_out_leaves_image_and_nodes_unchanged(hal):
    po2, zk = 10, 300
    n = 1 << po2
    desc, blob, code, data, image = pc.case("two", 41, po2, zk)
    args = logup.Arguments.parse(blob)
    c = _circuit(hal, desc, blob)
    W = len(image)
    full = logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1), image=image).reshape(-1, n)
    dimage = _image(hal, image)
    nodes = hal.image_commit(dimage)
    tree = nodes.to_vec()
    for edits, words in ([(pc.P_ADDR, 30, full[pc.P_ADDR, 29])], "does not follow a smaller one"), ([(pc.P_ADDR, 49, pc.enc(W))], f"address {W} outside the image"), \
                        ([(pc.P_ON, 30, pc.enc(2) + np.uint32(P))], "p_on 2, not 0 or 1"):
        bad = full.copy()
        for col, row, v in edits:
            bad[col, row] = v
        with pytest.raises(logup.ReferenceError, match=re.escape(words)) as e:
            logup.reference_page_out(args, po2, zk, bad.reshape(-1), image)
        ddata = hal.copy_from("data", bad.reshape(-1))
        message = re.escape("page_out: " + str(e.value) + ": the image is unchanged")
        with pytest.raises(HalError, match=message):
            hal.page_out(c, po2, zk, ddata, dimage)
        with pytest.raises(HalError, match=message):
            hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)
        assert np.array_equal(dimage.to_vec(), image) and np.array_equal(nodes.to_vec(), tree)
    ddata = hal.copy_from("data", full.reshape(-1))
    for size in (tree.size // 2, tree.size * 2, tree.size - 8):               # a wrong-sized `nodes`: refused before anything is written
        wrong = hal.alloc_elem("nodes", size)
        with pytest.raises(HalError, match=f"page_out: nodes of {size} words; an image of {W} words has a tree of {tree.size}"):
            hal.page_out_tree(c, po2, zk, ddata, dimage, wrong)
        assert np.array_equal(dimage.to_vec(), image)
    plain = _circuit(hal, desc, args.plain().blob())
    with pytest.raises(HalError, match="page_out: the circuit's arguments hold no PAGES record"):
        hal.page_out_tree(plain, po2, zk, ddata, dimage, nodes)
    hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)                      # and the table that was derived passes
    assert np.array_equal(nodes.to_vec(), logup.reference_image_tree(dimage.to_vec()).reshape(-1))


# ---- determinism and the prover ----
def test_the_same_call_twice_gives_identical_nodes(hal, big):
    first = _run_table(hal, big, "spread", 13, 1994, seed=9)[1]
    again = _run_table(hal, big, "spread", 13, 1994, seed=9)[1]
    assert np.array_equal(first, again)


def test_a_seal_that_pages_out_through_the_tree(hal):
    po2, zk, W = 8, 40, 64
    desc, blob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True, reads=True, pages=True)
    image = np.random.default_rng(po2).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, full, out = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=W, link=True, reads=True, pages=True, image=image)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=W, count=False, limbs=False, link=False, reads=True, pages=False, image=image)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    plain_image, tree_image = _image(hal, image), _image(hal, image)
    tree = hal.image_commit(tree_image)
    without = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out, image=plain_image, page_out=True)
    with_tree = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out, image=tree_image, page_out=True, tree=tree)
    assert np.array_equal(with_tree.seal, without.seal)
    image1 = logup.reference_page_out(logup.Arguments.parse(blob), po2, zk, full, image)
    assert not np.array_equal(image1, image)
    assert np.array_equal(plain_image.to_vec(), image1) and np.array_equal(tree_image.to_vec(), image1)
    assert np.array_equal(tree.to_vec(), logup.reference_image_tree(image1).reshape(-1))
    assert np.array_equal(hal.image_root(tree), logup.reference_image_root(image1))
