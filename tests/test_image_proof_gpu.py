"""The update's proof on the GPU (zkh_page_out_proof; csrc/image.hip, the check pass of csrc/page_out.hip): the ZKU1 proof built on the
device equals logup.reference_page_out_proof word for word, the reference reading the `nodes` that the device committed; the call leaves
data, image and nodes as they were, writes no word past the proof's length, and the host verifier (zkh_image_proof_verify) walks the
proof from the root before to the root that zkh_page_out_tree leaves.

Through the real derive: every kind of pages_cases at two sizes.  Hand-made tables (p_on, p_addr, p_in = the image's word, p_out) over the
image of 2^22 - 3 words (L = 2^19: for more than 1024 rows nine layers of three launches each, then the top kernel), over 8189 words (L = 2^10: the whole tree
inside the top kernel), over 9 words (h = 1) and 8 words (L = 1: no layer); and the seam tables of pages_cases over 4096 words (L = 512), whose
rows 255 and 256 put a head decision of the leaf compaction on the seam between two workgroups.

Mutants these cases are meant to catch:
  * a carry dropped at a scan-workgroup boundary, in either run of the packed scan: `spread` and `twins` on the big image (24 workgroups);
  * the two packed counts mixed up, or a count of 256 overflowing its half: `spread` (a full workgroup of clean siblings) and `all` (a
    full workgroup of heads and none clean);
  * a sibling taken from the layer above or below, or the node itself instead of its sibling: every table but `none`;
  * both children dirty but a sibling emitted all the same: `twins` (leaf layer and the layer above), `all` (every layer);
  * the first item odd with nothing before it, the last even with nothing after it: `edges`;
  * the new leaf in place of the old one, or residues forgotten: every table (a third of the image, p_in and p_out are raw words >= P);
  * a section's offset that skips a layer without clean siblings: `edges` (c = 0 at the top), `all`;
  * the hand-over from the listed layers to the top kernel (count, offset, which of the two lists): every table on the big image."""
import re

import numpy as np
import pytest

import pages_cases as pc
from args_gpu import circuit as _circuit, image_buf as _image, profiled, upload as _upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
ONE = (1 << 32) % P
POISON = 0xDEADBEEF
SLACK = 40                                                                   # poisoned words past the bound
TINY = syn_lookup.TINY
BIG_W = (1 << 22) - 3                                                        # L = 2^19
SCOPES = {"proof_table", "proof_leaves", "proof_layer", "proof_top"}


def _words(rng, size, big=True):
    """random non-zero residues, a third of them as the raw word >= P of the same residue"""
    w = rng.integers(1, P, size, dtype=np.uint64).astype(np.uint32)
    if big:
        w[rng.random(size) < 0.33] += np.uint32(P)
    return w


def _small_case():
    return pc.case("range5", 3, 8, 40)[:2]


def _proof(hal, c, po2, zk, ddata, dimage, dnodes, W):
    """page_out_proof into a poisoned buffer of the bound for every active row plus SLACK -> (the proof, the profile); nothing past the
    proof's length is written"""
    bound = hal.image_proof_words(W, (1 << po2) - zk)
    buf = hal.copy_from("proof", np.full(bound + SLACK, POISON, dtype=np.uint32))
    got = []
    prof = profiled(hal, lambda: got.append(hal.page_out_proof(c, po2, zk, ddata, dimage, dnodes, proof=buf)))
    proof = got[0]
    whole = buf.to_vec()
    assert np.array_equal(whole[:proof.size], proof) and (whole[proof.size:] == POISON).all(), "words past the proof's length were written"
    return proof, prof


def _same(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} words, the reference has {want.size}; headers {got[:5 + int(want[4])]} / {want[:5 + int(want[4])]}"
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, the first at {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"


# ---- through the real derive ----
@pytest.mark.parametrize("po2,zk", [(8, 40), (12, 1994)])
def test_the_proof_of_a_derived_table(hal, po2, zk):
    for i, kind in enumerate(pc.KINDS):
        desc, blob, code, data, image0 = pc.case(kind, 200 * po2 + i, po2, zk)
        args = logup.Arguments.parse(blob)
        W = len(image0)
        c = _circuit(hal, desc, blob)
        dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
        dimage = _image(hal, image0)
        nodes = hal.image_commit(dimage)
        hal.derive_links_paged(c, po2, zk, dcode, ddata, dimage)
        full, before = ddata.to_vec(), nodes.to_vec()
        proof, prof = _proof(hal, c, po2, zk, ddata, dimage, nodes, W)
        _same(proof, logup.reference_page_out_proof(args, po2, zk, full, W, before), kind)
        assert int(proof[2]) > 0 and "proof_top" in prof and "proof_layer" not in prof, kind
        assert np.array_equal(ddata.to_vec(), full) and np.array_equal(dimage.to_vec(), image0) and np.array_equal(nodes.to_vec(), before), kind
        hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)
        assert np.array_equal(nodes.to_vec(), hal.image_commit(dimage).to_vec()), kind
        after = zhal.image_proof_verify(proof, before[8:16])
        assert np.array_equal(after, hal.image_root(nodes)) and not np.array_equal(after, before[8:16]), kind
        assert np.array_equal(after, logup.check_page_out_proof(proof, before[8:16])), kind


# ---- hand-made tables ----
@pytest.fixture(scope="module")
def images(hal):
    """W -> (image, nodes): a third of the words raw words >= P, the nodes committed on the device and read back once; the tests upload
    their own copies"""
    out = {}
    for W in (BIG_W, 8189, 4096, 9, 8):
        image = _words(np.random.default_rng(W), W)
        out[W] = (image, hal.image_commit(_image(hal, image)).to_vec())
    return out


def _table(po2, image, addrs, out):
    """a data trace of zeros but for the page table's p_on, p_addr, p_in (the image's raw word) and p_out on its first len(addrs) rows"""
    data = np.zeros((pc.PAGED_W + 1, 1 << po2), dtype=np.uint32)
    D = len(addrs)
    data[pc.P_ON, :D], data[pc.P_ADDR, :D], data[pc.P_IN, :D], data[pc.P_OUT, :D] = ONE, pc.enc(addrs), image[addrs], out
    return data.reshape(-1)


def _addresses(what, W, A, rng, rows=None):
    L = logup.image_tree_leaves(W)
    if what in pc.SEAM_TABLES:
        return pc.seam_table(what, rows, W, rng)
    if what == "spread":
        return np.sort(rng.choice(W, min(A, 3 * W // 4), replace=False)).astype(np.int64)
    if what == "twins":                                                      # 8 j and 8 j + 7 of the leaves 2 q and 2 q + 1
        q = np.sort(rng.choice(L // 2 - 1, min(A // 4, L // 4), replace=False)).astype(np.int64)
        leaves = np.stack([2 * q, 2 * q + 1], axis=1).reshape(-1)
        return np.stack([8 * leaves, 8 * leaves + 7], axis=1).reshape(-1)
    if what == "edges":
        return np.array([0, W - 1], dtype=np.int64)
    if what == "one":
        return np.array([(W * 1234567) // BIG_W], dtype=np.int64)
    if what == "none":
        return np.zeros(0, dtype=np.int64)
    assert what == "all"
    return 8 * np.arange(L, dtype=np.int64)


def _run_table(hal, images, W, what, po2, zk, seed=5, walk=True, rows=None):
    image0, nodes0 = images[W]
    A = (1 << po2) - zk
    rng = np.random.default_rng(seed)
    addrs = _addresses(what, W, A, rng, rows)
    D = len(addrs)
    assert D <= A and (D < 2 or (np.diff(addrs) > 0).all()) and (D == 0 or addrs[-1] < W)
    out = _words(rng, D)
    desc, blob = _small_case()
    c = _circuit(hal, desc, blob)
    data = _table(po2, image0, addrs, out)
    ddata = hal.copy_from("data", data)
    dimage, nodes = _image(hal, image0), hal.copy_from("nodes", nodes0)
    proof, prof = _proof(hal, c, po2, zk, ddata, dimage, nodes, W)
    _same(proof, logup.reference_page_out_proof(logup.Arguments.parse(blob), po2, zk, data, W, nodes0), f"{what} over {W}")
    assert np.array_equal(ddata.to_vec(), data) and np.array_equal(dimage.to_vec(), image0) and np.array_equal(nodes.to_vec(), nodes0)
    hal.page_out_tree(c, po2, zk, ddata, dimage, nodes)                      # the proof left the tree fit for its update
    assert np.array_equal(nodes.to_vec(), hal.image_commit(dimage).to_vec())
    if walk:
        assert np.array_equal(zhal.image_proof_verify(proof, nodes0[8:16]), hal.image_root(nodes))
    h = int(proof[4])
    return proof, prof, [int(x) for x in proof[5:5 + h]]


@pytest.mark.parametrize("what", ["spread", "twins", "edges", "one", "none"])
def test_a_hand_made_table_over_the_big_image(hal, images, what):
    proof, prof, c = _run_table(hal, images, BIG_W, what, 13, 1994)
    D, M, h = int(proof[2]), int(proof[3]), int(proof[4])
    assert h == 19 and len(c) == 19
    if what == "none":
        assert D == 0 and proof.size == 5 + 19 and not SCOPES & set(prof), set(prof)
        return
    assert {"proof_table", "proof_leaves", "proof_top"} <= set(prof) and prof["proof_top"]["calls"] == 1, prof
    if what in ("spread", "twins"):                                          # nine layers of up to D items, then lists that fit the top kernel
        assert prof["proof_layer"]["calls"] == 9, prof
    else:                                                                    # a list of two items fits it from the leaves up
        assert "proof_layer" not in prof, prof
    if what == "spread":
        assert D == 6198 and M > 6100 and c[0] > 6000
    if what == "twins":
        assert D == 4 * (6198 // 4) and M == D // 2 and c[0] == 0 and M // 2 - 60 < c[1] <= M // 2      # a few of the random pairs are siblings themselves
    if what == "edges":
        assert (D, M) == (2, 2) and c == [2] * 18 + [0]
    if what == "one":
        assert (D, M) == (1, 1) and c == [1] * 19 and proof.size == hal.image_proof_words(BIG_W, 1)


def test_every_leaf_dirty(hal, images):
    """D = L = 2^19 at po2 20: no clean sibling on any layer.  Compared with the reference only: the host walk of 2^20 nodes is skipped
    (two host permutations per node; the walk has the other tables)"""
    proof, prof, c = _run_table(hal, images, BIG_W, "all", 20, 1994, walk=False)
    assert int(proof[2]) == int(proof[3]) == 1 << 19 and c == [0] * 19 and proof.size == 5 + 19 + 11 * (1 << 19)
    assert SCOPES <= set(prof)


@pytest.mark.parametrize("what", ["spread", "twins", "edges", "one", "none"])
def test_a_tree_inside_the_top_kernel(hal, images, what):
    proof, prof, c = _run_table(hal, images, 8189, what, 13, 1994)
    assert int(proof[4]) == 10
    if what == "none":
        assert not SCOPES & set(prof)
        return
    assert {"proof_table", "proof_leaves", "proof_top"} <= set(prof) and "proof_layer" not in prof, set(prof)
    if what == "spread":
        assert int(proof[2]) == 6141 and int(proof[3]) > 1000
    if what == "edges":
        assert c == [2] * 9 + [0]
    if what == "one":
        assert c == [1] * 10


@pytest.mark.parametrize("D", pc.SEAM_ROWS)
@pytest.mark.parametrize("what", pc.SEAM_TABLES)
def test_a_head_on_the_seam_of_two_workgroups(hal, images, what, D):
    """rows 255 and 256 share a leaf, lie in sibling leaves, or lie under different parents: lane 0 of the second workgroup is no head
    of the leaf list, or one; 984 active rows"""
    proof, prof, c = _run_table(hal, images, 4096, what, 10, 40, seed=D, rows=D)
    assert [int(x) for x in proof[1:3]] == [4096, D] and int(proof[4]) == 9 and {"proof_table", "proof_leaves", "proof_top"} <= set(prof)
    if D == 257:                                                             # the two rows of the seam: one leaf, or two
        assert int(proof[3]) == (256 if what == "seam_leaf" else 257)


@pytest.mark.parametrize("W", [9, 8])
@pytest.mark.parametrize("what", ["spread", "edges", "one", "none"])
def test_one_layer_and_none(hal, images, W, what):
    proof, prof, c = _run_table(hal, images, W, what, 8, 40)
    assert int(proof[4]) == (1 if W == 9 else 0) and "proof_layer" not in prof
    assert ("proof_top" in prof) == (W == 9 and what != "none")
    if what == "one" and W == 9:
        assert c == [1]


# ---- refusals ----
def test_refusals_leave_image_and_nodes_unchanged(hal):
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
    D = int((pc.dec(full[pc.P_ON, :n - zk]) == 1).sum())
    assert D > 49
    roomy = hal.alloc_elem("proof", hal.image_proof_words(W, n - zk))
    off_by_one = np.uint32((int(full[pc.P_IN, 30]) % P + 1) % P)
    for edits, words in ([(pc.P_ADDR, 30, full[pc.P_ADDR, 29])], "does not follow a smaller one"), ([(pc.P_ADDR, 49, pc.enc(W))], f"address {W} outside the image"), \
                        ([(pc.P_ON, 30, pc.enc(2) + np.uint32(P))], "p_on 2, not 0 or 1"), ([(pc.P_IN, 30, off_by_one)], "at row 30: p_in "):
        bad = full.copy()
        for col, row, v in edits:
            bad[col, row] = v
        with pytest.raises(logup.ReferenceError, match=re.escape(words)) as e:
            logup.reference_page_out_proof(args, po2, zk, bad.reshape(-1), W, tree)
        ddata = hal.copy_from("data", bad.reshape(-1))
        with pytest.raises(HalError) as f:
            hal.page_out_proof(c, po2, zk, ddata, dimage, nodes, proof=roomy)
        assert str(f.value) == "page_out_proof: " + str(e.value)
        assert np.array_equal(dimage.to_vec(), image) and np.array_equal(nodes.to_vec(), tree)
    assert ", the tree holds " in str(e.value)
    ddata = hal.copy_from("data", full.reshape(-1))
    for size in (tree.size // 2, tree.size * 2, tree.size - 8):               # a wrong-sized `nodes`: refused before any launch
        wrong = hal.alloc_elem("nodes", size)
        with pytest.raises(HalError, match=f"page_out_proof: nodes of {size} words; an image of {W} words has a tree of {tree.size}"):
            hal.page_out_proof(c, po2, zk, ddata, dimage, wrong, proof=roomy)
    bound = hal.image_proof_words(W, D)                                      # for the actual D, and the message names it
    with pytest.raises(HalError, match=f"page_out_proof: a proof buffer of {bound - 1} words; {D} pages over an image of {W} words take up to {bound} "):
        hal.page_out_proof(c, po2, zk, ddata, dimage, nodes, proof=hal.alloc_elem("proof", bound - 1))
    plain = _circuit(hal, desc, args.plain().blob())
    with pytest.raises(HalError, match="page_out_proof: the circuit's arguments hold no PAGES record"):
        hal.page_out_proof(plain, po2, zk, ddata, dimage, nodes, proof=roomy)
    assert np.array_equal(dimage.to_vec(), image) and np.array_equal(nodes.to_vec(), tree)
    exact = hal.page_out_proof(c, po2, zk, ddata, dimage, nodes, proof=hal.alloc_elem("proof", bound))     # and the bound itself is enough
    _same(exact, logup.reference_page_out_proof(args, po2, zk, full.reshape(-1), W, tree), "two")
    assert np.array_equal(exact, hal.page_out_proof(c, po2, zk, ddata, dimage, nodes))


# ---- determinism and the prover ----
def test_the_same_call_twice_gives_identical_words(hal, images):
    first = _run_table(hal, images, BIG_W, "spread", 13, 1994, seed=9, walk=False)[0]
    again = _run_table(hal, images, BIG_W, "spread", 13, 1994, seed=9, walk=False)[0]
    assert np.array_equal(first, again)


def test_the_prover_returns_a_proof_from_the_old_root_to_the_new(hal):
    po2, zk, W = 8, 40, 64
    desc, blob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True, reads=True, pages=True)
    image = np.random.default_rng(po2).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, full, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=W, link=True, reads=True, pages=True, image=image)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=W, count=False, limbs=False, link=False, reads=True, pages=False, image=image)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=0x0C07)
    prover = SegmentProver(hal, desc, arguments=blob)
    dcode, ddata = _upload(hal, np.ascontiguousarray(code).reshape(-1), np.ascontiguousarray(bare).reshape(-1))
    dimage = _image(hal, image)
    tree = hal.image_commit(dimage)
    root0 = hal.image_root(tree)
    hal.derive_all_paged(prover.circuit, po2, zk, dcode, ddata, dimage)
    with pytest.raises(HalError, match="proof=True needs the image's committed tree"):
        prover.page_out(seg, ddata, dimage, proof=True)
    assert np.array_equal(dimage.to_vec(), image)
    proof = prover.page_out(seg, ddata, dimage, tree=tree, proof=True)
    image1 = logup.reference_page_out(logup.Arguments.parse(blob), po2, zk, full, image)
    assert not np.array_equal(image1, image) and np.array_equal(dimage.to_vec(), image1)
    root1 = zhal.image_proof_verify(proof, root0)
    assert np.array_equal(root1, hal.image_root(tree)) and np.array_equal(root1, logup.reference_image_root(image1))
    assert np.array_equal(root1, logup.check_page_out_proof(proof, root0))
    assert prover.page_out(seg, ddata, dimage, tree=tree) is None            # without proof=True nothing is returned
