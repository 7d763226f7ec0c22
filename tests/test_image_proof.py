"""The update's proof on the host (include/zkhal.h "THE UPDATE'S PROOF", ZKU1): logup.reference_page_out_proof builds the proof of a page
table from the nodes of logup.reference_image_tree, and both verifiers, logup.check_page_out_proof (numpy) and the library's
zkh_image_proof_verify (hal.image_proof_verify: host only), walk it from the old root to the root of the paged-out image with nothing
else in hand.  Every refusal of the verifier has its mutation, refused by both with the same words."""
import ctypes as C

import numpy as np
import pytest

import pages_cases as pc
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup

P = 2013265921
ONE = (1 << 32) % P
PO2 = 11                                                                     # the hand-made tables: up to 1025 rows, no blinding rows
MAGIC = 0x5A4B5531


def _words(rng, size, big=False):
    w = rng.integers(1, P, size, dtype=np.uint64).astype(np.uint32)
    if big:
        w[rng.random(size) < 0.33] += np.uint32(P)
    return w


@pytest.fixture(scope="module")
def args():
    return logup.Arguments.parse(pc.case("range5", 3, 8, 40)[1])


def _table(image, addrs, out, po2=PO2):
    """a data trace of zeros but for the page table: p_on, p_addr, p_in = the image's word, p_out on its first len(addrs) rows"""
    data = np.zeros((pc.PAGED_W + 1, 1 << po2), dtype=np.uint32)
    D = len(addrs)
    data[pc.P_ON, :D], data[pc.P_ADDR, :D], data[pc.P_IN, :D], data[pc.P_OUT, :D] = ONE, pc.enc(addrs), image[addrs], out
    return data.reshape(-1)


def _addresses(what, W, rng):
    L = logup.image_tree_leaves(W)
    if what == "none":
        return np.zeros(0, dtype=np.int64)
    if what == "one":
        return np.array([W // 2], dtype=np.int64)
    if what == "five":
        return np.sort(rng.choice(W, min(5, W), replace=False)).astype(np.int64)
    if what == "all":
        return np.arange(W, dtype=np.int64)
    if what == "edges":
        return np.unique(np.array([0, W - 1], dtype=np.int64))
    assert what == "twins"                                                   # 8 j and 8 j + 7 of the leaves 2 q and 2 q + 1 (whole leaves only)
    q = np.sort(rng.choice(max(W // 16, 1), min(3, max(W // 16, 1)), replace=False)).astype(np.int64)
    leaves = np.stack([2 * q, 2 * q + 1], axis=1).reshape(-1)
    a = np.stack([8 * leaves, 8 * leaves + 7], axis=1).reshape(-1)
    return a[a < W]


def _both(proof, root):
    """root_after from both verifiers, which must agree"""
    a, b = logup.check_page_out_proof(proof, root), zhal.image_proof_verify(proof, root)
    assert np.array_equal(a, b) and a.dtype == np.uint32 and a.shape == (8,)
    return a


def _counts(proof):
    h = int(proof[4])
    return [int(x) for x in proof[5:5 + h]]


def _case(args, W, what, seed=0, big=False):
    rng = np.random.default_rng(1000 * W + seed)
    image = _words(rng, W, big)
    addrs = _addresses(what, W, rng)
    out = _words(rng, len(addrs), big)
    nodes = logup.reference_image_tree(image)
    proof = logup.reference_page_out_proof(args, PO2, 0, _table(image, addrs, out), W, nodes)
    after = image.copy()
    after[addrs] = out
    return image, addrs, out, nodes, proof, after


@pytest.mark.parametrize("W", [1, 7, 8, 9, 650, 1000, 1025])
@pytest.mark.parametrize("what", ["none", "one", "five", "all", "twins", "edges"])
def test_both_verifiers_reach_the_root_of_the_paged_out_image(args, W, what):
    image, addrs, out, nodes, proof, after = _case(args, W, what)
    D, L = len(addrs), logup.image_tree_leaves(W)
    h = L.bit_length() - 1
    assert proof.dtype == np.uint32 and proof[0] == MAGIC and list(proof[1:3]) == [W, D] and proof[4] == h
    M, c = int(proof[3]), _counts(proof)
    assert M == len(np.unique(addrs >> 3))
    assert proof.size == 5 + h + 3 * D + 8 * M + 8 * sum(c)
    bound = logup.image_proof_words(W, D)
    assert proof.size <= bound == zhal.load_library().zkh_image_proof_words(W, D)
    if D == 1 or W <= 8:
        assert proof.size == bound, (proof.size, bound)
    if D == 0:
        assert proof.size == 5 + h
    if what == "all":                                                        # every leaf that holds a word is dirty: only padding is clean
        assert M == (W + 7) // 8 and (any(c) == (M < L))
    assert np.array_equal(_both(proof, nodes[1]), logup.reference_image_root(after))
    assert np.array_equal(_both(proof, nodes[1]), logup.reference_image_tree(after)[1])


@pytest.mark.parametrize("D", pc.SEAM_ROWS)
@pytest.mark.parametrize("what", pc.SEAM_TABLES)
def test_both_verifiers_walk_the_seam_tables(args, what, D):
    """rows 255 and 256 on the seam between two workgroups of the device's kernels (pages_cases.seam_table), W = 4096 (L = 512, h = 9):
    the proofs the GPU modules compare against pass both host verifiers first"""
    W = 4096
    rng = np.random.default_rng(D + len(what))
    image = _words(rng, W, big=True)
    addrs = pc.seam_table(what, D, W, rng)
    out = _words(rng, D, big=True)
    nodes = logup.reference_image_tree(image)
    proof = logup.reference_page_out_proof(args, PO2, 0, _table(image, addrs, out), W, nodes)
    assert list(proof[1:5]) == [W, D, len(np.unique(addrs >> 3)), 9]
    image[addrs] = out
    assert np.array_equal(_both(proof, nodes[1]), logup.reference_image_root(image))


def test_raw_words_above_p_give_the_proof_of_their_residues(args):
    W = 1000
    image, addrs, out, nodes, proof, after = _case(args, W, "five", seed=7, big=True)
    assert (image >= P).sum() > 200
    lifted = image[addrs].copy()
    lifted[lifted < P] += np.uint32(P)
    assert (lifted >= P).all()
    data = _table(image, addrs, out).reshape(-1, 1 << PO2)
    data[pc.P_IN, :len(addrs)] = lifted
    other = out % np.uint32(P) + np.uint32(P)
    data[pc.P_OUT, :len(addrs)] = other
    again = logup.reference_page_out_proof(args, PO2, 0, data.reshape(-1), W, logup.reference_image_tree(image % P))
    assert np.array_equal(again, proof) and (proof[5 + int(proof[4]):] < np.uint32(P)).all()
    assert np.array_equal(_both(proof, nodes[1]), logup.reference_image_root(after))


def test_pinned_counts(args):
    proof = _case(args, 650, "one")[4]
    assert int(proof[4]) == 7 and _counts(proof) == [1] * 7
    proof = _case(args, 8189, "edges")[4]
    assert int(proof[4]) == 10 and _counts(proof) == [2, 2, 2, 2, 2, 2, 2, 2, 2, 0]
    assert list(proof[2:4]) == [2, 2]


# ---- mutations: one per refusal ----
@pytest.fixture(scope="module")
def good(args):
    """W = 650 (h = 7), 5 spread rows plus two rows in one leaf: (proof, root_before, root_after, layout)"""
    rng = np.random.default_rng(650)
    W = 650
    image = _words(rng, W)
    addrs = np.array([3, 4, 100, 101 + 8, 333, 500, 649], dtype=np.int64)
    out = _words(rng, len(addrs))
    nodes = logup.reference_image_tree(image)
    proof = logup.reference_page_out_proof(args, PO2, 0, _table(image, addrs, out), W, nodes)
    after = _both(proof, nodes[1])
    image[addrs] = out
    assert np.array_equal(after, logup.reference_image_root(image))
    h, D, M = int(proof[4]), int(proof[2]), int(proof[3])
    t0 = 5 + h
    return proof, nodes[1].copy(), after, {"t0": t0, "l0": t0 + 3 * D, "s0": t0 + 3 * D + 8 * M, "D": D, "M": M, "h": h, "addrs": addrs}


def _refused(proof, root, words):
    """both verifiers refuse with the same message, which holds `words`; the C verifier leaves root_after untouched"""
    with pytest.raises(logup.ReferenceError) as e:
        logup.check_page_out_proof(proof, root)
    assert words in str(e.value), str(e.value)
    with pytest.raises(zhal.HalError) as f:
        zhal.image_proof_verify(proof, root)
    assert str(f.value) == "image_proof_verify: " + str(e.value)
    lib = zhal.load_library()
    pf, rb = np.ascontiguousarray(proof, dtype=np.uint32), np.ascontiguousarray(root, dtype=np.uint32)
    after = np.full(8, 0xdeadbeef, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    err = lib.zkh_image_proof_verify(pf.ctypes.data_as(u32p), pf.size, rb.ctypes.data_as(u32p), after.ctypes.data_as(u32p))
    assert err
    lib.zkh_free_error(err)
    assert (after == 0xdeadbeef).all()
    return str(e.value)


def _bump(word):
    return np.uint32((int(word) + 1) % P)


def test_a_flipped_sibling_word_opens_another_root(good):
    proof, root, _, at = good
    for off in (at["s0"], at["s0"] + 11, proof.size - 1):
        bad = proof.copy()
        bad[off] = _bump(bad[off])
        _refused(bad, root, "not root_before")


def test_a_flipped_unpaged_leaf_word_opens_another_root(good):
    proof, root, _, at = good
    bad = proof.copy()
    assert at["addrs"][0] == 3
    bad[at["l0"] + 6] = _bump(bad[at["l0"] + 6])                             # word 6 of leaf 0: rows 0 and 1 page its words 3 and 4
    _refused(bad, root, "not root_before")


def test_a_wrong_in_is_refused(good):
    proof, root, _, at = good
    bad = proof.copy()
    bad[at["t0"] + 3 * 2 + 1] = _bump(bad[at["t0"] + 3 * 2 + 1])
    msg = _refused(bad, root, "row 2: in ")
    assert f"at address 100, but its leaf holds {int(proof[at['t0'] + 7])}" in msg


def test_a_swapped_pair_of_rows_is_refused(good):
    proof, root, _, at = good
    bad = proof.copy()
    r3, r4 = at["t0"] + 9, at["t0"] + 12
    bad[r3:r3 + 3], bad[r4:r4 + 3] = proof[r4:r4 + 3], proof[r3:r3 + 3]
    _refused(bad, root, "row 4: address 109 does not follow a smaller one (row 3: address 333)")
    bad = proof.copy()
    bad[at["t0"] + 3 * 6] = 650
    _refused(bad, root, "row 6: address 650 outside the image of 650 words")


@pytest.mark.parametrize("step", [1, -1])
def test_a_wrong_sibling_count_is_refused(good, step):
    proof, root, _, at = good
    c = _counts(proof)
    k = next(k for k in range(at["h"]) if c[k] >= 1 and k >= 2)
    j = next(j for j in range(at["h"]) if j != k and c[j] >= 1)
    bad = proof.copy()                                                       # the length stays what the header describes
    bad[5 + k], bad[5 + j] = c[k] + step, c[j] - step
    first = min(k, j)
    moved = step if first == k else -step
    _refused(bad, root, f"layer {first}: {c[first] + moved} siblings, but the walk takes {c[first]}")
    alone = proof.copy()                                                     # the count alone: the length no longer fits
    alone[5 + k] = c[k] + step
    _refused(alone, root, f"a proof of {proof.size} words, but the header describes {proof.size + 8 * step}")


@pytest.mark.parametrize("step", [1, -1])
def test_a_wrong_leaf_count_is_refused(good, step):
    proof, root, _, at = good
    c = _counts(proof)
    bad = proof.copy()
    bad[3], bad[5] = at["M"] + step, c[0] - step
    assert c[0] >= 1
    _refused(bad, root, f"M {at['M'] + step}, but the table's rows lie in {at['M']} leaves")


def test_a_truncated_or_extended_blob_is_refused(good):
    proof, root, _, at = good
    _refused(proof[:-1], root, f"a proof of {proof.size - 1} words, but the header describes {proof.size}")
    _refused(np.concatenate([proof, proof[-1:]]), root, f"a proof of {proof.size + 1} words, but the header describes {proof.size}")
    _refused(proof[:4], root, "a proof of 4 words: the header alone has 5")
    _refused(proof[:8], root, "a proof of 8 words, but the header describes at least 12")


def test_a_word_plus_p_is_refused(good):
    proof, root, _, at = good
    for off in (at["t0"] + 1, at["t0"] + 5, at["l0"] + 2, at["s0"] + 9):
        bad = proof.copy()
        bad[off] += np.uint32(P)
        _refused(bad, root, f"word {off} is {int(proof[off]) + P}, not below P")


def test_a_wrong_root_before_bad_magic_and_h_are_refused(good):
    proof, root, _, at = good
    other = root.copy()
    other[5] = _bump(other[5])
    _refused(proof, other, "the proof opens root " + " ".join(f"{int(w):08x}" for w in root) + ", not root_before")
    bad = proof.copy()
    bad[0] = 0x5A4B4131
    _refused(bad, root, "bad magic 0x5a4b4131 (ZKU1 is 0x5a4b5531)")
    bad = proof.copy()
    bad[4] = 6
    _refused(bad, root, "h 6, but an image of 650 words has h 7")
    bad = proof.copy()
    bad[1] = 1025                                                            # another W with another h
    _refused(bad, root, "h 7, but an image of 1025 words has h 8")


def test_a_flipped_out_succeeds_with_another_root(good):
    """what the proof is for: whoever changes an `out` gets the root of that other memory, not a refusal"""
    proof, root, after, at = good
    bad = proof.copy()
    bad[at["t0"] + 3 * 4 + 2] = _bump(bad[at["t0"] + 3 * 4 + 2])
    other = _both(bad, root)
    assert not np.array_equal(other, after)


def test_the_builder_refuses_what_the_page_out_refuses_and_a_wrong_in(args):
    W = 650
    rng = np.random.default_rng(5)
    image = _words(rng, W)
    nodes = logup.reference_image_tree(image)
    addrs = np.array([3, 4, 100, 333], dtype=np.int64)
    data = _table(image, addrs, _words(rng, 4)).reshape(-1, 1 << PO2)
    i = args.records.index(args.pages)
    for col, row, v, words in [(pc.P_ADDR, 2, pc.enc(4), f"record {i} at row 2: page address 4 does not follow a smaller one (row 1: p_on 1, address 4)"),
                               (pc.P_ADDR, 3, pc.enc(W), f"record {i} at row 3: address {W} outside the image of {W} words"),
                               (pc.P_ON, 1, pc.enc(2), f"record {i} at row 1: p_on 2, not 0 or 1"),
                               (pc.P_IN, 2, pc.enc(9), f"record {i} at row 2: p_in 9 at address 100, the tree holds {int(pc.dec(image[100]))}")]:
        bad = data.copy()
        bad[col, row] = v
        with pytest.raises(logup.ReferenceError) as e:
            logup.reference_page_out_proof(args, PO2, 0, bad.reshape(-1), W, nodes)
        assert str(e.value) == words
        if col != pc.P_IN:                                                   # the page-out's own text is what it was
            with pytest.raises(logup.ReferenceError) as f:
                logup.reference_page_out(args, PO2, 0, bad.reshape(-1), image)
            assert str(f.value) == words
    with pytest.raises(logup.ReferenceError, match="nodes of 2032 words; an image of 650 words has a tree of 2048"):
        logup.reference_page_out_proof(args, PO2, 0, data.reshape(-1), W, nodes.reshape(-1)[:-16])


# ---- a chain of two segments ----
def test_a_verifier_with_the_first_root_follows_two_segments():
    po2, zk, kind = 8, 40, "sparse"
    A = (1 << po2) - zk
    desc, blob, code1, data1, image0 = pc.case(kind, 31, po2, zk)
    args = logup.Arguments.parse(blob)
    root0 = logup.reference_image_root(image0)
    full1 = logup.reference_links(args, po2, zk, code1.reshape(-1), data1.reshape(-1), image=image0)
    proof1 = logup.reference_page_out_proof(args, po2, zk, full1, len(image0), logup.reference_image_tree(image0))
    image1 = logup.reference_page_out(args, po2, zk, full1, image0)
    _, _, code2, data2, _ = pc.case(kind, 31, po2, zk, image=image1, trace_seed=32)
    full2 = logup.reference_links(args, po2, zk, code2.reshape(-1), data2.reshape(-1), image=image1)
    proof2 = logup.reference_page_out_proof(args, po2, zk, full2, len(image1), logup.reference_image_tree(image1))
    _, mem1 = pc.walk(code1, data1, image0, A, kind)
    _, mem2 = pc.walk(code2, data2, image0, A, kind, memory=mem1)
    final = image0.copy()
    for a, v in list(mem1.items()) + list(mem2.items()):
        final[a] = v
    root1 = _both(proof1, root0)                                             # the verifier holds root0 and the two proofs, nothing else
    root2 = _both(proof2, root1)
    assert int(proof1[2]) > 0 and int(proof2[2]) > 0 and not np.array_equal(root1, root0)
    assert np.array_equal(root2, logup.reference_image_root(final))
    with pytest.raises(logup.ReferenceError, match="not root_before"):       # the second proof does not open the first root
        logup.check_page_out_proof(proof2, root0)
