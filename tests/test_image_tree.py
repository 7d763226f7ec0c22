"""The image's commitment on the host (logup.reference_image_tree, reference_image_root; include/zkhal.h "THE IMAGE'S COMMITMENT"): the
definition the device tree (zkh_image_commit, zkh_page_out_tree; tests/test_image_tree_gpu.py) is held to.  The tree is a function of the
residues of the image's raw Montgomery words: leaves are eight words verbatim, zero-padded, every node above is hash_pair of its two
children, the root is digest 1.  One path per image is recomputed with the oracle's zko_hash_pair, which shares nothing with the
library's host permutation."""
import numpy as np
import pytest

from zeth_amd import host
from zeth_amd.circuits import logup

P = 2013265921


def _image(W, seed, big=False):
    rng = np.random.default_rng(seed)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    if big:                                                                  # about a third of the words as raw words >= P
        image[(rng.random(W) < 0.35) & (image < np.uint32(2 ** 32 - P))] += np.uint32(P)
    return image


def _oracle_path(oracle, nodes, leaf):
    """the root from leaf `leaf` of `nodes` up its path, every step the oracle's hash_pair of the node and its sibling"""
    L = len(nodes) // 2
    i = L + leaf
    cur = np.ascontiguousarray(nodes[i])
    while i > 1:
        sib, nxt = np.ascontiguousarray(nodes[i ^ 1]), np.zeros(8, dtype=np.uint32)
        if i & 1:
            oracle.zko_hash_pair(sib, cur, nxt)
        else:
            oracle.zko_hash_pair(cur, sib, nxt)
        cur, i = nxt, i >> 1
        assert np.array_equal(cur, nodes[i]), i
    return cur


def test_two_leaves_are_one_hash_pair(oracle):
    image = _image(16, 1, big=True)
    nodes = logup.reference_image_tree(image)
    assert nodes.shape == (4, 8) and nodes.dtype == np.uint32 and not nodes[0].any()
    assert np.array_equal(nodes[2], image[:8] % P) and np.array_equal(nodes[3], image[8:] % P)
    assert np.array_equal(nodes[1], host.hash_pair(image[:8] % P, image[8:] % P))
    assert np.array_equal(logup.reference_image_root(image), nodes[1])
    assert np.array_equal(_oracle_path(oracle, nodes, 1), nodes[1])


@pytest.mark.parametrize("W", [1, 8])
def test_one_leaf_is_the_root(W):
    image = _image(W, W)
    nodes = logup.reference_image_tree(image)
    assert nodes.shape == (2, 8) and not nodes[0].any()
    assert np.array_equal(nodes[1], np.concatenate([image, np.zeros(8 - W, dtype=np.uint32)]))
    assert np.array_equal(logup.reference_image_root(image), nodes[1])


def test_a_partial_last_leaf_is_zero_padded():
    image = _image(9, 9)
    nodes = logup.reference_image_tree(image)
    assert nodes.shape == (4, 8)
    assert np.array_equal(nodes[2], image[:8]) and nodes[3, 0] == image[8] and not nodes[3, 1:].any()
    assert np.array_equal(nodes[1], host.hash_pair(nodes[2], nodes[3]))


def test_the_leaf_count_is_the_next_power_of_two(oracle):
    for W, L in [(1024, 128), (1025, 256)]:
        image = _image(W, W)
        nodes = logup.reference_image_tree(image)
        assert nodes.shape == (2 * L, 8) and logup.image_tree_leaves(W) == L
        assert np.array_equal(nodes[L:].reshape(-1)[:W], image) and not nodes[L:].reshape(-1)[W:].any()
        for i in (1, L // 2 + 3, L - 1):
            assert np.array_equal(nodes[i], host.hash_pair(nodes[2 * i], nodes[2 * i + 1])), (W, i)
        # W = 1025: leaf 128 is the partial one, leaves 129 .. 255 are padding; a path through each side
        for leaf in (0, (W - 1) // 8, L - 1):
            assert np.array_equal(_oracle_path(oracle, nodes, leaf), nodes[1])
    with pytest.raises(logup.ReferenceError, match="an image of 0 words"):
        logup.reference_image_tree(np.zeros(0, dtype=np.uint32))


def test_raw_words_above_p_have_the_root_of_their_residues(oracle):
    image = _image(1000, 3, big=True)
    assert (image >= P).sum() > 200
    nodes = logup.reference_image_tree(image)
    assert np.array_equal(nodes, logup.reference_image_tree(image % P))
    assert (nodes < P).all()
    assert np.array_equal(_oracle_path(oracle, nodes, 77), nodes[1])
    lifted = image % P
    lifted[lifted < np.uint32(2 ** 32 - P)] += np.uint32(P)                  # every word that has one as its other raw word
    assert np.array_equal(logup.reference_image_root(lifted), nodes[1])


def test_one_word_changes_exactly_its_path():
    W = 1000
    image = _image(W, 4)
    nodes = logup.reference_image_tree(image)
    L = len(nodes) // 2
    for a in (0, 517, W - 1):
        other = image.copy()
        other[a] = (int(other[a]) + 1) % P
        changed = set(np.nonzero((logup.reference_image_tree(other) != nodes).any(axis=1))[0].tolist())
        path, i = set(), L + a // 8
        while i >= 1:
            path.add(i)
            i >>= 1
        assert changed == path, a
    same = image.copy()
    same[517] += np.uint32(P) if same[517] < 2 ** 32 - P else 0             # the other raw word of the same residue: no node changes
    assert np.array_equal(logup.reference_image_tree(same), nodes)
