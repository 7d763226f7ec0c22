"""The dirty-node table of a page-out on the CPU (logup.reference_page_out_nodes, the numpy twin of zkh_image_proof_nodes; csrc/zkn1.h):
the twin against the two dense trees of the image before and after, at every table of page_tree_cases that has a row and at the table of
600 rows; the size function against the twin's length; and the ctypes bindings of the new calls against the header's declarations.

The yardstick is logup.reference_image_tree of the two images: it knows nothing of proofs or walks."""
import os
import re

import numpy as np
import pytest

import page_nodes_cases as nc
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_IDS = [f"{s[0]}-{s[1]}-{s[2]}-{what}" for s, what in nc.TABLES]


@pytest.mark.parametrize("s,what", nc.TABLES, ids=TABLE_IDS)
def test_the_twin_lists_every_dirty_node_once_with_its_children_from_the_dense_trees(s, what):
    t, p = nc.table(*s, what), nc.proved(*s, what)
    W, D, h, layers, words = nc.sections(p["nodes"])
    assert (W, D, h) == (t["W"], len(t["addrs"]), t["h"]) and words == p["nodes"].size and len(layers) == h
    assert np.array_equal(p["root_after"], p["after"][1])
    L = 1 << h
    dirty = set(int(a) >> 3 for a in t["addrs"])                              # the dirty nodes of layer k - 1, by their index in the layer
    for k, (ids, records) in enumerate(layers, start=1):
        want = sorted({x >> 1 for x in dirty})
        assert [int(i) for i in ids] == [(L >> k) + x for x in want], f"layer {k}: not every dirty node exactly once, in increasing id"
        for i, r in zip(ids, records):
            i = int(i)
            for c in range(2):
                old, new = r[16 * c:16 * c + 8], r[16 * c + 8:16 * c + 16]
                assert np.array_equal(old, p["before"][2 * i + c]) and np.array_equal(new, p["after"][2 * i + c]), f"layer {k}, node {i}, child {c}"
                if 2 * i + c - (L >> (k - 1)) not in dirty:
                    assert np.array_equal(old, new), f"layer {k}, node {i}: the clean child {c} has two digests"
        dirty = set(want)
    assert [int(i) for i in layers[-1][0]] == [1]


@pytest.mark.parametrize("s,what", nc.TABLES, ids=TABLE_IDS)
def test_the_size_function_bounds_the_table(s, what):
    t, p = nc.table(*s, what), nc.proved(*s, what)
    bound = logup.image_dirty_words(t["W"], len(t["addrs"]))
    assert p["nodes"].size <= bound
    assert zhal.image_dirty_words(t["W"], len(t["addrs"])) == bound
    L = 1 << t["h"]
    assert bound <= 33 * (L - 1) + t["h"] + 4


def test_the_size_function_at_its_edges():
    assert zhal.image_dirty_words(0, 5) == logup.image_dirty_words(0, 5) == 0
    for W, D in ((1, 1), (8, 3), (9, 1), (17, 0), (64, 64), (1 << 20, 662267), (1 << 26, 662267), ((1 << 17) + 5, 6000)):
        assert zhal.image_dirty_words(W, D) == logup.image_dirty_words(W, D), (W, D)
    assert logup.image_dirty_words(64, 64) == 4 + 3 + 33 * 7                  # every node of a full tree of height 3


def test_an_empty_table_has_no_dirty_nodes():
    image = np.arange(1, 65, dtype=np.uint32)
    tree = logup.reference_image_tree(image)
    proof = nc.pcases.host_proof(image, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.uint32), tree)
    with pytest.raises(logup.ReferenceError, match=r"an empty table \(D = 0\) has no dirty nodes.*sealed from the tree"):
        logup.reference_page_out_nodes(proof, tree[1])


def test_the_bindings_have_the_headers_argument_counts():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zkhal.h")).read(), flags=re.S)
    lib = zhal.load_library()
    for name, count in (("zkh_image_dirty_words", 2), ("zkh_image_proof_nodes", 6), ("zkh_page_tree_witgen_nodes", 13)):
        declared = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", src)
        assert declared, f"{name} is not declared in include/zkhal.h"
        assert len(declared.group(1).split(",")) == count, name
        assert len(zhal.ABI[name][1]) == count and len(getattr(lib, name).argtypes) == count, name
    # the nodes call is the walk's operands and `dirty`; the witness call is the two-tree call's with `dirty` for the two trees
    assert zhal.ABI["zkh_image_proof_nodes"][1][:5] == zhal.ABI["zkh_image_proof_walk"][1]
    two = zhal.ABI["zkh_page_tree_witgen"][1]
    assert zhal.ABI["zkh_page_tree_witgen_nodes"][1] == two[:7] + two[8:]
