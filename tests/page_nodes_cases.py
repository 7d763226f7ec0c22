"""What the tests of the dirty-node table share (tests/test_page_nodes.py, tests/test_page_nodes_gpu.py; imported the way
page_tree_cases is): the tables of page_tree_cases that have a row, the table of 600 rows, each with its ZKU1 proof, its two dense trees
and the numpy twin of its dirty-node table (logup.reference_page_out_nodes).  Everything is built once per process and handed out
read-only."""
import functools

import numpy as np

import page_circuit_cases as pcases
import page_tree_cases as tc
from zeth_amd.circuits import logup, p2_tree as G

P = tc.P
# 600 rows, one per leaf, over W = 8192 (h = 10): 300 pairs of leaves, 522 dirty nodes, two parts, (0, 516) and (516, 84), at B = 522 block
# slots; more than 256 items on the two lowest layers, part 1's edge chain starts in the middle of every list, 17 workgroups of blocks
ROWS600 = (14, 200, 8192)
SETS = (1, 3, "first_last", "adjacent", "one_pair", "random", "all")
# (shape, what): the witness cases of the issue; "rows600" is the table above
WITNESS = [(s, what) for s in (tc.H3, tc.H5, tc.H6, tc.H8) for what in SETS] + [(tc.H12, "random"), (ROWS600, "rows600")]
# ... and every table of page_tree_cases.CASES with a row, for the table itself
TABLES = [(s, what) for s, what in tc.CASES if what != 0] + [(ROWS600, "rows600")]


@functools.lru_cache(maxsize=None)
def table(po2, zk, W, what):
    """page_tree_cases.table, and the same dict for "rows600" """
    if what != "rows600":
        return tc.table(po2, zk, W, what)
    rng = np.random.default_rng(600)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    image[rng.random(W) < 0.33] += np.uint32(P)
    addrs = 8 * np.arange(600, dtype=np.int64) + 3
    outs = rng.integers(0, P, len(addrs), dtype=np.uint64).astype(np.uint32)
    after = image.copy()
    after[addrs] = outs
    t = {"po2": po2, "zk": zk, "W": W, "h": 10, "B": G.block_slots(po2, zk), "image": image, "addrs": addrs, "outs": outs, "image_after": after,
         "table": [(int(a), int(image[a]) % P, int(o)) for a, o in zip(addrs, outs)], "plan": G.parts(po2, zk, W, addrs)}
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def proved(po2, zk, W, what):
    """-> a dict: proof (the ZKU1 words), before, after (the dense trees as (2 L, 8) digests), root_before, root_after, nodes (the twin)"""
    t = table(po2, zk, W, what)
    before, after = logup.reference_image_tree(t["image"]), logup.reference_image_tree(t["image_after"])
    proof = pcases.host_proof(t["image"], t["addrs"], t["outs"], before)
    root_after, nodes = logup.reference_page_out_nodes(proof, before.reshape(-1, 8)[1])
    p = {"proof": proof, "before": before.reshape(-1, 8), "after": after.reshape(-1, 8), "root_before": before.reshape(-1, 8)[1].copy(), "root_after": root_after,
         "nodes": nodes}
    for v in p.values():
        v.setflags(write=False)
    return p


def sections(nodes):
    """a dirty-node table's words -> (W, D, h, [(ids, records (n_k, 32)) for k = 1 .. h], the words it takes)"""
    nodes = np.asarray(nodes, dtype=np.uint32)
    assert int(nodes[0]) == logup.NODES_MAGIC
    W, D, h = (int(x) for x in nodes[1:4])
    at, out = logup.NODES_HEADER + h, []
    for k in range(1, h + 1):
        n = int(nodes[logup.NODES_HEADER + k - 1])
        out.append((nodes[at:at + n], nodes[at + n:at + 33 * n].reshape(n, 32)))
        at += 33 * n
    return W, D, h, out, at


def grid():
    """(shape, what, p) over WITNESS and every part of each plan"""
    return [(s, what, p) for s, what in WITNESS for p in range(len(table(*s, what)["plan"]))]


grid_id = tc.grid_id
