"""What the P2-PAGE tests share (tests/test_page_circuit.py, tests/test_page_circuit_gpu.py; imported the way pages_cases is): images,
hand-made page tables, the Python reference's trace of each, and the ZKU1 proof of the same table.  Every case is built once per
process and handed out read-only."""
import functools

import numpy as np

import pages_cases as pc
from zeth_amd.circuits import logup, p2_page as G

P = 2013265921
ONE = (1 << 32) % P
# (po2, zk_cycles, W): h = 1 (the leaf block is the top; N = 16 = W, so D = N pages every word), h = 5 with a last partial leaf
# (8 * 17 + 3 words: 18 leaves of 32), h = 3 with every leaf full
SHAPES = [(10, 500, 16), (12, 1994, 8 * 17 + 3), (12, 1994, 64)]
NOISE = 0x0C09


def slots(po2, zk, W):
    return G.slots(po2, zk, G.tree_height(W))


@functools.lru_cache(maxsize=None)
def pages_args():
    """the arguments of a paging circuit: what logup.reference_page_out_proof reads a hand-made page table through"""
    return logup.Arguments.parse(pc.case("range5", 3, 8, 40)[1])


def addresses(what, po2, zk, W, seed=0):
    """the table's addresses, increasing: an int D (D random addresses), or a named pattern"""
    N = slots(po2, zk, W)
    rng = np.random.default_rng(1000 + seed)
    if what == "N":
        what = N
    if isinstance(what, int):
        return np.sort(rng.choice(W, what, replace=False)).astype(np.int64)
    return np.array({"one_leaf": [8, 13],                      # two addresses in one leaf
                     "one_pair": [3, 12, W - 1],               # two in one pair of leaves (16 words); the last word of the image
                     "last": [W - 1],                          # a word of the last (for W = 8 * 17 + 3: partial) leaf, alone
                     "first_last": [0, W - 1]}[what], dtype=np.int64)


def host_proof(image, addrs, outs, nodes):
    """the ZKU1 proof of the table (addrs, image[addrs], outs) over the tree `nodes` of `image`, built on the host"""
    D = len(addrs)
    po2 = max(int(D - 1).bit_length(), 3) if D > 1 else 3
    data = np.zeros((pc.PAGED_W + 1, 1 << po2), dtype=np.uint32)
    data[pc.P_ON, :D], data[pc.P_ADDR, :D], data[pc.P_IN, :D], data[pc.P_OUT, :D] = ONE, pc.enc(addrs), image[addrs], outs
    return logup.reference_page_out_proof(pages_args(), po2, 0, data.reshape(-1), len(image), nodes)


@functools.lru_cache(maxsize=None)
def case(po2, zk, W, what, seed=0):
    """-> a dict: image (raw words, a third of them >= P), addrs, outs (residues), table [(a, in, out)], image_after, code and data
    ((columns, n): the reference's, the blinding rows zero), out = root_before ‖ root_after, N, h"""
    rng = np.random.default_rng(seed)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    image[rng.random(W) < 0.33] += np.uint32(P)
    addrs = addresses(what, po2, zk, W, seed)
    outs = rng.integers(0, P, len(addrs), dtype=np.uint64).astype(np.uint32)
    table = [(int(a), int(image[a]) % P, int(o)) for a, o in zip(addrs, outs)]
    active, root_before, root_after = G.reference_page_trace(po2, zk, W, table, image)
    n = 1 << po2
    data = np.zeros((G.WD, n), dtype=np.uint32)
    data[:, :n - zk] = active
    after = image.copy()
    after[addrs] = outs
    h = G.tree_height(W)
    c = {"po2": po2, "zk": zk, "W": W, "h": h, "N": G.slots(po2, zk, h), "image": image, "addrs": addrs, "outs": outs, "table": table, "image_after": after,
         "code": G.reference_page_code(po2, zk, h), "data": data, "out": np.concatenate([root_before, root_after]).astype(np.uint32)}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c
