"""What the tests of P2-TREE share (tests/test_page_tree.py, tests/test_page_tree_gpu.py; imported the way page_ordered_cases is): images,
page tables, the plan and the Python reference's trace of each part (p2_tree.reference_tree_part).  Every table and every part is built
once per process and handed out read-only."""
import functools

import numpy as np

from zeth_amd.circuits import p2_page, p2_tree as G

P = 2013265921
ONE = (1 << 32) % P
NOISE = 0x0C0A
# (po2, zk_cycles, W): B block slots, tree height h
H3 = (10, 500, 64)                        # B 16, h 3: a full image is 7 blocks
H5 = (12, 1994, 8 * 17 + 3)               # B 67, h 5: W is not a power of two, the last leaf is partial
H6 = (10, 500, 512)                       # B 16, h 6: a full image is 63 nodes, several parts whose edges meet at different layers
H12 = (12, 1994, (1 << 14) + 3)           # B 67, h 12: 40 random addresses take several parts
H8 = (12, 200, 2048)                      # B 125, h 8: two workgroups of the block kernel (250 lanes of 64)
SHAPES = [H3, H5, H6, H12, H8]
SETS = (0, 1, 3, "first_last", "adjacent", "one_pair", "random", "all")
# every shape with every address set; `all` (every word of the image) is left out at h = 12 only, where it is 1025 pairs in some 30 parts
# that take no path the 40 random addresses do not
CASES = [(s, what) for s in SHAPES for what in SETS if not (s == H12 and what == "all")]


def addresses(what, W, seed=0):
    """the table's addresses, increasing: an int D (D random addresses) or a named pattern"""
    rng = np.random.default_rng(3000 + seed)
    if isinstance(what, int):
        return np.sort(rng.choice(W, what, replace=False)).astype(np.int64)
    if what == "random":
        return np.sort(rng.choice(W, 40, replace=False)).astype(np.int64)
    return np.array({"first_last": [0, W - 1],
                     "adjacent": [5, 6, 7, W - 1],                  # three words of one leaf, then a long gap
                     "one_pair": [3, 12, W - 1],                    # two words of one pair of leaves, in different leaves
                     "all": list(range(W))}[what], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def table(po2, zk, W, what, seed=0):
    """-> a dict: image (raw words, a third of them >= P), addrs, outs (residues), table [(a, in, out)], image_after, h, B, plan"""
    rng = np.random.default_rng(seed)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    image[rng.random(W) < 0.33] += np.uint32(P)
    addrs = addresses(what, W, seed)
    outs = rng.integers(0, P, len(addrs), dtype=np.uint64).astype(np.uint32)
    after = image.copy()
    after[addrs] = outs
    t = {"po2": po2, "zk": zk, "W": W, "h": p2_page.tree_height(W), "B": G.block_slots(po2, zk), "image": image, "addrs": addrs, "outs": outs,
         "image_after": after, "table": [(int(a), int(image[a]) % P, int(o)) for a, o in zip(addrs, outs)], "plan": G.parts(po2, zk, W, addrs)}
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def part(po2, zk, W, what, p=0, seed=0):
    """-> (data, out, code) of part p of table(...)'s plan: the reference's data group as (106, n) with the blinding rows zero,
    root_before ‖ root_after ‖ lo ‖ hi, and the reference's code group (41, n)"""
    t = table(po2, zk, W, what, seed)
    first, count = t["plan"][p]
    active, out = G.reference_tree_part(po2, zk, W, t["table"], t["image"], first, count)
    n = 1 << po2
    data = np.zeros((G.WD, n), dtype=np.uint32)
    data[:, :n - zk] = active
    data.setflags(write=False)
    out.setflags(write=False)
    return data, out, code_of(po2, zk)


@functools.lru_cache(maxsize=None)
def code_of(po2, zk):
    code = G.reference_tree_code(po2, zk)
    code.setflags(write=False)
    return code


@functools.lru_cache(maxsize=None)
def args():
    from zeth_amd.circuits import logup
    return logup.Arguments.parse(G.arguments())


def grid():
    """(shape, what, p) over CASES and every part of each plan"""
    return [(s, what, p) for s, what in CASES for p in range(len(table(*s, what)["plan"]))]


def grid_id(g):
    (po2, zk, W), what, p = g
    return f"{po2}-{zk}-{W}-{what}-part{p}"


def node_count(h, addrs):
    """the dirty nodes of a part with the addresses `addrs`, counted from the set of ids: every pair of leaves and all its ancestors"""
    ids = set()
    for a in addrs:
        i = (1 << (h - 1)) + (int(a) >> 4)
        while i:
            ids.add(i)
            i >>= 1
    return max(len(ids), 1)
