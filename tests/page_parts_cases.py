"""What the tests of P2-PAGE's parts share (tests/test_page_parts.py, tests/test_page_parts_gpu.py; imported the way page_circuit_cases
is): page tables of D > N rows, their plan, and the Python reference's trace of each part (p2_page.reference_page_part: the updates
before the part applied to the image in numpy, then reference_page_trace).  Every table and every part is built once per process and
handed out read-only."""
import functools

import numpy as np

import page_circuit_cases as cases
from zeth_amd.circuits import p2_page as G

P = cases.P
H5 = (12, 1994, 8 * 17 + 3)                                                  # h = 5, N = 13, a partial last leaf


@functools.lru_cache(maxsize=None)
def table(po2, zk, W, what, seed=0):
    """-> a dict: image (raw words, a third of them >= P), addrs, outs (residues), table [(a, in, out)], image_after, h, N and plan =
    p2_page.parts.  what: "all" (every word of the image, in order) or an int D (D random addresses)"""
    rng = np.random.default_rng(seed)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    image[rng.random(W) < 0.33] += np.uint32(P)
    addrs = np.arange(W, dtype=np.int64) if what == "all" else np.sort(np.random.default_rng(2000 + seed).choice(W, what, replace=False)).astype(np.int64)
    outs = rng.integers(0, P, len(addrs), dtype=np.uint64).astype(np.uint32)
    after = image.copy()
    after[addrs] = outs
    h = G.tree_height(W)
    t = {"po2": po2, "zk": zk, "W": W, "h": h, "N": G.slots(po2, zk, h), "image": image, "addrs": addrs, "outs": outs, "image_after": after,
         "table": [(int(a), int(image[a]) % P, int(o)) for a, o in zip(addrs, outs)], "plan": G.parts(po2, zk, W, len(addrs))}
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def image_at(t, rows):
    """the image of table `t` with its updates [0, rows) applied"""
    image = t["image"].copy()
    image[t["addrs"][:rows]] = t["outs"][:rows]
    return image


@functools.lru_cache(maxsize=None)
def part(po2, zk, W, what, first, seed=0):
    """-> (data, out) of the part at `first` of table(...): the reference's data group as (125, n) with the blinding rows zero, and
    root_before ‖ root_after of the part"""
    t = table(po2, zk, W, what, seed)
    active, root_before, root_after = G.reference_page_part(po2, zk, W, t["table"], t["image"], first)
    n = 1 << po2
    data = np.zeros((G.WD, n), dtype=np.uint32)
    data[:, :n - zk] = active
    out = np.concatenate([root_before, root_after]).astype(np.uint32)
    data.setflags(write=False)
    out.setflags(write=False)
    return data, out
