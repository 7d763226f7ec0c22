"""What the tests of P2-PAGE-ordered share (tests/test_page_ordered.py, tests/test_page_ordered_gpu.py; imported the way
page_circuit_cases is): images, page tables, and the Python reference's trace of each part (p2_page_ordered.reference_ordered_part).
Every table and every part is built once per process and handed out read-only."""
import functools

import numpy as np

import page_circuit_cases as cases
from zeth_amd.circuits import p2_page, p2_page_ordered as G

P = cases.P
ONE = cases.ONE
SHAPES = cases.SHAPES
H12 = (12, 1994, (1 << 14) + 3)                                              # h = 12, N = 5: gaps with bit 13 set
WIDE = (12, 200, 64)                                                         # h = 3, N = 41: two workgroups of the path kernel
# the grid both files walk: (shape, what, first)
GRID = ([(s, what, 0) for s in SHAPES for what in (0, 1, 3, "N")]
        + [(s, "first_last", 0) for s in SHAPES] + [(s, "adjacent", 0) for s in SHAPES]
        + [(H12, what, 0) for what in ("first_last", "adjacent", "N")]
        + [(SHAPES[1], "2N+3", first) for first in (0, 13, 26)])


def grid_id(g):
    (po2, zk, W), what, first = g
    return f"{po2}-{zk}-{W}-{what}-{first}"


def addresses(what, po2, zk, W, seed=0):
    """the table's addresses, increasing: page_circuit_cases' (an int D, "N", a named pattern), `adjacent` (a gap of 0 three times,
    then a long one) or "2N+3" (random addresses, three parts)"""
    if what == "adjacent":
        return np.array([5, 6, 7, W - 1], dtype=np.int64)
    if what == "2N+3":
        D = 2 * cases.slots(po2, zk, W) + 3
        return np.sort(np.random.default_rng(2000 + seed).choice(W, D, replace=False)).astype(np.int64)
    return cases.addresses(what, po2, zk, W, seed)


@functools.lru_cache(maxsize=None)
def table(po2, zk, W, what, seed=0):
    """-> a dict: image (raw words, a third of them >= P), addrs, outs (residues), table [(a, in, out)], image_after, h, N, plan"""
    rng = np.random.default_rng(seed)
    image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    image[rng.random(W) < 0.33] += np.uint32(P)
    addrs = addresses(what, po2, zk, W, seed)
    outs = rng.integers(0, P, len(addrs), dtype=np.uint64).astype(np.uint32)
    after = image.copy()
    after[addrs] = outs
    h = p2_page.tree_height(W)
    t = {"po2": po2, "zk": zk, "W": W, "h": h, "N": p2_page.slots(po2, zk, h), "image": image, "addrs": addrs, "outs": outs, "image_after": after,
         "table": [(int(a), int(image[a]) % P, int(o)) for a, o in zip(addrs, outs)], "plan": p2_page.parts(po2, zk, W, len(addrs))}
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def part(po2, zk, W, what, first=0, seed=0):
    """-> (data, out, code) of the part at `first` of table(...): the reference's data group as (129, n) with the blinding rows zero,
    root_before ‖ root_after ‖ lo ‖ hi, and the reference's code group (42, n)"""
    t = table(po2, zk, W, what, seed)
    active, out = G.reference_ordered_part(po2, zk, W, t["table"], t["image"], first)
    n = 1 << po2
    data = np.zeros((G.WD, n), dtype=np.uint32)
    data[:, :n - zk] = active
    code = code_of(po2, zk, t["h"])
    data.setflags(write=False)
    out.setflags(write=False)
    return data, out, code


@functools.lru_cache(maxsize=None)
def code_of(po2, zk, h):
    code = G.reference_ordered_code(po2, zk, h)
    code.setflags(write=False)
    return code


def bounds(t, first):
    """(lo, hi) of the part at `first` by the plain formula: one more than the address before the part (0 if none); one more than the
    part's last address (lo if it has none)"""
    a = t["addrs"]
    lo = int(a[first - 1]) + 1 if first else 0
    last = min(first + t["N"], len(a))
    return lo, (int(a[last - 1]) + 1 if last > first else lo)
