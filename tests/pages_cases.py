"""What the paging tests share (tests/test_logup_pages.py, tests/test_logup_pages_gpu.py; imported the way args_gpu is): hand-built load /
store traces over a memory image under one paged LINK record and its PAGES record (ZKA1 version 7), as test_logup_reads_gpu.py's `_case`
builds them for the read rule.  And the SEAM TABLES (seam_table) of the page-out's proof, walk and tree update (tests/test_image_proof.py,
test_image_proof_gpu.py, test_image_walk_gpu.py, test_image_tree_gpu.py): hand-made page tables that put a head decision of the
compactions on the seam between two workgroups of 256 lanes."""
import numpy as np

from conftest import rand_fp
from zeth_amd.circuits import logup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA

P = 2013265921
ONE = (1 << 32) % P
RINV = pow(ONE, -1, P)
WC = 8                                          # code columns
# data columns of the paged record: key, clock, value, linked, last, prev clock, prev value, 3 limbs of 8 bits, the write flag, then the
# page table: p_on, p_addr, p_in, p_out, p_time, 3 address limbs, 3 gap limbs of 8 bits
KEY, CLOCK, VALUE, LINKED, LAST, PCLOCK, PVALUE, LIMB0, WRITE, P_ON, P_ADDR, P_IN, P_OUT, P_TIME, ALIMB0, GAP0 = 0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16, 19
PAGED_W = 22
SECOND = 22                                     # `two`: a second LINK record, not paged, no READS: key, clock, value, 7 destinations
KINDS = ["equal", "distinct", "range5", "sparse", "edges", "big", "two"]


def enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def dec(x):
    return np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(RINV) % np.uint64(P)


def image_words(kind, A):
    """the image's size: `distinct` spreads A addresses over 3 A + 2 words"""
    return 3 * A + 2 if kind == "distinct" else 1000


def case(kind, seed, po2, zk, image=None, trace_seed=None):
    """-> (desc, blob, code, data, image): code / data as (columns, n) arrays with the destinations and the blinding rows poisoned, image
    the W raw Montgomery words (random non-zero residues, unless one is given: a second segment starts from the first one's).  A load /
    store trace: every access draws a write flag (the first access to an address is mostly a load, which the image must answer), a load
    takes what the previous access to its address left, or the image's word; clocks start at 1 or above and rise by a step per address,
    so every difference fits 3 limbs of 8 bits.  Kinds: `equal` one address for every access; `distinct` all addresses distinct;
    `range5` five addresses; `sparse` a selector (code 3) and 40 addresses; `edges` the addresses 0 and W - 1 among four; `big` a third
    of the key, clock, value and image words as raw words >= P next to their residues; `two` a second LINK record that is not paged"""
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    two = kind == "two"
    wd = PAGED_W + (10 if two else 0) + 1
    W = image_words(kind, A) if image is None else len(image)
    if image is None:
        image = rng.integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    image = np.array(image, dtype=np.uint32)
    if trace_seed is not None:
        rng = np.random.default_rng(trace_seed)
    code, data = rand_fp(rng, WC, n), rand_fp(rng, wd, n)
    b = logup.LogupBuilder((4, WC, wd), (4, 8))
    b.term(0, [(GROUP_DATA, wd - 1)], tag=1)
    sel = 3 if kind == "sparse" else None
    if kind == "equal":
        keys = np.full(A, 77, dtype=np.int64)
    elif kind == "distinct":
        keys = rng.permutation(A).astype(np.int64) * 3 + 1
    elif kind == "range5":
        keys = rng.choice(W, 5, replace=False)[rng.integers(0, 5, A)].astype(np.int64)
    elif kind == "sparse":
        keys = rng.integers(0, 40, A).astype(np.int64) * 7
    elif kind == "edges":
        keys = np.array([0, W - 1, 5, W - 2])[rng.integers(0, 4, A)].astype(np.int64)
    else:
        keys = rng.integers(0, 50, A).astype(np.int64)
    on = rng.random(A) < 0.3 if sel is not None else np.ones(A, dtype=bool)
    if sel is not None:
        code[sel, :A] = enc(on.astype(np.uint64))
    step = int(rng.integers(1, 40))
    store = rng.random(A) < 0.5
    seen, held, clock = {}, {}, np.zeros(A, dtype=np.int64)
    for r in np.nonzero(on)[0]:
        k = int(keys[r])
        if k not in seen and (kind in ("equal", "range5", "edges") or rng.random() < 0.8):       # a first access: mostly a load (always, of few addresses), answered by the image
            store[r] = False
        clock[r] = seen[k] + step if k in seen else int(rng.integers(1, 1000))
        seen[k] = int(clock[r])
        if not store[r]:
            data[VALUE, r] = held.get(k, int(image[k]))
        held[k] = int(data[VALUE, r])
    clock[~on] = rng.integers(0, P, int((~on).sum()))
    data[KEY, :A], data[CLOCK, :A], data[WRITE, :A] = enc(keys), enc(clock), enc(store.astype(np.uint64))
    if kind == "big":                                                        # about a third of the cells as raw words >= P
        for col in (data[KEY], data[CLOCK], data[VALUE], data[WRITE]):
            col[:A][(rng.random(A) < 0.3) & (col[:A] < P)] += np.uint32(P)
        image[(rng.random(W) < 0.3) & (image < P)] += np.uint32(P)
    link = b.derive_links(sel, (GROUP_DATA, KEY), [(GROUP_DATA, CLOCK), (GROUP_DATA, VALUE)], list(range(LINKED, LINKED + 7)), 8, write=(GROUP_DATA, WRITE))
    if two:                                                                  # keys from nine values, clocks that count, random values: no read rule
        k2 = rng.integers(0, 9, A).astype(np.int64)
        data[SECOND, :A], data[SECOND + 1, :A] = enc(k2 + 1000), enc(np.arange(A) * 3)
        b.derive_links(None, (GROUP_DATA, SECOND), [(GROUP_DATA, SECOND + 1), (GROUP_DATA, SECOND + 2)], list(range(SECOND + 3, SECOND + 10)), 8)
    b.derive_pages(link, list(range(P_ON, P_ON + 11)), 8)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code, data, image


def accesses(code, data, A, kind):
    """the paged record's access rows"""
    return np.nonzero(code[3, :A] == ONE)[0] if kind == "sparse" else np.arange(A)


def walk(code, data, image, A, kind, memory=None):
    """the paged record's destinations the slow way, independent of logup.reference_links: one access after another with the memory in a
    dictionary {address: (raw value word, raw clock word, row)}, every load compared with what the memory holds, else with the image
    -> ({column: A words}, memory).  memory: what an earlier segment left: {address: raw value word}, used in place of the image"""
    x = lambda v: int(v) % P * RINV % P
    out = {c: np.zeros(A, dtype=np.uint32) for c in range(LINKED, LINKED + 7)}
    out.update({c: np.zeros(A, dtype=np.uint32) for c in range(P_ON, P_ON + 11)})
    mem, first = {}, {}
    for r in accesses(code, data, A, kind):
        a = x(data[KEY, r])
        assert a < len(image)
        w = x(data[WRITE, r])
        assert w in (0, 1)
        start = image[a] if memory is None or a not in memory else memory[a]
        pval, pclock, prow = mem.get(a, (start, 0, -1))
        if not w:
            assert x(data[VALUE, r]) == x(pval), (r, a)
        d = x(data[CLOCK, r]) - x(pclock) - 1
        assert 0 <= d < 1 << 24 and (prow >= 0 or x(data[CLOCK, r]) > 0), (r, d)
        out[LAST][r] = ONE
        if prow >= 0:
            out[LINKED][r], out[LAST][prow], out[PCLOCK][r] = ONE, 0, pclock
        else:
            first[a] = r
        out[PVALUE][r] = pval
        for j in range(3):
            out[LIMB0 + j][r] = (d >> (8 * j)) % 256 * ONE % P
        mem[a] = (data[VALUE, r], data[CLOCK, r], r)
    below = None
    for i, a in enumerate(sorted(mem)):
        gap = 0 if below is None else a - below - 1
        out[P_ON][i], out[P_ADDR][i], out[P_OUT][i], out[P_TIME][i] = ONE, data[KEY, first[a]], mem[a][0], mem[a][1]
        out[P_IN][i] = image[a] if memory is None or a not in memory else memory[a]
        for j in range(3):
            out[ALIMB0 + j][i] = (a >> (8 * j)) % 256 * ONE % P
            out[GAP0 + j][i] = (gap >> (8 * j)) % 256 * ONE % P
        below = a
    return out, {a: v[0] for a, v in mem.items()}


SEAM_TABLES = ["seam_leaf", "seam_pair", "seam_new"]
SEAM_ROWS = [256, 257, 513]                     # the table ends on the seam; one row past it; a second seam under random rows


def seam_table(what, D, W, rng):
    """-> D sorted, distinct addresses below W (an image of at least 512 leaves), random except around rows 255 and 256: the last lane of
    workgroup 0 and lane 0 of workgroup 1 of every kernel that takes a row per lane, 256 lanes a workgroup.  `seam_leaf`: the two rows
    are words 3 and 4 of one leaf (lane 0 of workgroup 1 is no head of the leaf list); `seam_pair`: they lie in the leaves 2 q and
    2 q + 1 (a head of the leaf list, no head of the parents'); `seam_new`: in the leaves 2 q + 1 and 2 q + 2, under different parents
    (a head of both).  Rows [0, 255) lie in distinct leaves, so row 256's leaf is item 255 or 256 of the leaf list as well."""
    assert what in SEAM_TABLES and D >= 256
    above = max(D - 257, 0)                                                  # the random rows past row 256
    j = int(rng.integers(256, (W + 7) // 8 - 3 - (above + 7) // 8))          # row 255's leaf: 255 leaves below it, room above row 256's
    if what == "seam_leaf":
        lo, hi = 8 * j + 3, 8 * j + 4
    else:
        j = j & ~1 if what == "seam_pair" else j | 1
        lo, hi = 8 * j + int(rng.integers(0, 8)), 8 * (j + 1) + int(rng.integers(0, 8))
    below = 8 * np.sort(rng.choice(j, 255, replace=False)).astype(np.int64) + rng.integers(0, 8, 255)
    after = hi + 1 + np.sort(rng.choice(W - hi - 1, above, replace=False)).astype(np.int64)
    addrs = np.concatenate([below, [lo, hi], after]).astype(np.int64)[:D]
    assert len(addrs) == D and (np.diff(addrs) > 0).all() and addrs[-1] < W and addrs[255] == lo and len(np.unique(addrs[:256] >> 3)) == 256
    if D > 256:
        same_leaf, same_parent = (lo >> 3) == (hi >> 3), (lo >> 4) == (hi >> 4)
        assert addrs[256] == hi and (same_leaf, same_parent) == {"seam_leaf": (True, True), "seam_pair": (False, True), "seam_new": (False, False)}[what]
    return addrs
