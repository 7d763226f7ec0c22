"""What the tests of WIDE paging share (tests/test_logup_wide.py, tests/test_logup_wide_gpu.py; imported the way pages_cases is): hand-built
load / store traces over a paged memory of TWO value words per address (ZKA1 version 10) under one paged LINK record with nc = 3, or under
the k = 3 ports of one such memory, and its PAGES record with V = 2; and an independent dictionary walk over the accesses that is not
logup.reference_links: the memory as {address: (raw word 0, raw word 1, raw clock, (row, port))}, the image flat, word j of address a at
2 a + j."""
import numpy as np

from conftest import rand_fp
from zeth_amd.circuits import logup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA

P = 2013265921
ONE = (1 << 32) % P
RINV = pow(ONE, -1, P)
WC = 8                                          # code columns; port q of the ported case selects by code column 3 + q, `sparse` by code column 3
# data columns of a port, from its base PER q: key, clock, the two value words, the write flag, then the LINK's destinations linked, last,
# prev clock, prev value 0, prev value 1 and 3 limbs of 8 bits
KEY, CLOCK, V0, V1, WRITE, LINKED, LAST, PCLOCK, PV0, PV1, LIMB0 = range(11)
PER = 13
# ... and of the page table, from PER k: p_on, p_addr, p_in_0, p_in_1, p_out_0, p_out_1, p_time, 3 address limbs, 3 gap limbs of 8 bits
P_ON, P_ADDR, P_IN0, P_IN1, P_OUT0, P_OUT1, P_TIME, ALIMB0, GAP0 = 0, 1, 2, 3, 4, 5, 6, 7, 10
TABLE_W = 13
KINDS = ["equal", "distinct", "range5", "sparse", "edges", "big", "two"]
SIZES = [(8, 40), (12, 1994), (13, 1994)]       # A = 216: no wave multiple; 2102; 6198: past one sort tile and one scan workgroup


def enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def dec(x):
    return np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(RINV) % np.uint64(P)


def table_base(k=1):
    return PER * k


def image_addresses(kind, A):
    """W, the image's addresses (it has 2 W words): `distinct` spreads A addresses over 3 A + 2"""
    return 3 * A + 2 if kind == "distinct" else 1000


def case(kind, seed, po2, zk, image=None, trace_seed=None, k=1):
    """-> (desc, blob, code, data, image): code / data as (columns, n) arrays with the destinations and the blinding rows poisoned, image the
    2 W raw Montgomery words of the flat image (random non-zero residues whose two halves differ at every address, unless one is given: a
    second segment starts from the first one's).  A load / store trace by one walk over the accesses in (row, port) order: every access
    draws a write flag (the first access to an address is mostly a load, which the image must answer with BOTH words), a load takes what
    the previous access to its address left, or the image's two words; clocks start at 1 or above and rise by a step per address, so every
    difference fits 3 limbs of 8 bits.  Kinds as pages_cases': `equal` one address; `distinct` all distinct; `range5` five; `sparse` a
    selector (code 3) and 40 addresses; `edges` the addresses 0 and W - 1 among four; `big` a third of the key, clock, BOTH value columns
    and the image as raw words >= P; `two` a second LINK record that is not paged.  k = 3: the ported case, three LINK records of one
    memory, every port with a selector of its own (code 3 + q)"""
    assert k == 1 or kind != "distinct", "k A distinct addresses do not fit the A rows of the page table"
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    two = kind == "two"
    pg0 = table_base(k)
    second = pg0 + TABLE_W
    wd = second + (10 if two else 0) + 1
    W = image_addresses(kind, A) if image is None else len(image) // 2
    if image is None:
        image = rng.integers(1, P, 2 * W, dtype=np.uint64).astype(np.uint32)
        same = image[0::2] == image[1::2]
        image[1::2][same] = image[1::2][same] % np.uint32(P - 1) + np.uint32(1)  # the halves differ: v + 1, or 1 after P - 1
    image = np.array(image, dtype=np.uint32)
    if trace_seed is not None:
        rng = np.random.default_rng(trace_seed)
    code, data = rand_fp(rng, WC, n), rand_fp(rng, wd, n)
    b = logup.LogupBuilder((4, WC, wd), (4, 8))
    b.term(0, [(GROUP_DATA, wd - 1)], tag=1)
    if kind == "equal":
        keys = np.full((k, A), 77, dtype=np.int64)
    elif kind == "distinct":
        keys = (rng.permutation(k * A).astype(np.int64) * 3 + 1).reshape(k, A)
    elif kind == "range5":
        keys = rng.choice(W, 5, replace=False)[rng.integers(0, 5, (k, A))].astype(np.int64)
    elif kind == "sparse":
        keys = rng.integers(0, 40, (k, A)).astype(np.int64) * 7
    elif kind == "edges":
        keys = np.array([0, W - 1, 5, W - 2])[rng.integers(0, 4, (k, A))].astype(np.int64)
    else:
        keys = rng.integers(0, 50, (k, A)).astype(np.int64)
    sels = [3 + q for q in range(k)] if k > 1 else [3 if kind == "sparse" else None]
    on = np.stack([rng.random(A) < (0.6 if k > 1 else 0.3) if s is not None else np.ones(A, dtype=bool) for s in sels])
    for q, s in enumerate(sels):
        if s is not None:
            code[s, :A] = enc(on[q].astype(np.uint64))
    step = int(rng.integers(1, 40))
    store = rng.random((k, A)) < 0.5
    clock = rng.integers(0, P, (k, A)).astype(np.int64)                      # the cells of rows that are no access stay random
    seen, held = {}, {}
    for r in range(A):
        for q in range(k):
            if not on[q, r]:
                continue
            a = int(keys[q, r])
            if a not in seen and (kind in ("equal", "range5", "edges") or rng.random() < 0.8):     # a first access: mostly a load, answered by the image
                store[q, r] = False
            clock[q, r] = seen[a] + step if a in seen else int(rng.integers(1, 1000))
            seen[a] = int(clock[q, r])
            if not store[q, r]:
                data[PER * q + V0, r], data[PER * q + V1, r] = held.get(a, (int(image[2 * a]), int(image[2 * a + 1])))
            held[a] = (int(data[PER * q + V0, r]), int(data[PER * q + V1, r]))
    head = None
    for q in range(k):
        base = PER * q
        data[base + KEY, :A], data[base + CLOCK, :A], data[base + WRITE, :A] = enc(keys[q]), enc(clock[q]), enc(store[q].astype(np.uint64))
        if kind == "big":                                                    # about a third of the cells as raw words >= P
            for c in (KEY, CLOCK, V0, V1, WRITE):
                col = data[base + c]
                col[:A][(rng.random(A) < 0.3) & (col[:A] < P)] += np.uint32(P)
        link = b.derive_links(sels[q], (GROUP_DATA, base + KEY), [(GROUP_DATA, base + CLOCK), (GROUP_DATA, base + V0), (GROUP_DATA, base + V1)],
                              list(range(base + LINKED, base + LINKED + 8)), 8, write=(GROUP_DATA, base + WRITE), joins=head)
        head = head or link
    if kind == "big":
        image[(rng.random(2 * W) < 0.3) & (image < P)] += np.uint32(P)
    if two:                                                                  # keys from nine values, clocks that count, random values: no read rule
        k2 = rng.integers(0, 9, A).astype(np.int64)
        data[second, :A], data[second + 1, :A] = enc(k2 + 1000), enc(np.arange(A) * 3)
        b.derive_links(None, (GROUP_DATA, second), [(GROUP_DATA, second + 1), (GROUP_DATA, second + 2)], list(range(second + 3, second + 10)), 8)
    b.derive_pages(head, list(range(pg0, pg0 + TABLE_W)), 8)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code, data, image


def accesses(code, data, A, kind, k=1):
    """the paged memory's accesses, in (row, port) order"""
    if k == 1:
        rows = np.nonzero(code[3, :A] == ONE)[0] if kind == "sparse" else np.arange(A)
        return [(int(r), 0) for r in rows]
    return [(r, q) for r in range(A) for q in range(k) if code[3 + q, r] == ONE]


def walk(code, data, image, A, kind, memory=None, k=1):
    """the paged memory's destinations the slow way, independent of logup.reference_links: one access after another, in (row, port) order,
    with the memory in a dictionary {address: (raw word 0, raw word 1, raw clock word, (row, port))}, every load compared, in both halves,
    with what the memory holds, else with the image's words 2 a and 2 a + 1 -> ({column: A words}, memory, the FLAT page table as rows
    (2 a + j, in_j, out_j), raw words).  memory: what an earlier segment left: {address: (raw word 0, raw word 1)}, in the image's place"""
    x = lambda v: int(v) % P * RINV % P
    pg0 = table_base(k)
    out = {PER * q + c: np.zeros(A, dtype=np.uint32) for q in range(k) for c in range(LINKED, LINKED + 8)}
    out.update({c: np.zeros(A, dtype=np.uint32) for c in range(pg0, pg0 + TABLE_W)})
    mem, first = {}, {}
    start = lambda a: (image[2 * a], image[2 * a + 1]) if memory is None or a not in memory else memory[a]
    for r, q in accesses(code, data, A, kind, k):
        base = PER * q
        a = x(data[base + KEY, r])
        assert 2 * a + 1 < len(image)
        w = x(data[base + WRITE, r])
        assert w in (0, 1)
        p0, p1, pclock, at = mem.get(a, start(a) + (0, None))
        if not w:
            assert (x(data[base + V0, r]), x(data[base + V1, r])) == (x(p0), x(p1)), (r, q, a)
        d = x(data[base + CLOCK, r]) - x(pclock) - 1
        assert 0 <= d < 1 << 24 and (at is not None or x(data[base + CLOCK, r]) > 0), (r, q, d)
        out[base + LAST][r] = ONE
        if at is not None:
            out[base + LINKED][r], out[PER * at[1] + LAST][at[0]], out[base + PCLOCK][r] = ONE, 0, pclock
        else:
            first[a] = (r, q)
        out[base + PV0][r], out[base + PV1][r] = p0, p1
        for j in range(3):
            out[base + LIMB0 + j][r] = (d >> (8 * j)) % 256 * ONE % P
        mem[a] = (data[base + V0, r], data[base + V1, r], data[base + CLOCK, r], (r, q))
    below, flat = None, []
    for i, a in enumerate(sorted(mem)):
        gap = 0 if below is None else a - below - 1
        ins = start(a)
        out[pg0 + P_ON][i], out[pg0 + P_ADDR][i] = ONE, data[PER * first[a][1] + KEY, first[a][0]]
        out[pg0 + P_IN0][i], out[pg0 + P_IN1][i] = ins
        out[pg0 + P_OUT0][i], out[pg0 + P_OUT1][i], out[pg0 + P_TIME][i] = mem[a][:3]
        for j in range(3):
            out[pg0 + ALIMB0 + j][i] = (a >> (8 * j)) % 256 * ONE % P
            out[pg0 + GAP0 + j][i] = (gap >> (8 * j)) % 256 * ONE % P
        flat += [(2 * a, ins[0], mem[a][0]), (2 * a + 1, ins[1], mem[a][1])]
        below = a
    return out, {a: v[:2] for a, v in mem.items()}, np.array(flat, dtype=np.uint32).reshape(-1, 3)


def check_conditions(kind, code, data, image, A, k=1):
    """what the issue asks of every case, asserted against the walk alone: the two halves of every image address differ (as residues), at
    least a quarter of the first accesses are loads answered by an image address whose two words are both non-zero, and in `big` at least
    a sixth of the image's words are >= P (and both value columns hold some)"""
    assert (image[0::2] % P != image[1::2] % P).all(), "the two halves of an image address are equal"
    seen, firsts, answered = set(), 0, 0
    for r, q in accesses(code, data, A, kind, k):
        a = int(dec(data[PER * q + KEY, r]))
        if a in seen:
            continue
        seen.add(a)
        firsts += 1
        answered += int(data[PER * q + WRITE, r] % P == 0 and image[2 * a] % P != 0 and image[2 * a + 1] % P != 0)
    assert firsts and 4 * answered >= firsts, (kind, firsts, answered)
    if kind == "big":
        assert 6 * int((image >= P).sum()) >= image.size
        assert all((data[PER * q + c, :A] >= P).any() for q in range(k) for c in (KEY, CLOCK, V0, V1))
    return firsts
