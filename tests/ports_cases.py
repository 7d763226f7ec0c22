"""What the tests of PORTS share (tests/test_logup_ports.py, tests/test_logup_ports_gpu.py; imported the way pages_cases is): LINK records
that join a head's memory (ZKA1 version 9).  Small circuits built directly with LogupBuilder, so that every port has a selector of its own,
with a valid load / store trace made by one walk over the accesses in (row, port) order; SYN-LOOKUP-reads-ported at MULTI with its host-made
witness; the paged ported witness over an image of 64 words; and the forgeries of those witnesses that the links stage must refuse."""
import functools

import numpy as np

from conftest import rand_fp
from zeth_amd.circuits import logup, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA

P = logup.P
ONE = (1 << 32) % P
RINV = pow(ONE, -1, P)
MULTI = sl.MULTI
W = 64                                          # the paged cases' image
WC0 = 8                                         # code columns before the selectors: port j of a case selects by code column WC0 + j
PER = 11                                        # data columns of a port: key, clock, value, write flag, then linked, last, 2 prevs, 3 limbs of 8 bits
KEY, CLOCK, VALUE, WRITE, DST0, N_DST = 0, 1, 2, 3, 4, 7


def enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def dec(x):
    return np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(RINV) % np.uint64(P)


# kind -> (po2, zk, the ports of every memory): the GPU cases of the issue, one each
DIRECT = {
    "k2": (8, 40, [2]),                         # 432 items: the run crosses wave and 256-lane boundaries
    "k3": (12, 1994, [3]),                      # 6306 items: more than one 4096-item sort tile
    "k8": (8, 40, [8]),
    "idle_port": (8, 40, [3]),                  # port 1 is never selected
    "idle_head": (8, 40, [2]),                  # the head is never selected, its joiner is
    "one": (8, 40, [3]),                        # one access in the whole memory
    "equal": (8, 40, [2]),                      # all addresses equal: no live key bit, zero radix passes
    "disjoint": (8, 40, [2]),                   # port 0 below 16, port 1 at 2^16 and above: the live bits are the memory's, not a port's
    "big": (9, 100, [3]),                       # raw words >= P in keys, clocks and values
    "mixed": (9, 100, [2, 2, 1]),               # two memories of 2 ports and a single-record one, after two LIMBS records
}


@functools.lru_cache(maxsize=None)
def direct(kind):
    """-> (desc, blob, code, data, po2, zk): random traces (destinations and blinding rows poisoned) under the memories of DIRECT[kind], every
    record with READS, a clock, one value and 3 limbs of 8 bits.  One walk over the accesses in (row, port) order makes the witness valid: the
    clock of an access is its address's last clock plus a step, a load takes what the previous access of any port left there, or 0."""
    po2, zk, memories = DIRECT[kind]
    rng = np.random.default_rng(sum(map(ord, kind)))
    n, A = 1 << po2, (1 << po2) - zk
    n_rec = sum(memories)
    wc, wd = WC0 + n_rec, PER * n_rec + 4
    code, data = rand_fp(rng, wc, n), rand_fp(rng, wd, n)
    b = logup.LogupBuilder((4, wc, wd), (4, 8))
    b.term(0, [(GROUP_DATA, wd - 1)], tag=1)
    if kind == "mixed":                                                      # LIMBS records come before every LINK: the joiners' head indices count them
        b.derive_limbs((GROUP_CODE, 2), [wd - 4, wd - 3], 16)
    rec = 0
    for k in memories:
        every = kind in ("k2", "k3", "equal")                                # no selector: every active row is an access of every port
        on = np.ones((k, A), dtype=bool) if every else rng.random((k, A)) < (0.3 if kind == "k8" else 0.6)
        if kind == "idle_port":
            on[1] = False
        if kind == "idle_head":
            on[0] = False
        if kind == "one":
            on[:] = False
            on[2, A // 2] = True
        keys = rng.integers(0, 1 << 12 if kind == "k3" else 12, (k, A)).astype(np.int64)
        if kind == "equal":
            keys[:] = 77777
        if kind == "disjoint":
            keys[0], keys[1] = rng.integers(0, 16, A), (1 << 16) + 16 * rng.integers(0, 8, A)
            keys[1, ::5] = keys[0, ::5]                                      # and some addresses that both ports touch, in the same row
        step = int(rng.integers(1, 40))
        clock, value = rng.integers(0, P, (k, A)).astype(np.int64), rng.integers(0, P, (k, A)).astype(np.int64)
        store = rng.random((k, A)) < 0.5
        seen, held = {}, {}
        for r in range(A):
            for q in range(k):
                if not on[q, r]:
                    continue
                a = int(keys[q, r])
                clock[q, r] = seen[a] + step if a in seen else int(rng.integers(0, 1000))
                seen[a] = int(clock[q, r])
                if not store[q, r]:
                    value[q, r] = held.get(a, 0)
                held[a] = int(value[q, r])
        head = None
        for q in range(k):
            base = PER * rec
            sel = None if every else WC0 + rec
            if sel is not None:
                code[sel, :A] = enc(on[q].astype(np.uint64))
            data[base + KEY, :A], data[base + CLOCK, :A], data[base + VALUE, :A] = enc(keys[q]), enc(clock[q]), enc(value[q])
            data[base + WRITE, :A] = enc(store[q].astype(np.uint64))
            if kind == "big":                                                # about a third of the cells as raw words >= P next to their residues
                for c in (KEY, CLOCK, VALUE, WRITE):
                    col = data[base + c]
                    col[:A][(rng.random(A) < 0.3) & (col[:A] < P)] += np.uint32(P)
            link = b.derive_links(sel, (GROUP_DATA, base + KEY), [(GROUP_DATA, base + CLOCK), (GROUP_DATA, base + VALUE)],
                                  list(range(base + DST0, base + DST0 + N_DST)), 8, write=(GROUP_DATA, base + WRITE), joins=head)
            head = head or link
            rec += 1
    if kind == "mixed":                                                      # ... and one added after them moves every LINK, and the heads the joiners name
        b.derive_limbs((GROUP_CODE, 3), [wd - 2], 16)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code.reshape(-1), data.reshape(-1), po2, zk


# ---- SYN-LOOKUP-reads-ported at MULTI: the experiment of the issue
SYN = [(8, 40, 8), (8, 40, 1 << 20), (10, 200, 8), (10, 200, 1 << 20)]        # (po2, zk, the addresses' range)


@functools.lru_cache(maxsize=None)
def syn(po2, zk, addr_range, seed=3):
    """-> a dict: desc, the ported blob (version 9), the blob of separate memories over the same columns (version 6), the flag-free blob, code,
    the host-made witness `full` and `bare`, the one the library derives from (limbs, link columns and multiplicities zero), out"""
    desc, blob = sl.build_syn_lookup(MULTI, derive=True, limbs=True, link=True, reads=True, ports=True)
    same, apart = sl.build_syn_lookup(MULTI, derive=True, limbs=True, link=True, reads=True)
    code, full, out = sl.witness(MULTI, po2, zk, seed=seed, addr_range=addr_range, link=True, reads=True, ports=True)
    _, bare, _ = sl.witness(MULTI, po2, zk, seed=seed, addr_range=addr_range, count=False, limbs=False, link=False, reads=True, ports=True)
    return {"desc": desc, "same": same, "blob": blob, "apart": apart, "plain": logup.Arguments.parse(blob).plain().blob(), "code": code, "full": full, "bare": bare,
            "out": out, "args": logup.Arguments.parse(blob)}


def columns(order_limbs=sl.ORDER_LIMBS):
    """MULTI's per-port data columns [addr, val, time, linked, last, pval, ptime, limbs ..] and write flags"""
    return sl.link_layout(MULTI.n_words, MULTI.n_limbs, MULTI.n_mem, order_limbs), sl.reads_layout(MULTI.n_words, MULTI.n_limbs, MULTI.n_mem, order_limbs)


def accesses(data, po2, zk):
    """the accesses of MULTI's one memory in (row, port) order -> [(row, port, address, is store, linked, last, the (row, port) of the access before it
    to its address or None)] from the host-made columns and a walk"""
    n, A = 1 << po2, (1 << po2) - zk
    d = np.asarray(data).reshape(-1, n)
    lcols, wcols = columns()
    out, seen = [], {}
    for r in range(A):
        for q, c in enumerate(lcols):
            a = int(dec(d[c[0], r]))
            out.append((r, q, a, d[wcols[q], r] != 0, d[c[3], r] != 0, d[c[4], r] != 0, seen.get(a)))
            seen[a] = (r, q)
    return out


PAGED_SEED = 4                                  # a seed of `paged` under which an address is first touched through port 2 and last through port 0


@functools.lru_cache(maxsize=None)
def paged(po2=8, zk=40, seed=PAGED_SEED, tied=False, shape=MULTI):
    """the ported paged witness over an image of W words -> a dict like `syn`'s, with the image and the host walk's page table as ZKU1 rows"""
    desc, blob = sl.build_syn_lookup(shape, derive=True, limbs=True, link=True, reads=True, ports=True, pages=True, tied=tied)
    args = logup.Arguments.parse(blob)
    image = np.random.default_rng(seed).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, full, _ = sl.witness(shape, po2, zk, seed=seed, link=True, reads=True, ports=True, pages=True, image=image)
    _, bare, _ = sl.witness(shape, po2, zk, seed=seed, count=False, limbs=False, link=False, reads=True, ports=True, pages=False, image=image)
    n, A = 1 << po2, (1 << po2) - zk
    d, pg = full.reshape(-1, n), args.pages
    on = d[pg.p_on, :A] == ONE
    table = np.array([(int(a), int(i), int(o)) for a, i, o in zip(dec(d[pg.p_addr, :A][on]), d[pg.p_in, :A][on], d[pg.p_out, :A][on])], dtype=np.uint32)
    after = image.copy()
    after[table[:, 0]] = table[:, 2]
    return {"desc": desc, "blob": blob, "args": args, "plain": args.plain().blob(), "code": code, "full": full, "bare": bare, "image": image, "table": table,
            "after": after, "out": np.zeros(sl.TIED_OUT if tied else 4, dtype=np.uint32)}


def overfull(spread=True):
    """-> (desc, blob, code, data, image, po2, zk): 2 ports over 6 active rows of an 8-row trace, every access a store with a clock that rises.
    spread: the 12 accesses touch 12 addresses, twice what the page table has rows; else port 1 touches port 0's address of its row: 6 pages"""
    b = logup.LogupBuilder((4, 4, 40), (4, 8))
    b.term(0, [(GROUP_DATA, 39)], tag=1)
    link = lambda base, **kw: b.derive_links(None, (GROUP_DATA, base), [(GROUP_DATA, base + 1), (GROUP_DATA, base + 2)], list(range(base + 4, base + 11)), 8,
                                             write=(GROUP_DATA, base + 3), **kw)
    head = link(0)
    link(11, joins=head)
    b.derive_pages(head, list(range(22, 33)), 8)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0)))
    n, A = 8, 6
    data = np.zeros((40, n), dtype=np.uint32)
    for q in range(2):
        data[11 * q, :A], data[11 * q + 1, :A], data[11 * q + 3, :A] = enc(np.arange(A) * 2 + (q if spread else 0)), enc(np.arange(A) * 2 + q + 1), ONE
    return desc, blob, np.zeros(4 * n, dtype=np.uint32), data.reshape(-1), np.zeros(16, dtype=np.uint32), 3, 2


OVERFULL = "record 2: the trace pages 12 addresses, but the page table has the 6 active rows"


# ---- forgeries: -> (data, the reference's words), the refusal named being the lowest (record, row) by construction
def _record(args, port):
    return [i for i, r in enumerate(args.records) if isinstance(r, logup.Link)][port]


def _shared_row(acc, want):
    """the first row in which ports 0 and 1 touch one address and want(port 0's access, port 1's access, the accesses after them) holds"""
    for i, a in enumerate(acc[:-1]):
        if a[1] == 0 and acc[i + 1][2] == a[2] and want(a, acc[i + 1], [x for x in acc[i + 2:] if x[2] == a[2]]):
            return a[0]
    raise AssertionError("no such row in this witness")


def forge(what, case, po2, zk):
    """what: `clock` port 1's clock is port 0's at the same row and address; `load` a load through port 1 does not return what port 0 stored in the
    same row; `range` port 1's clock leaves a difference to port 0's that does not fit the limbs; (paged) `clock0` clock 0 on a joiner's first
    access to an address; `outside` an address outside the image on a joiner.  Each touches an access after which nothing reads what it left
    (or, `clock` and `clock0`, leaves a smaller clock behind), so that no other row is refused"""
    n = 1 << po2
    d = np.array(case["full"], dtype=np.uint32).reshape(-1, n)
    lcols, _ = columns()
    acc = accesses(case["full"], po2, zk)
    args = case["args"]
    x = lambda c, r: int(dec(d[c, r]))
    if what == "clock":
        r = _shared_row(acc, lambda a0, a1, later: True)
        d[lcols[1][2], r] = d[lcols[0][2], r]
        t = x(lcols[0][2], r)
        return d.reshape(-1), f"record {_record(args, 1)} at row {r}: clock not increasing ({t} after {t} at row {r} of record {_record(args, 0)})"
    if what == "load":                          # the next access of the address, if any, is a store: it reads nothing
        r = _shared_row(acc, lambda a0, a1, later: a0[3] and not a1[3] and (not later or later[0][3]))
        d[lcols[1][1], r] = (int(d[lcols[1][1], r]) + ONE) % P
        return d.reshape(-1), (f"record {_record(args, 1)} at row {r}: a load of carried column 1 returns {x(lcols[1][1], r)}, but {x(lcols[0][1], r)} was last stored "
                               f"(row {r} of record {_record(args, 0)})")
    if what == "range":                         # a joiner's access after another port's, the last of its address: no later clock is measured against it
        r, q, _, _, _, _, (pr, pq) = next(a for a in acc if a[1] >= 1 and a[5] and a[6] is not None and a[6][1] != a[1])
        d[lcols[q][2], r] = enc(x(lcols[pq][2], pr) + 1 + (1 << 12))
        return d.reshape(-1), (f"record {_record(args, q)} at row {r}: the clock difference {1 << 12} (after row {pr} of record {_record(args, pq)}) does not fit 3 limbs "
                               f"of 4 bits")
    # a joiner's access: `clock0` the first of its address (the later ones measure against a smaller clock), `outside` the last (nothing reads what it left)
    r, q = next(a for a in acc if a[1] >= 1 and (not a[4] if what == "clock0" else a[5]))[:2]
    if what == "clock0":
        d[lcols[q][2], r] = 0
        return d.reshape(-1), f"record {_record(args, q)} at row {r}: clock 0 is the image's"
    assert what == "outside"
    d[lcols[q][0], r] = enc(W)
    return d.reshape(-1), f"record {_record(args, q)} at row {r}: address {W} outside the image of {W} words"
