"""Witnesses shared by test_check_bus.py (reference_bus against the accumulate's own test and against hand-stated numbers) and
test_check_bus_gpu.py (zkh_check_bus against reference_bus).  Every case is built once per process and handed out read-only.

A case is (desc, blob, po2, zk, code, data): raw Montgomery words, `blob` the arguments the bus is checked under."""
import functools

import numpy as np

import check_rows_cases as rows_cases
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA, P

ONE = (1 << 32) % P
TINY, MULTI = syn_lookup.TINY, syn_lookup.MULTI
enc, frozen = rows_cases.enc, rows_cases.frozen
SIZES = [(8, 40), (9, 100), (10, 300)]                    # (po2, zk_cycles)
ADDR_RANGE = {8: 16, 9: 32, 10: 64}
MIX = rows_cases.mix_words(77)                            # the suites' way of fixing a mix (the bus itself reads none)


# ---- SYN-LOOKUP: honest witnesses of every variant, as the host leaves them (`zero`) and as the derives complete them (`full`) ----
VARIANTS = {
    # name: (shape, build_syn_lookup flags, witness flags of the full witness, witness flags of what the host uploads)
    "plain": (TINY, {}, {}, {}),
    "derived": (TINY, dict(derive=True), {}, dict(count=False)),
    "sorted": (TINY, dict(sort=True), {}, dict(sort=False)),
    "ordered": (TINY, dict(order=True, derive=True, sort=True, limbs=True), dict(order=True), dict(order=False, count=False, sort=False, limbs=False)),
    "linked": (TINY, dict(link=True, derive=True, limbs=True), dict(link=True), dict(link=False, count=False, limbs=False)),
    "reads": (TINY, dict(link=True, reads=True, derive=True, limbs=True), dict(link=True, reads=True), dict(link=False, reads=True, count=False, limbs=False)),
    "multi_sorted": (MULTI, dict(sort=True), {}, dict(sort=False)),
}


@functools.lru_cache(maxsize=None)
def circuit(variant):
    """-> (desc, blob)"""
    shape, flags, _full, _zero = VARIANTS[variant]
    return syn_lookup.build_syn_lookup(shape, **flags)


@functools.lru_cache(maxsize=None)
def honest(variant, po2, zk):
    """-> (desc, blob, po2, zk, code, data, uploaded): `data` the finished witness, `uploaded` what the host hands over before the derives"""
    shape, _flags, full, zero = VARIANTS[variant]
    kw = {} if variant in ("plain", "derived", "sorted", "multi_sorted") else {"addr_range": ADDR_RANGE[po2]}
    code, data, _out = syn_lookup.witness(shape, po2, zk, seed=po2, **full, **kw)
    _code, uploaded, _out = syn_lookup.witness(shape, po2, zk, seed=po2, **{**full, **zero}, **kw)
    return circuit(variant) + (po2, zk) + frozen(code, data, uploaded)


# ---- the forged witnesses of the logup suites ----
FORGERIES = ("corrupt_limb", "swap_sorted_rows", "relink_row", "misread_row", "wrong_pval", "sorted_value_tiny", "sorted_value_multi",
             "unsorted_tiny", "unsorted_multi")
BALANCED = ("swap_sorted_rows", "relink_row", "misread_row")              # these break a constraint, not the bus


@functools.lru_cache(maxsize=None)
def forgery(kind, po2=10, zk=300):
    """-> (desc, blob, po2, zk, code, data)
      corrupt_limb, swap_sorted_rows, relink_row, misread_row: check_rows_cases.lookup_forgery
      wrong_pval          tests/test_logup_links.py: one pval of SYN-LOOKUP-linked raised by one
      sorted_value_*      tests/test_logup_sorted.py: one value of one sorted row raised by one (TINY by (addr, time); MULTI by addr alone)
      unsorted_*          the same witnesses with the sorted copy left zero"""
    n, A = 1 << po2, (1 << po2) - zk
    if kind in rows_cases.FORGERIES:
        variant, _accum, code, data, _out, _mix, _row, _cols = rows_cases.lookup_forgery(kind, po2, zk)
        return rows_cases.lookup_circuit(variant) + (po2, zk, code, data)
    if kind == "wrong_pval":
        desc, blob = syn_lookup.build_syn_lookup(TINY, link=True, derive=True, limbs=True)
        code, data, _out = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=ADDR_RANGE[po2], link=True)
        lcols = syn_lookup.link_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0]
        wrong = data.reshape(-1, n).copy()
        r2 = next(r for r in range(A // 3, A) if wrong[lcols[3], r] == ONE)
        wrong[lcols[5], r2] = (int(wrong[lcols[5], r2]) + ONE) % P
        return (desc, blob, po2, zk) + frozen(code, wrong.reshape(-1))
    shape, keys, wit = (TINY, (0, 2), syn_lookup.witness) if kind.endswith("tiny") else (MULTI, (0,), syn_lookup.witness_equal_keys)
    desc, blob = syn_lookup.build_syn_lookup(shape, sort=True, sort_keys=keys)
    code, zero, _out = wit(shape, po2, zk, seed=4, sort=False)
    if kind.startswith("unsorted"):
        return (desc, blob, po2, zk) + frozen(code, zero)
    data = logup.reference_sorted(logup.Arguments.parse(blob), po2, zk, code, zero)
    perm = syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)[4]
    bad = data.reshape(-1, n).copy()
    bad[perm[-1][1], 77] = (int(bad[perm[-1][1], 77]) + ONE) % P
    return (desc, blob, po2, zk) + frozen(code, bad.reshape(-1))


# ---- a hand-built pair: 3 code and 5 data columns, two terms of tag 5 in one accum column ----
#   term 0: + sel code[0] m data[2] (data[0])            a width-1 tuple
#   term 1: -             m data[3] (data[1], data[4])   a width-2 tuple: with data[4] = 0 the same keys
PAIR_TAG = 5


@functools.lru_cache(maxsize=None)
def pair_circuit():
    b = logup.LogupBuilder((4, 3, 5), (4, 8))
    b.term(0, [(GROUP_DATA, 0)], sign=1, sel=0, mult=(GROUP_DATA, 2), tag=PAIR_TAG)
    b.term(0, [(GROUP_DATA, 1), (GROUP_DATA, 4)], sign=-1, mult=(GROUP_DATA, 3), tag=PAIR_TAG)
    return b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))


def pair(po2, zk, key, key2=None, sel=1, m=1, m2=1, pad=0, raw=None):
    """-> a case over pair_circuit: the canonical values of data[0] (`key`), data[1] (`key2`, default: the same), code[0] (`sel`),
    data[2] (`m`), data[3] (`m2`), data[4] (`pad`) on the active rows, a scalar or one value per row; the blinding rows and the unused
    code columns are random words.  raw: {(group, column): rows} whose words get P added (another word of the same residue)"""
    n, A = 1 << po2, (1 << po2) - zk
    rng = np.random.default_rng(po2 * 1000 + zk)
    code = rng.integers(0, P, size=(3, n), dtype=np.uint64).astype(np.uint32)
    data = rng.integers(0, P, size=(5, n), dtype=np.uint64).astype(np.uint32)
    col = lambda v: enc(np.broadcast_to(np.asarray(v, dtype=np.uint64), (A,)))
    code[0, :A] = col(sel)
    for c, v in ((0, key), (1, key if key2 is None else key2), (2, m), (3, m2), (4, pad)):
        data[c, :A] = col(v)
    for (g, c), at in (raw or {}).items():
        t = code if g == GROUP_CODE else data
        t[c, at] = (t[c, at].astype(np.uint64) + np.uint64(P)).astype(np.uint32)          # 2 P < 2^32
    return pair_circuit() + (po2, zk) + frozen(code.reshape(-1), data.reshape(-1))


def _rows(A, **at):
    """a column of ones with the given rows set: _rows(A, r5=0) is 1 everywhere and 0 on row 5"""
    v = np.ones(A, dtype=np.uint64)
    for k, x in at.items():
        v[int(k[1:])] = x
    return v


@functools.lru_cache(maxsize=None)
def hand(name):
    """the hand-built cases, by name -> a case; HAND lists what each must give"""
    po2, zk = 9, 100
    A = (1 << po2) - zk                                                       # 412: no multiple of 64
    base = 1000 + np.arange(A, dtype=np.uint64)                               # a key per row
    if name == "balanced":
        return pair(po2, zk, base)
    if name == "report_order":
        # key 1200: + weight 2 against - weight 1, representative (term 0, row 200); key 7: on term 1 alone at row 10 (the + side of
        # row 10 has weight 0, so 1010 is no key): representative (term 1, row 10).  Term-major order reports (0, 200).
        k2 = base.copy(); k2[10] = 7
        return pair(po2, zk, base, k2, m=_rows(A, r200=2, r10=0))
    if name == "representative":
        # key 1005 on rows 5 and 300 of both terms; the error is term 1's weight 3 on row 300; the representative is (term 0, row 5)
        k = base.copy(); k[300] = 1005
        return pair(po2, zk, k, m2=_rows(A, r300=3))
    if name == "raw_words":
        # the same residues as other words on both sides; key 0 as the raw word P on the + side of row 9 and as 0 on the - side
        k = base.copy(); k[9] = 0
        at = np.arange(0, A, 3)
        return pair(po2, zk, k, raw={(GROUP_DATA, 0): np.union1d(at, [9]), (GROUP_DATA, 1): at[at != 9] + 0, (GROUP_DATA, 2): at, (GROUP_CODE, 0): at})
    if name == "sum_of_p":
        # rows 20 and 21 hold key 4444 on the + side with weights P - 1 and 1 and nothing on the - side: 64-bit sums P and 0, net 0
        k = base.copy(); k[20] = k[21] = 4444
        return pair(po2, zk, k, m=_rows(A, r20=P - 1, r21=1), m2=_rows(A, r20=0, r21=0))
    if name == "net_p_minus_3":
        # key 1030 on the - side alone, weight 3
        return pair(po2, zk, base, m=_rows(A, r30=0), m2=_rows(A, r30=3))
    if name == "weights":
        # selector 2 x multiplicity 3 against one - entry of 6 on every row; row 40's + side has weight 0 and a key found nowhere else
        k = base.copy(); k[40] = 999999
        k2 = base.copy()
        return pair(po2, zk, k, k2, sel=_rows(A, r40=0) * 2, m=3, m2=_rows(A, r40=0) * 6)
    if name == "padding":
        return pair(po2, zk, base, pad=0)
    if name == "padding_one_cell":
        # (1050) against (1050, 8): two keys
        pad = np.zeros(A, dtype=np.uint64); pad[50] = 8
        return pair(po2, zk, base, pad=pad)
    raise KeyError(name)


# name: (term, row, key, net, unbalanced_keys, distinct_keys), stated by hand
HAND = {
    "balanced": (-1, -1, (0, 0, 0, 0), 0, 0, 412),
    "report_order": (0, 200, (1200, 0, 0, 0), 1, 2, 412),                    # 411 keys of the + side (row 10 has no weight) and key 7
    "representative": (0, 5, (1005, 0, 0, 0), P - 2, 1, 411),
    "raw_words": (-1, -1, (0, 0, 0, 0), 0, 0, 412),
    "sum_of_p": (-1, -1, (0, 0, 0, 0), 0, 0, 411),
    "net_p_minus_3": (1, 30, (1030, 0, 0, 0), P - 3, 1, 412),
    "weights": (-1, -1, (0, 0, 0, 0), 0, 0, 411),                            # row 40 has no entry on either side
    "padding": (-1, -1, (0, 0, 0, 0), 0, 0, 412),
    "padding_one_cell": (0, 50, (1050, 0, 0, 0), 1, 2, 413),
}


# ---- contention and lanes: how the rows fall onto slots, waves and workgroups ----
CONTENTION = ("one_key", "distinct", "runs_of_37", "few_keys", "below_a_wave", "one_row", "two_workgroups_and_a_bit")


@functools.lru_cache(maxsize=None)
def contention(name):
    if name == "one_key":                                                     # A entries of each term in one slot: every lane of every wave equal
        return pair(10, 300, 31)
    if name == "distinct":
        return pair(10, 300, 5 + 7 * np.arange(724, dtype=np.uint64))
    if name == "runs_of_37":                                                  # equal slots straddle wave and workgroup boundaries
        return pair(10, 300, np.arange(724, dtype=np.uint64) // 37, m=2, m2=2)
    if name == "few_keys":                                                    # 5 keys in a fixed shuffle, one - weight off: a hot unbalanced key
        k = (np.arange(724, dtype=np.uint64) * 7919) % 5
        return pair(10, 300, k, m2=_rows(724, r700=2))
    if name == "below_a_wave":                                                # A = 50
        return pair(6, 14, np.arange(50, dtype=np.uint64) % 9, m2=_rows(50, r49=5))
    if name == "one_row":                                                     # A = 1
        return pair(4, 15, 3, m=2)
    if name == "two_workgroups_and_a_bit":                                    # A = 513
        return pair(10, 511, np.arange(513, dtype=np.uint64) % 100, m=_rows(513, r512=4))
    raise KeyError(name)


def reference(case):
    desc, blob, po2, zk, code, data = case[:6]
    return logup.reference_bus(logup.Arguments.parse(blob), po2, zk, code, data)


def same(got, want):
    """field for field: the scalar fields, the per-term table, and the line (None when nothing is reported)"""
    scalars = ("term", "row", "tag", "key", "net", "unbalanced_keys", "distinct_keys", "slots")
    assert {k: got[k] for k in scalars} == {k: want[k] for k in scalars}
    assert np.array_equal(got["per_term"], want["per_term"]), (got["per_term"], want["per_term"])
