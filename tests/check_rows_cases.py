"""Witnesses and hand-built descriptions shared by test_check_rows.py (the reference against the oracle) and test_check_rows_gpu.py
(the library against the reference).  Every witness is built once per process and handed out read-only."""
import functools

import numpy as np

import zko
from zeth_amd.circuits import keccak_f as K, logup, recursion as R, syn_air, syn_lookup
from zeth_amd.circuits.desc import GROUP_ACCUM, GROUP_CODE, GROUP_DATA, CircuitBuilder, P

ONE = (1 << 32) % P
TINY = syn_lookup.TINY
SIZES = [(8, 40), (10, 300), (12, 1994)]                  # (po2, zk_cycles) of the CPU modules of the same circuits
ADDR_RANGE = {8: 16, 10: 64, 12: 5}
LOOKUP_VARIANTS = ("plain", "ordered", "linked", "reads")


def enc(x) -> np.ndarray:
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def mix_words(seed, k=8) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, P, k, dtype=np.uint64).astype(np.uint32)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- syn_tiny: the oracle's witness and accum ----
@functools.lru_cache(maxsize=None)
def syn_tiny_witness(po2, zk):
    """-> (desc, accum, code, data, out, mix)"""
    oracle = zko.load()
    desc = syn_air.syn_tiny()
    oc = zko.OracleCircuit(oracle, desc)
    code, data, out = oc.witgen(po2, zk)
    mix = mix_words(po2, int(desc[8]))
    accum = np.zeros(int(desc[3]) << po2, np.uint32)
    oracle.zko_syn_accum(oc.h, po2, zk, zko.key_words(0x2E80), data, mix, accum)
    return (desc,) + frozen(accum, code, data, out, mix)


# ---- SYN-LOOKUP TINY: plain, ordered, linked, reads; host-made witnesses (syn_lookup.witness) and the reference accumulate ----
@functools.lru_cache(maxsize=None)
def lookup_circuit(variant):
    """-> (desc, blob)"""
    return {"plain": lambda: syn_lookup.syn_lookup_tiny(),
            "ordered": lambda: syn_lookup.build_syn_lookup(TINY, order=True, derive=True, sort=True, limbs=True),
            "linked": lambda: syn_lookup.build_syn_lookup(TINY, link=True, derive=True, limbs=True),
            "reads": lambda: syn_lookup.build_syn_lookup(TINY, link=True, reads=True, derive=True, limbs=True)}[variant]()


@functools.lru_cache(maxsize=None)
def lookup_witness(variant, po2, zk):
    """-> (code, data, out, mix): the honest host-made traces"""
    kw = {"plain": {}, "ordered": {"order": True}, "linked": {"link": True}, "reads": {"link": True, "reads": True}}[variant]
    if variant != "plain":
        kw["addr_range"] = ADDR_RANGE[po2]
    code, data, out = syn_lookup.witness(TINY, po2, zk, seed=po2, **kw)
    return frozen(code, data, out, mix_words(po2))


def lookup_accum(variant, po2, zk, code, data, mix, check_balance=True):
    args = logup.Arguments.parse(lookup_circuit(variant)[1])
    accum, _total = logup.reference_accumulate(args, po2, zk, code, data, mix, check_balance=check_balance)
    return accum


@functools.lru_cache(maxsize=None)
def lookup_forgery(kind, po2, zk):
    """-> (variant, accum, code, data, out, mix, row, columns): a forged witness whose lowest failing row is `row`, and the (group,
    column) pairs of which the failing constraint must read at least one.
      bad_accum    (plain)   one accum cell moved, as in test_logup.py: the running sum of its column objects on the row
      corrupt_limb (plain)   a limb outside the table with its word moved along: only the bus objects, on the last active row; the
                             constraint reads the accum columns' totals, the forged limb's column among them
      swap_sorted_rows (ordered), relink_row (linked), misread_row (reads): as in test_logup_columns / _links / _reads.py"""
    n, A = 1 << po2, (1 << po2) - zk
    variant = {"bad_accum": "plain", "corrupt_limb": "plain", "swap_sorted_rows": "ordered", "relink_row": "linked", "misread_row": "reads"}[kind]
    code, data, out, mix = lookup_witness(variant, po2, zk)
    args = logup.Arguments.parse(lookup_circuit(variant)[1])
    balance = True
    if kind == "bad_accum":
        accum = lookup_accum(variant, po2, zk, code, data, mix)
        accum[n * 5 + 7] ^= 1
        return (variant,) + frozen(accum, code, data, out, mix) + (7, ((GROUP_ACCUM, 5),))
    if kind == "corrupt_limb":
        row, word = A // 3, 1
        forged, balance = syn_lookup.corrupt_limb(TINY, data, po2, row=row, word=word), False
        limb = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[1][word][0]
        term = next(t for t in args.terms if tuple(t.tuple_cols) == ((GROUP_DATA, limb),))
        row, cols = A - 1, tuple((GROUP_ACCUM, 4 * term.col + j) for j in range(4))
    elif kind == "swap_sorted_rows":
        row = A // 2
        forged = syn_lookup.swap_sorted_rows(TINY, data, po2, row)
        cols = tuple((GROUP_DATA, c) for c in syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[4][0])
    elif kind == "relink_row":
        lcols = syn_lookup.link_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0]
        w = data.reshape(-1, n)
        row = next(r for r in range(A // 2, A) if (w[lcols[0], r + 1:A] == w[lcols[0], r]).any())
        f = syn_lookup.relink_row(TINY, data, po2, row).reshape(-1, n)
        f[10, :A] = 0                                    # the multiplicities counted again, the forged limbs included
        counted = logup.Arguments.parse(syn_lookup.build_syn_lookup(TINY, link=True, derive=True)[1])
        forged = logup.reference_multiplicities(counted, po2, zk, code, f.reshape(-1))
        cols = tuple((GROUP_DATA, c) for c in lcols[3:])                     # linked, last, pval, ptime and the limbs
    else:
        f, row = syn_lookup.misread_row(TINY, data, po2, zk)
        f = f.reshape(-1, n).copy()
        f[10, :A] = 0
        forged = logup.reference_multiplicities(args, po2, zk, code, f.reshape(-1))
        cols = ((GROUP_DATA, syn_lookup.link_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0][1]),)    # val
    accum, _ = logup.reference_accumulate(args, po2, zk, code, forged, mix, check_balance=balance)
    return (variant,) + frozen(accum, code, forged, out, mix) + (row, cols)


FORGERIES = ("bad_accum", "corrupt_limb", "swap_sorted_rows", "relink_row", "misread_row")


# ---- KECCAK-F at po2 8: six permutations, the last one the padded block of a message ----
def _keccak_pub(msg):
    return np.array([w for lane in K.sha3_256_block(msg) for w in (lane & 0xFFFFFFFF, lane >> 32)], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def keccak_witness(po2=8, zk=40):
    """-> (desc, accum, code, data, out, claimed, mix, bind_row): `claimed` = the honest output with ANOTHER input claimed"""
    oracle = zko.load()
    desc = K.keccak_f_circuit()
    oc = zko.OracleCircuit(oracle, desc)
    code, data, out = oc.witgen(po2, zk, seed=1, noise_seed=2, pub=_keccak_pub(b"zeth: keccak accelerator call"))
    n = 1 << po2
    mix = np.array([5, 6, 7, 8], dtype=np.uint32)
    accum = np.zeros(4 * n, dtype=np.uint32)
    oracle.zko_syn_accum(oc.h, po2, zk, zko.key_words(2), data, mix, accum)
    claimed = out.copy()
    claimed[100:200] = enc(K.out_words(K.sha3_256_block(b"another message")))
    return (desc,) + frozen(accum, code, data, out, claimed, mix) + (25 * ((n - zk) // 25 - 1),)


# ---- RECURSION: a small program through the oracle's witness generator ----
REC_MIX = np.array([(i * 7919 + 13) * ONE % P for i in range(20)], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def recursion_witness():
    """-> (desc, po2, accum, code, data, out, mix)"""
    oracle = zko.load()
    pr = R.Program()
    x, y = pr.input(0, 4), pr.input(4, 4)
    s, m = pr.add(x, y), pr.mul(x, y)
    iv = pr.inv(m)
    pr.eq(pr.mul(m, iv), pr.const(1))
    a, b, _, _ = pr.unpack(x)
    bits = pr.bits31(a, 12)
    sel = pr.mux(bits[0], s, m)
    h = pr.p2([x, y, s, m, pr.zero(), pr.zero()])
    sw = pr.p2([h[0], h[1], x, y, bits[0], pr.zero()], swap=True)
    pr.eq(pr.is_zero(b), pr.zero())
    pr.public(h[0], sw[1], pr.pack(2, x, y, s, m), pr.mul(pr.const(3, 1, 4, 1), sel))
    zk = 50
    po2 = pr.min_po2(zk)
    desc = R.recursion_circuit()
    rec = zko.OracleCircuit(oracle, desc)
    code, data, out = rec.rec_witgen(pr.finish(po2, zk), enc([5, 6, 7, 8, 11, 12, 13, 14]))
    accum = rec.rec_accum(po2, code, data, REC_MIX, zk)
    return (desc, po2) + frozen(accum, code, data, out, REC_MIX.copy())


# ---- hand-built descriptions for F itself: 1 accum, 1 code and 4 data columns, 2 out and 4 mix words, 8 rows ----
HAND_PO2 = 3
HAND_GROUPS, HAND_GLOBALS = (1, 1, 4), (2, 4)


def hand_trace(d0=0, d1=0, d2=0, d3=0, accum=0, code=0):
    """-> (accum, code, data) raw traces; every argument is one canonical value or eight (one per row)"""
    col = lambda v: enc(np.broadcast_to(np.asarray(v, dtype=np.uint64), (1 << HAND_PO2,)))
    return col(accum), col(code), np.concatenate([col(d0), col(d1), col(d2), col(d3)])


HAND_OUT, HAND_MIX = enc([3, 4]), enc([5, 6, 7, 8])


def hand_cond(ext_cond=False):
    """ret = and_cond(true, cond, and_eqz(true, d0)), cond = d1 (or the Fp4 (0, 0, d1, 0)) -> (desc, the and_eqz step)"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    d0, d1 = b.get(GROUP_DATA, 0), b.get(GROUP_DATA, 1)
    cond = b.mul(b.const_ext(0, 0, 1, 0), d1) if ext_cond else d1
    inner = b.and_eqz(b.true(), d0)
    step = len(b.steps) - 1
    return b.finish(b.and_cond(b.true(), cond, inner)), step


def hand_nested():
    """ret = and_cond(true, d2, and_cond(true, d1, and_eqz(true, d0))) -> (desc, the and_eqz step, [outer and_cond, inner and_cond])"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    d0, d1, d2 = (b.get(GROUP_DATA, c) for c in range(3))
    leaf = b.and_eqz(b.true(), d0)
    step = len(b.steps) - 1
    mid = b.and_cond(b.true(), d1, leaf)
    mid_step = len(b.steps) - 1
    ret = b.and_cond(b.true(), d2, mid)
    return b.finish(ret), step, [len(b.steps) - 1, mid_step]


def hand_ext_value():
    """ret = and_eqz(true, (0, 0, 0, 1) * d0): an Fp4 that is non-zero in component 3 alone -> (desc, step)"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    ret = b.and_eqz(b.true(), b.mul(b.const_ext(0, 0, 0, 1), b.get(GROUP_DATA, 0)))
    return b.finish(ret), len(b.steps) - 1


def hand_two_failures():
    """ret = and_cond(and_eqz(true, d1), 1, and_eqz(true, d0)): the inner chain was built first, so its step is the LOWER one although
    the chain from ret meets the other first -> (desc, step of d0's and_eqz, step of d1's and_eqz)"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    d0, d1 = b.get(GROUP_DATA, 0), b.get(GROUP_DATA, 1)
    inner = b.and_eqz(b.true(), d0)
    low = len(b.steps) - 1
    x = b.and_eqz(b.true(), d1)
    high = len(b.steps) - 1
    return b.finish(b.and_cond(x, b.const(1), inner)), low, high


def hand_back3():
    """ret = and_eqz(true, d0 - d1@3): d0[r] = d1[r - 3 mod n] -> (desc, step)"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    ret = b.and_eqz(b.true(), b.sub(b.get(GROUP_DATA, 0), b.get(GROUP_DATA, 1, 3)))
    return b.finish(ret), len(b.steps) - 1


def hand_globals():
    """ret = and_eqz(true, d0 * out[1] - mix[2] * code0) -> (desc, step)"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    ret = b.and_eqz(b.true(), b.sub(b.mul(b.get(GROUP_DATA, 0), b.get_global(0, 1)), b.mul(b.get_global(1, 2), b.get(GROUP_CODE, 0))))
    return b.finish(ret), len(b.steps) - 1


def live_ext_desc(k=400):
    """k Fp4 values all live at once (each is read only after the last is made): more than the step interpreter's LDS holds"""
    b = CircuitBuilder(HAND_GROUPS, HAND_GLOBALS, kind=0)
    d0 = b.get(GROUP_DATA, 0)
    vals = [b.mul(b.const_ext(1, i + 1, 0, 0), d0) for i in range(k)]
    tot = vals[0]
    for v in vals[1:]:
        tot = b.add(tot, v)
    return b.finish(b.and_eqz(b.true(), tot))
