"""The read rule of LINK records (ZKA1 version 6; zeth_amd/circuits/logup.py, csrc/arguments.hip's validator): a load returns the last
store.  The builder and parser of the version-6 blob, a blob without READS still the version-5 blob it was, the new rules in the builder,
the parser and the C validator on a GPU-less circuit with equal messages, the host reference against a walk over the rows with a
dictionary on random load / store traces, its refusals and their order, and SYN-LOOKUP-reads against the oracle's row checker: the
honest witness holds, a forged load fails on its row although the bus balances, and the same forged values satisfy every constraint of
SYN-LOOKUP-linked, which has no read rule.  No GPU."""
import hashlib
import re
from dataclasses import replace

import numpy as np
import pytest

import zko
from conftest import rand_fp
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_ACCUM, GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError

P = 2013265921
ONE = (1 << 32) % P
RINV = pow(ONE, -1, P)
TINY, FULL = syn_lookup.TINY, syn_lookup.FULL
NONE = logup.NONE
_digest = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()[:16]


def _enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


# ---- the version-6 blob ----
N_TERMS = 5
REC_AT = [logup.ARGS_HEADER + 16 * N_TERMS + off for off in (0, 16, 48, 80)]    # record 0: LIMBS (16 words); records 1, 2, 3: LINK (32 words)
SIZES = (8, 6, 40)
WORDS = REC_AT[3] + 32


def _term(i, w):
    return logup.ARGS_HEADER + logup.TERM_WORDS * i + w


def _rec(i, w):
    return REC_AT[i] + w


def _builder(reads=True):
    """record 1: READS, a selector, nc = 2, the write flag data 22; record 2: no READS, nc = 1; record 3: READS, nc = 3 (the second value
    column a code column), the write flag code 0.  reads = False: the same records without READS"""
    b = logup.LogupBuilder(SIZES, (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1)                                          # term 0
    b.term(0, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, tag=1, sorted_from=0, sort_keys=(0, 1))  # term 1: sorted columns 2, 3
    b.term(1, [(GROUP_CODE, 1)], sign=-1, mult=(GROUP_DATA, 4), tag=0, derive=True)               # term 2: derived multiplicity 4
    r0 = b.derive_limbs((GROUP_CODE, 2), [5, 6, 7], 5)
    r1 = b.derive_links(3, (GROUP_DATA, 8), [(GROUP_DATA, 9), (GROUP_DATA, 10)], [11, 12, 13, 14, 15, 16, 17], 8,
                        write=(GROUP_DATA, 22) if reads else None)
    r2 = b.derive_links(None, (GROUP_CODE, 4), [(GROUP_DATA, 18)], [19, 20, 21], 4)
    r3 = b.derive_links(None, (GROUP_DATA, 23), [(GROUP_DATA, 24), (GROUP_DATA, 25), (GROUP_CODE, 5)], [26, 27, 28, 29, 30], 4,
                        write=(GROUP_CODE, 0) if reads else None)
    b.term(1, [(GROUP_DATA, 8), (GROUP_DATA, 14), (GROUP_DATA, 13)], sign=-1, mult=(GROUP_DATA, 11), tag=2)   # term 3: -linked (key, prev)
    b.term(1, [(GROUP_DATA, 15)], tag=0)                                                          # term 4: a lookup reads a limb
    return b, (r0, r1, r2, r3)


def _all(reads=True):
    b, _ = _builder(reads)
    return b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 0)))


def test_builder_round_trips_version_6():
    b, (r0, r1, r2, r3) = _builder()
    assert b.records == [r0, r1, r2, r3]
    assert (r1.write, r2.write, r3.write) == ((GROUP_DATA, 22), None, (GROUP_CODE, 0))
    assert r1.srcs == ((GROUP_DATA, 8), (GROUP_DATA, 9), (GROUP_DATA, 10), (GROUP_DATA, 22)) and r2.srcs == ((GROUP_CODE, 4), (GROUP_DATA, 18))
    a = b.args()
    blob = a.blob()
    assert blob[1] == 6 and blob[6] == 4 and blob[7] == 2 and blob.size == WORDS and a.reads == 2
    assert list(blob[_rec(1, 0):_rec(2, 0)]) == [3, 8, 3, 2, 3, 1, GROUP_DATA, 8, GROUP_DATA, 9, GROUP_DATA, 10, 0, 0, GROUP_DATA, 22,
                                                 11, 12, 13, 14, 15, 16, 17] + [0] * 9
    assert list(blob[_rec(2, 0):_rec(3, 0)]) == [3, 4, 0, 1, NONE, 0, GROUP_CODE, 4, GROUP_DATA, 18, 0, 0, 0, 0, 0, 0, 19, 20, 21] + [0] * 13
    assert list(blob[_rec(3, 0):]) == [3, 4, 0, 3, NONE, 1, GROUP_DATA, 23, GROUP_DATA, 24, GROUP_DATA, 25, GROUP_CODE, 5, GROUP_CODE, 0,
                                       26, 27, 28, 29, 30] + [0] * 11
    back = logup.Arguments.parse(blob)
    assert back.version == 6 and back.records == [r0, r1, r2, r3] and back.terms == a.terms
    assert np.array_equal(back.blob(), blob)
    plain = back.plain()
    assert plain.version == 1 and not plain.records and plain.blob()[7] == 0
    # without READS the same records are the version-5 blob: the version-6 words apart, word for word
    _, blob5 = _all(reads=False)
    assert blob5[1] == 5 and blob5[7] == 0 and blob5.size == WORDS
    differ = [int(w) for w in np.nonzero(blob5 != blob)[0]]
    assert differ == [1, 7, _rec(1, 5), _rec(1, 14), _rec(1, 15), _rec(3, 5), _rec(3, 14)]      # record 3's write flag is (code = 1, 0)
    assert np.array_equal(logup.Arguments.parse(blob5).blob(), blob5)


# the blobs and descriptions of SYN-LOOKUP-linked as they were before version 6 existed: (version, blob digest, description digest)
RECORDED = {
    (TINY, ("link",)): (5, "43f73eebe3d18dc3", "006bd6849cb7ec4e"), (TINY, ("link", "derive", "limbs")): (5, "ac4580a71b1c64ec", "006bd6849cb7ec4e"),
    (FULL, ("link",)): (5, "d2a0a1abd37b3896", "6ce7aa223e1d2a0a"), (FULL, ("link", "derive", "limbs")): (5, "fbc7e714b3ef8dbb", "6ce7aa223e1d2a0a"),
}


def test_a_blob_without_reads_is_byte_identical():
    for (shape, switches), want in RECORDED.items():
        desc, blob = syn_lookup.build_syn_lookup(shape, **{s: True for s in switches})
        assert (int(blob[1]), _digest(blob), _digest(desc)) == want, switches
    code, data, _ = syn_lookup.witness(TINY, 10, 300, seed=5, addr_range=64, link=True)
    assert (_digest(code), _digest(data)) == ("05d3073fd18abae7", "061698c6c06c1f7a")


READS_NC = r"READS needs a clock and a value column \(2\.\.3 carried columns\), this LINK carries 1"
RESERVED5 = r"a reserved word of a LINK is not 0 \(words 5, 14, 15, the unused carried pairs and the unused destination words\)"
# (edits of the blob of `_all()`, the message of the parser and of the C validator), in the order of the rules
BLOB_EDITS = [
    ([(7, 1)], "header word 7 is 1, the blob has 2 LINK records with READS"),
    ([(7, 3)], "header word 7 is 3, the blob has 2 LINK records with READS"),
    ([(_rec(1, 5), 0), (_rec(1, 14), 0), (_rec(1, 15), 0)], "header word 7 is 2, the blob has 1 LINK records with READS"),
    ([(_rec(1, 5), 3)], r"record 1: word 5 of a LINK is 0x3 \(bit 0: READS, the read rule; the other bits are reserved\)"),
    ([(_rec(3, 5), 0x80000001)], "record 3: word 5 of a LINK is 0x80000001"),
    ([(_rec(2, 5), 2)], "record 2: word 5 of a LINK is 0x2"),
    ([(_rec(2, 14), GROUP_DATA)], r"record 2: words 14, 15 of a LINK name a write flag, but bit 0 of word 5 \(READS\) is not set"),
    ([(_rec(2, 15), 31)], "record 2: words 14, 15 of a LINK name a write flag"),
    ([(7, 3), (_rec(2, 5), 1), (_rec(2, 14), GROUP_DATA), (_rec(2, 15), 31)], "record 2: " + READS_NC),
    ([(_rec(1, 12), GROUP_DATA)], "record 1: " + RESERVED5),                                     # the unused third carried pair, as in version 5
    ([(_rec(1, 14), GROUP_ACCUM)], r"record 1: source \(0, 22\) is not a code or data column"),
    ([(_rec(3, 14), 3)], r"record 3: source \(3, 0\) is not a code or data column"),
    ([(_rec(1, 15), 2)], r"record 1: its source \(data 2\) is written by the sorted copy term 1 \(a LINK reads what no derive writes\)"),
    ([(_rec(1, 15), 5)], r"record 1: its source \(data 5\) is a destination of record 0 \(records never chain\)"),
    ([(_rec(1, 15), 12)], r"record 1: its source \(data 12\) is a destination of record 1"),    # its own
    ([(_rec(1, 15), 27)], r"record 1: its source \(data 27\) is a destination of record 3"),
    ([(_rec(1, 15), 4)], r"record 1: its source \(data 4\) is the derived multiplicity of term 2"),
    ([(_rec(2, 18), 22)], r"record 1: its source \(data 22\) is a destination of record 2"),    # another record writes the write flag
]
# ... and what only a validator that knows the circuit can refuse (the builder and the C validator)
SHAPE_EDITS = [
    ([(_rec(1, 15), 40)], r"record 1: source \(2, 40\) is not a code or data column"),
    ([(_rec(3, 15), 6)], r"record 3: source \(1, 6\) is not a code or data column"),
]
# ... and what the rules allow
GOOD_EDITS = [
    [(_rec(1, 14), GROUP_CODE), (_rec(1, 15), 5)],                                               # a code write flag
    [(_rec(1, 15), 31)],
    [(_rec(3, 14), GROUP_DATA), (_rec(3, 15), 22)],                                              # two records read one write flag
    [(_rec(3, 14), GROUP_DATA), (_rec(3, 15), 10)],                                              # a write flag that another record carries
    [(7, 1), (_rec(3, 5), 0), (_rec(3, 14), 0), (_rec(3, 15), 0)],                               # one READS record of three LINKs
]


def _edited(blob, edit):
    bad = blob.copy()
    for w, v in edit:
        bad[w] = v
    return bad


def test_parser_refuses_every_rule():
    _, blob = _all()
    assert blob.size == WORDS and blob[1] == 6 and blob[7] == 2
    with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
        logup.Arguments.parse(_edited(blob, [(7, 0)]))
    with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
        logup.Arguments.parse(_edited(blob, [(1, 7)]))
    for edit, msg in BLOB_EDITS:
        with pytest.raises(ValueError, match="ZKA1: " + msg):
            logup.Arguments.parse(_edited(blob, edit))
    for edit in GOOD_EDITS:
        a = logup.Arguments.parse(_edited(blob, edit))
        assert np.array_equal(a.blob(), _edited(blob, edit))
    for edit, msg in SHAPE_EDITS:
        a = logup.Arguments.parse(_edited(blob, edit))
        assert logup.check_links(a.terms, a.records) is None
        assert re.search(msg, logup.check_links(a.terms, a.records, SIZES))
    # a version-5 blob keeps its own message for words 5, 14, 15 ...
    _, blob5 = _all(reads=False)
    for w, v in ((5, 1), (14, GROUP_DATA), (15, 22)):
        with pytest.raises(ValueError, match="ZKA1: record 1: " + RESERVED5):
            logup.Arguments.parse(_edited(blob5, [(_rec(1, w), v)]))
    # ... and leaves header word 7 unread, as it always was
    assert logup.Arguments.parse(_edited(blob5, [(7, 9)])).version == 5
    # marked version 6, the version-5 blob is no ZKA1 blob (its header word 7 is 0)
    with pytest.raises(ValueError, match="^not a ZKA1 argument blob$"):
        logup.Arguments.parse(_edited(blob5, [(1, 6)]))


def test_builder_refuses_and_keeps_its_state():
    b, _ = _builder()
    n = len(b.records)
    with pytest.raises(ValueError, match="record 4: " + READS_NC):
        b.derive_links(None, (GROUP_DATA, 8), [(GROUP_DATA, 9)], [32, 33, 34], 8, write=(GROUP_DATA, 22))
    with pytest.raises(ValueError, match=r"record 4: source \(2, 40\) is not a code or data column"):
        b.derive_links(None, (GROUP_DATA, 8), [(GROUP_DATA, 9), (GROUP_DATA, 10)], [32, 33, 34, 35], 8, write=(GROUP_DATA, 40))
    with pytest.raises(ValueError, match=r"record 4: source \(0, 1\) is not a code or data column"):
        b.derive_links(None, (GROUP_DATA, 8), [(GROUP_DATA, 9), (GROUP_DATA, 10)], [32, 33, 34, 35], 8, write=(GROUP_ACCUM, 1))
    for col, msg in ((5, r"record 4: its source \(data 5\) is a destination of record 0 \(records never chain\)"),
                     (28, r"record 3: its destination \(data 28\) is read by record 4"),      # record 3 comes first, and objects first
                     (2, r"record 4: its source \(data 2\) is written by the sorted copy term 1"),
                     (4, r"record 4: its source \(data 4\) is the derived multiplicity of term 2")):
        with pytest.raises(ValueError, match=msg):
            b.derive_links(None, (GROUP_DATA, 8), [(GROUP_DATA, 9), (GROUP_DATA, 10)], [32, 33, 34, 35], 8, write=(GROUP_DATA, col))
    with pytest.raises(ValueError, match=r"record 1: its source \(data 22\) is a destination of record 4"):
        b.derive_links(None, (GROUP_DATA, 8), [(GROUP_DATA, 9)], [22, 33, 34], 8)
    with pytest.raises(ValueError, match=r"record 1: its source \(data 22\) is the derived multiplicity of term 5"):
        b.term(0, [(GROUP_CODE, 1)], sign=-1, mult=(GROUP_DATA, 22), tag=5, derive=True)
    assert len(b.records) == n and len(b.terms) == 5 and b.args().version == 6


def _c_set(hc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))


def _derived(hc):
    cols, n = np.zeros(64, dtype=np.uint32), zhal.C.c_size_t()
    zhal._check(zhal._lib.zkh_circuit_derived_data_columns(hc.h, zhal._ptr(cols), cols.size, zhal.C.byref(n)))
    return [int(x) for x in cols[:n.value]]


def test_c_validator_on_a_gpu_less_circuit_gives_the_same_messages():
    desc, blob = _all()
    hc = zhal.HostCircuit(desc)
    reads = lambda: zhal._lib.zkh_circuit_links_check_reads(hc.h)
    assert reads() == 0
    _c_set(hc, blob)
    assert zhal._lib.zkh_circuit_derives_links(hc.h) == 1 and reads() == 2
    want = [2, 3, 4, 5, 6, 7] + list(range(11, 18)) + [19, 20, 21] + list(range(26, 31))
    assert _derived(hc) == want                                               # the write flags are the host's columns
    for bad in (_edited(blob, [(7, 0)]), _edited(blob, [(1, 7)])):
        with pytest.raises(HalError, match=r"set_arguments: not a ZKA1 \(version 1\) argument blob$"):
            _c_set(hc, bad)
    for edit, msg in BLOB_EDITS + SHAPE_EDITS:
        with pytest.raises(HalError, match="set_arguments: " + msg):
            _c_set(hc, _edited(blob, edit))
    assert _derived(hc) == want and reads() == 2                             # a refused blob leaves the circuit's arguments as they were
    for edit in GOOD_EDITS:
        _c_set(hc, _edited(blob, edit))
    assert reads() == 1
    _, blob5 = _all(reads=False)
    for w, v in ((5, 1), (14, GROUP_DATA), (15, 22)):
        with pytest.raises(HalError, match="set_arguments: record 1: " + RESERVED5):
            _c_set(hc, _edited(blob5, [(_rec(1, w), v)]))
    with pytest.raises(HalError, match=r"set_arguments: not a ZKA1 \(version 1\) argument blob$"):
        _c_set(hc, _edited(blob5, [(1, 6)]))
    _c_set(hc, _edited(blob5, [(7, 9)]))
    assert reads() == 0 and _derived(hc) == want
    _c_set(hc, logup.Arguments.parse(blob).plain().blob())
    assert zhal._lib.zkh_circuit_derives_links(hc.h) == 0 and reads() == 0


# ---- the reference against a walk over the rows ----
def _walk(rec, A, code, data, n):
    """the destinations of one LINK record over the active rows, the slow way: one access after another, the last access to every key
    in a dictionary, and with READS every load compared with what that access left -> {column: A words}"""
    groups = {GROUP_CODE: code.reshape(-1, n), GROUP_DATA: data.reshape(-1, n)}
    x = lambda gc, r: int(groups[gc[0]][gc[1], r]) % P * RINV % P
    out = {c: np.zeros(A, dtype=np.uint32) for c in rec.dsts}
    seen = {}
    for r in range(A):
        if rec.sel is not None and x((GROUP_CODE, rec.sel), r) != 1:
            continue
        key = x(rec.key, r)
        out[rec.last][r] = ONE
        if rec.write is not None:
            assert x(rec.write, r) in (0, 1)
            if x(rec.write, r) == 0:
                for src in rec.carried[1:]:
                    assert x(src, r) == (x(src, seen[key]) if key in seen else 0), (r, src)
        if key in seen:
            q = seen[key]
            out[rec.last][q] = 0
            out[rec.linked][r] = ONE
            for c, src in zip(rec.prevs, rec.carried):
                out[c][r] = groups[src[0]][src[1], q]
            d = x(rec.carried[0], r) - x(rec.carried[0], q) - 1
            assert 0 <= d < 1 << (rec.limb_bits * rec.nl)
            for j, c in enumerate(rec.limbs):
                out[c][r] = (d >> (j * rec.limb_bits)) % (1 << rec.limb_bits) * ONE % P
        seen[key] = r
    return out


def _trace(rng, po2, zk, raw=True):
    """random traces under `_all()`'s records: load / store traces for records 1 (a selector, nc = 2) and 3 (nc = 3, a code value column)
    -> (code, data) as (columns, n) arrays.  raw: about a third of the flags, keys, clocks and values as raw words >= P"""
    n, A = 1 << po2, (1 << po2) - zk
    code, data = rand_fp(rng, SIZES[1], n), rand_fp(rng, SIZES[2], n)
    code[3, :A] = _enc(rng.random(A) < 0.5)                                  # record 1's selector
    data[8, :A] = _enc(rng.integers(0, 7, A))                                # its key ...
    data[23, :A] = _enc(rng.integers(0, 9, A))                               # ... and record 3's
    code[4, :A] = _enc(rng.integers(0, 1 << 31, 9)[rng.integers(0, 9, A)] % P)           # ... and record 2's
    data[9, :A] = _enc(np.cumsum(rng.integers(1, 1 << 12, A)))               # record 1's clock: increasing, differences below 2^24
    same = {}
    for r in range(A):                                                       # records 2 and 3 have no limbs: the clock counts the accesses to the key
        for clock, key in ((18, int(code[4, r])), (24, int(data[23, r]))):
            same[clock, key] = same.get((clock, key), -1) + 1
            data[clock, r] = _enc(same[clock, key])
    code[0, :A], data[22, :A] = _enc(rng.random(A) < 0.5), _enc(rng.random(A) < 0.5)     # the write flags of records 3 and 1
    for sel, key, flag, vals in ((code[3], data[8], data[22], [data[10]]), (None, data[23], code[0], [data[25], code[5]])):
        held = {}
        for r in range(A):
            if sel is not None and sel[r] != ONE:
                continue
            if flag[r] == 0:                                                 # a load
                for v, h in zip(vals, held.get(int(key[r]), [0] * len(vals))):
                    v[r] = h
            held[int(key[r])] = [int(v[r]) for v in vals]
    if raw:
        for col in (code[0], code[4], code[5], data[8], data[9], data[10], data[18], data[22], data[23], data[24], data[25]):
            col[:A][rng.random(A) < 0.3] += np.uint32(P)
    return code, data


@pytest.mark.parametrize("po2,zk,seed", [(6, 3, 1), (8, 40, 2), (10, 300, 3)])
def test_reference_links_equals_a_dictionary_walk(po2, zk, seed):
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    args = logup.Arguments.parse(_all()[1])
    args5 = logup.Arguments.parse(_all(reads=False)[1])
    code, data = _trace(rng, po2, zk)
    code, data = code.reshape(-1), data.reshape(-1)
    got = logup.reference_links(args, po2, zk, code, data).reshape(-1, n)
    want = data.reshape(-1, n).copy()
    for rec in args.records[1:]:
        for c, v in _walk(rec, A, code, data, n).items():
            want[c, :A] = v
    assert np.array_equal(got, want)
    assert np.array_equal(logup.reference_links(args5, po2, zk, code, data).reshape(-1, n), want)       # the rule adds no output
    assert (got[11, :A] == ONE).sum() > A // 4 and (got[26, :A] == ONE).sum() >= A - 9
    loads = (data.reshape(-1, n)[22, :A] % P == 0) & (code.reshape(-1, n)[3, :A] == ONE)
    assert loads.sum() > A // 8 and (loads & (got[11, :A] == 0)).any()        # linked loads, and a load of an address never accessed


def _refuses(args, po2, zk, code, data, msg):
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1))


def test_reference_links_refuses_as_documented():
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    args = logup.Arguments.parse(_all()[1])
    code, data = _trace(np.random.default_rng(4), po2, zk, raw=False)
    dec = lambda v: int(v) % P * RINV % P
    assert not np.array_equal(logup.reference_links(args, po2, zk, code.reshape(-1), data.reshape(-1)), data.reshape(-1))
    on1 = [r for r in range(A) if code[3, r] == ONE]
    chain = [r for r in on1 if data[8, r] == data[8, on1[9]]]                # the accesses of record 1 to one address, in row order
    assert len(chain) >= 5
    first = {}
    for r in range(A):
        first.setdefault(int(data[23, r]), r)
    r3 = max(r for r in first.values() if code[0, r] == 0)                  # record 3: the first access to some address, a load (of zeros)
    # a flag of 2
    bad = data.copy()
    bad[22, chain[2]] = _enc(2)
    _refuses(args, po2, zk, code, bad, f"record 1 at row {chain[2]}: write flag 2, not 0 or 1")
    # a load that differs from the last store: a store, then two loads, the second forged (the first still holds)
    bad = data.copy()
    bad[22, chain[1]], bad[22, chain[2]], bad[22, chain[3]] = ONE, 0, 0
    bad[10, chain[1]] = _enc(777)
    bad[10, chain[2]] = _enc(777) + np.uint32(P)                             # the same residue as a raw word >= P
    bad[10, chain[3]] = _enc(778)
    bad[22, chain[4]] = ONE
    _refuses(args, po2, zk, code, bad, f"record 1 at row {chain[3]}: a load of carried column 1 returns 778, but 777 was last stored (row {chain[2]})")
    # ... and of two bad rows the lower, of two bad records the lower
    bad[10, chain[2]] = _enc(5)
    msg = f"record 1 at row {chain[2]}: a load of carried column 1 returns 5, but 777 was last stored (row {chain[1]})"
    _refuses(args, po2, zk, code, bad, msg)
    c3 = code.copy()
    c3[0, 3] = _enc(7)                                                       # record 3's write flag at a lower row
    _refuses(args, po2, zk, c3, bad, msg)
    _refuses(args, po2, zk, c3, data, "record 3 at row 3: write flag 7, not 0 or 1")
    # a non-zero load of an address never accessed; the second value column (a code column) of nc = 3
    c3 = code.copy()
    c3[0, r3], c3[5, r3] = 0, _enc(9)
    d3 = data.copy()
    d3[25, r3] = np.uint32(P)                                                # the first value column: 0 as the raw word P
    _refuses(args, po2, zk, c3, d3, f"record 3 at row {r3}: a load of carried column 2 returns 9, but its address was never accessed: the value must be 0")
    d3[25, r3] = _enc(4)                                                     # the lowest column is named
    _refuses(args, po2, zk, c3, d3, f"record 3 at row {r3}: a load of carried column 1 returns 4, but its address was never accessed: the value must be 0")
    # an unlinked load whose raw words are P is accepted
    c3[5, r3], d3[25, r3] = np.uint32(P), np.uint32(P)
    logup.reference_links(args, po2, zk, c3.reshape(-1), d3.reshape(-1))
    # a row with a clock and a read violation reports the clock; a flag that is no flag comes before both
    bad = data.copy()
    bad[22, chain[1]], bad[22, chain[2]] = ONE, 0
    bad[10, chain[2]] = (bad[10, chain[1]] % P + ONE) % P
    bad[9, chain[2]] = bad[9, chain[1]]
    t = dec(bad[9, chain[1]])
    _refuses(args, po2, zk, code, bad, f"record 1 at row {chain[2]}: clock not increasing ({t} after {t} at row {chain[1]})")
    bad[22, chain[2]] = _enc(3)
    _refuses(args, po2, zk, code, bad, f"record 1 at row {chain[2]}: write flag 3, not 0 or 1")
    # selectors still come first, over all records
    sel = code.copy()
    sel[3, 200] = _enc(2)
    _refuses(args, po2, zk, sel, bad, "record 1 at row 200: selector 2, not 0 or 1")
    # a store is free, and so is everything under the version-5 blob
    bad = data.copy()
    bad[22, chain[2]], bad[10, chain[2]] = ONE, _enc(123456)
    bad[22, chain[3]] = ONE
    logup.reference_links(args, po2, zk, code.reshape(-1), bad.reshape(-1))
    bad[22, chain[3]] = _enc(2)
    logup.reference_links(logup.Arguments.parse(_all(reads=False)[1]), po2, zk, code.reshape(-1), bad.reshape(-1))


# ---- SYN-LOOKUP-reads against the oracle's row checker ----
def _mix(seed):
    return np.random.default_rng(seed).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)


def test_syn_lookup_reads_shape_and_switches():
    desc, blob = syn_lookup.syn_lookup_tiny_reads()
    a = logup.Arguments.parse(blob)
    assert (int(desc[5]), len(a.terms), a.k, a.version, len(a.records), int(blob[7])) == (22, 15, 5, 6, 1, 1)
    assert syn_lookup.reads_layout(2, 4, 1) == [21] and syn_lookup.reads_layout(2, 4, 3) == [41, 42, 43]
    linked = logup.Arguments.parse(syn_lookup.syn_lookup_tiny_linked()[1])
    assert a.records[0] == replace(linked.records[0], write=(GROUP_DATA, 21)) and a.terms == linked.terms
    assert not np.array_equal(desc, syn_lookup.syn_lookup_tiny_linked()[0])
    fdesc, fblob = syn_lookup.syn_lookup_reads()
    assert int(fdesc[5]) == 92 and logup.Arguments.parse(fblob).version == 6
    d2, b2 = syn_lookup.build_syn_lookup(TINY, link=True, reads=True, derive=True, limbs=True)
    assert np.array_equal(d2, desc) and logup.Arguments.parse(b2).version == 6
    for kw in (dict(), dict(derive=True), dict(sort=True), dict(order=True, sort=True)):
        with pytest.raises(ValueError, match="reads=True is the read rule of the LINK records: it needs link=True"):
            syn_lookup.build_syn_lookup(TINY, reads=True, **kw)
    with pytest.raises(ValueError, match="it needs link=True or link=False"):
        syn_lookup.witness(TINY, 8, 40, reads=True)
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    code, full, _ = syn_lookup.witness(TINY, po2, zk, seed=5, addr_range=64, link=True, reads=True)
    c2, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=5, addr_range=64, link=False, reads=True)
    w, z = full.reshape(-1, n), bare.reshape(-1, n).copy()
    assert np.array_equal(code, c2) and not z[14:21, :A].any() and np.array_equal(z[21], w[21])  # the write flag is the host's column
    z[14:21, :A] = w[14:21, :A]
    assert np.array_equal(w, z)
    store = w[21, :A] == ONE
    assert 0.3 * A < store.sum() < 0.7 * A and set(np.unique(w[21, :A])) == {0, ONE}
    load = ~store
    assert np.array_equal(w[12, :A][load], np.where(w[14, :A][load] == ONE, w[16, :A][load], 0))       # a load returns pval, or 0 unlinked
    assert (load & (w[14, :A] == 0)).any() and (load & (w[14, :A] == ONE) & (w[12, :A] != 0)).any()


@pytest.mark.parametrize("po2,zk,addr_range", [(8, 40, 16), (10, 300, 64), (12, 1994, 5)])
def test_reads_witness_satisfies_the_oracle_and_a_forged_load_fails_on_its_row(oracle, po2, zk, addr_range):
    desc, blob = syn_lookup.build_syn_lookup(TINY, link=True, reads=True, derive=True, limbs=True)
    args = logup.Arguments.parse(blob)
    n, A = 1 << po2, (1 << po2) - zk
    code, data, out = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=addr_range, link=True, reads=True)
    _, zero, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=addr_range, link=False, count=False, limbs=False, reads=True)
    chain = logup.reference_links(args, po2, zk, code, logup.reference_columns(args, po2, zk, code, zero))
    chain = logup.reference_multiplicities(args, po2, zk, code, chain)
    assert np.array_equal(chain, data)                                        # columns -> links -> multiplicities = the host-made witness
    mix = _mix(po2)
    accum, total = logup.reference_accumulate(args, po2, zk, code, data, mix)
    assert total == [0, 0, 0, 0]
    oc = zko.OracleCircuit(oracle, desc)
    assert oc.check_rows(po2, accum, code, data, out, mix) == -1
    ldesc, lblob = syn_lookup.build_syn_lookup(TINY, link=True, derive=True, limbs=True)
    largs = logup.Arguments.parse(lblob)
    lc = zko.OracleCircuit(oracle, ldesc)
    w = data.reshape(-1, n)
    lcols = syn_lookup.link_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0]
    # a forged load: the last access of its address (row = None), and one with a later access whose pval moves with it
    mid = next(r for r in range(A // 3, A) if w[21, r] == 0 and (w[lcols[0], r + 1:A] == w[lcols[0], r]).any())
    for want_row in (None, mid):
        forged, row = syn_lookup.misread_row(TINY, data, po2, zk, row=want_row)
        assert want_row in (None, row) and w[21, row] == 0 and (want_row is not None or w[lcols[4], row] == ONE)
        f = forged.reshape(-1, n).copy()
        assert np.array_equal(np.nonzero((f != w).any(axis=1))[0], [12] if want_row is None else [12, 16])
        f[10, :A] = 0                                                        # the multiplicities counted again: no lookup reads a value
        forged = logup.reference_multiplicities(args, po2, zk, code, f.reshape(-1))
        assert np.array_equal(forged.reshape(-1, n)[10], w[10])
        with pytest.raises(logup.ReferenceError, match=f"record 2 at row {row}: a load of carried column 1 returns"):   # records 0, 1: the words' limbs
            logup.reference_links(args, po2, zk, code, forged)
        accum, total = logup.reference_accumulate(args, po2, zk, code, forged, mix)
        assert total == [0, 0, 0, 0]                                         # the bus still balances
        assert oc.check_rows(po2, accum, code, forged, out, mix) == row      # ... and the first failing row is exactly that row
        # the same forged values under SYN-LOOKUP-linked, which has no read rule, satisfy every constraint: the gap this closes
        same = np.ascontiguousarray(forged.reshape(-1, n)[:21]).reshape(-1)
        laccum, ltotal = logup.reference_accumulate(largs, po2, zk, code, same, mix)
        assert ltotal == [0, 0, 0, 0]
        assert lc.check_rows(po2, laccum, code, same, out, mix) == -1
        assert np.array_equal(logup.reference_links(largs, po2, zk, code, same), same)
    # a write flag that is no flag fails on its row, too
    flag = data.reshape(-1, n).copy()
    flag[21, A // 2] = _enc(2)
    accum, _ = logup.reference_accumulate(args, po2, zk, code, flag.reshape(-1), mix)
    assert oc.check_rows(po2, accum, code, flag.reshape(-1), out, mix) == A // 2
