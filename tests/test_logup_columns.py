"""Derived-column records (ZKA1 version 4; zeth_amd/circuits/logup.py, csrc/columns.hip, csrc/arguments.hip's validator): the builder
and parser of the version-4 blob, the blobs of versions 1..3 word for word what they were, the rules a record must follow (in the
builder, the parser and the C validator on a GPU-less circuit, with equal messages), the host reference of the derivation with its
refusals, and SYN-LOOKUP-ordered against the oracle's row checker: the honest witness holds, two swapped sorted rows fail on their
row although the bus still balances.  No GPU."""
import hashlib
import re

import numpy as np
import pytest

import zko
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_ACCUM, GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError

P = 2013265921
ONE = (1 << 32) % P
TINY = syn_lookup.TINY
N_TERMS = 14                                # SYN-LOOKUP-ordered TINY: 8 limbs, the table (8, m = data 10), the memory tuple (9: data
#                                             11..13), its copy (10: data 14..16), the 3 order limbs (11..13: data 18..20; flag: data 17)


def _enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def _term(i, w):
    return logup.ARGS_HEADER + logup.TERM_WORDS * i + w


def _rec(i, w, n_terms=N_TERMS):
    return logup.ARGS_HEADER + logup.TERM_WORDS * n_terms + logup.RECORD_WORDS * i + w


def _ordered(**kw):
    return syn_lookup.build_syn_lookup(TINY, order=True, **kw)


def _all():
    """SYN-LOOKUP-ordered TINY with everything derived: records 0, 1 = the words' LIMBS, record 2 = the ORDER of the copy's (addr, time)"""
    return _ordered(derive=True, sort=True, limbs=True)


def _builder():
    b = logup.LogupBuilder((8, 4, 16), (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1)                                          # term 0
    b.term(0, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, tag=1, sorted_from=0, sort_keys=(0, 1))  # term 1: sorted columns 2, 3
    b.term(1, [(GROUP_CODE, 1)], sign=-1, mult=(GROUP_DATA, 4), tag=0, derive=True)               # term 2: derived multiplicity 4
    return b


def test_builder_round_trips_version_4():
    b = _builder()
    r0 = b.derive_limbs((GROUP_CODE, 2), [5, 6, 7], 5)
    r1 = b.derive_order([(GROUP_DATA, 2), (GROUP_DATA, 3)], [8, 9, 10], 12)                       # reads the sorted columns
    r2 = b.derive_order([(GROUP_DATA, 0)], [11], 16)
    b.term(1, [(GROUP_DATA, 9)], tag=0)                                                           # a lookup reads a destination
    assert (r0.kind, r0.nl, r0.n_src) == (logup.KIND_LIMBS, 3, 1) and (r1.kind, r1.nl, r1.n_src) == (logup.KIND_ORDER, 2, 2) and r2.nl == 1
    a = b.args()
    blob = a.blob()
    assert blob[1] == 4 and blob[6] == 3 and blob[7] == 0 and blob.size == logup.ARGS_HEADER + 16 * 4 + 16 * 3
    assert list(blob[_rec(0, 0, 4):_rec(1, 0, 4)]) == [1, 5, 3, 1, GROUP_CODE, 2, 0, 0, 5, 6, 7, 0, 0, 0, 0, 0]
    assert list(blob[_rec(1, 0, 4):_rec(2, 0, 4)]) == [2, 12, 2, 2, GROUP_DATA, 2, GROUP_DATA, 3, 8, 9, 10, 0, 0, 0, 0, 0]
    assert list(blob[_rec(2, 0, 4):]) == [2, 16, 1, 1, GROUP_DATA, 0, 0, 0, 11, 0, 0, 0, 0, 0, 0, 0]
    back = logup.Arguments.parse(blob)
    assert back.version == 4 and back.records == [r0, r1, r2] and back.terms == a.terms
    assert np.array_equal(back.blob(), blob)
    assert int(blob[_term(1, 7)]) == 0x422                                    # term word 7 is read as in version 3
    plain = back.plain()
    assert plain.version == 1 and not plain.records and plain.blob()[6] == 0 and np.array_equal(plain.blob()[8:], blob[8:8 + 64] * (np.arange(64) % 16 != 7))
    short = blob[:-1]
    with pytest.raises(ValueError, match="119 words for 4 terms and 3 records"):
        logup.Arguments.parse(short)


# the blobs and descriptions of every circuit that existed before version 4, by the default arguments: (blob, description) digests
RECORDED = {
    "tiny_00": ("4d53ba1cd485fcbe", "0654c55c0910907a"), "tiny_01": ("b0edc4f04cd0c1c1", "0654c55c0910907a"),
    "tiny_10": ("7458bf0359af39e4", "0654c55c0910907a"), "tiny_11": ("02f530acb4c77398", "0654c55c0910907a"),
    "full_00": ("e4e9efc09cb220c4", "134283b8996203b4"), "full_01": ("47657902228d4d17", "134283b8996203b4"),
    "full_10": ("c9101c8b5f43ac43", "134283b8996203b4"), "full_11": ("37b14791777f4f89", "134283b8996203b4"),
    "multi_00": ("7cd3e67714cc7c47", "2814d41fb8caeca1"), "multi_01": ("14039b4f33013ff2", "2814d41fb8caeca1"),
    "multi_10": ("adae8f0aecb4946c", "2814d41fb8caeca1"), "multi_11": ("1502333547e10b24", "2814d41fb8caeca1"),
    "wide_00": ("af17e93d6f0bef93", "a572280d129a4a82"), "wide_01": ("26de62d1ea915eba", "a572280d129a4a82"),
    "wide_10": ("3d7baef46dea21c0", "a572280d129a4a82"), "wide_11": ("2287472e5f74f471", "a572280d129a4a82"),
}
_digest = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()[:16]


def test_versions_1_to_3_are_unchanged_and_limbs_add_only_records():
    got = {}
    for name, shape in (("tiny", TINY), ("full", syn_lookup.FULL), ("multi", syn_lookup.MULTI), ("wide", syn_lookup.WIDE)):
        for d in (0, 1):
            for s in (0, 1):
                desc, blob = syn_lookup.build_syn_lookup(shape, derive=bool(d), sort=bool(s))
                got[f"{name}_{d}{s}"] = (_digest(blob), _digest(desc))
                assert blob[1] == max(1, 2 * d, 3 * s) and blob[6] == 0
                assert np.array_equal(logup.Arguments.parse(blob).blob(), blob)
                ldesc, lblob = syn_lookup.build_syn_lookup(shape, derive=bool(d), sort=bool(s), limbs=True)
                assert np.array_equal(ldesc, desc)                          # the same description: the same control root
                assert lblob[1] == 4 and lblob[6] == shape.n_words and np.array_equal(lblob[2:6], blob[2:6])
                assert np.array_equal(lblob[8:blob.size], blob[8:]) and lblob.size == blob.size + 16 * shape.n_words
    assert got == RECORDED
    code, data, _ = syn_lookup.witness(TINY, 10, 300, seed=5)                # the default witness, too
    assert (_digest(code), _digest(data)) == ("05d3073fd18abae7", "aa887d9a3cfaa021")


def test_syn_lookup_ordered_shape_and_witness_switches():
    desc, blob = _ordered()
    a = logup.Arguments.parse(blob)
    assert (int(desc[5]), len(a.terms), a.k, a.version, len(a.records)) == (21, 14, 5, 4, 1)
    assert not np.array_equal(desc, syn_lookup.syn_lookup_tiny()[0])
    assert syn_lookup.layout(2, 4, 1) == ([0, 1], [[2, 3, 4, 5], [6, 7, 8, 9]], 10, [[11, 12, 13]], [[14, 15, 16]])
    assert syn_lookup.order_layout(2, 4, 1) == [[17, 18, 19, 20]]
    assert a.records[0] == logup.Record(logup.KIND_ORDER, 4, 3, ((GROUP_DATA, 14), (GROUP_DATA, 16)), (17, 18, 19, 20))
    assert [t.tuple_cols for t in a.terms[11:]] == [((GROUP_DATA, c),) for c in (18, 19, 20)] and all(t.tag == 0 and t.sign == 1 for t in a.terms[11:])
    assert max(logup.column_degree(ts) for ts in a.by_column()) <= 5
    d4, b4 = _all()
    assert np.array_equal(d4, desc) and len(logup.Arguments.parse(b4).records) == 3
    assert np.array_equal(logup.Arguments.parse(b4).plain().blob(), a.plain().blob())
    mdesc, mblob = syn_lookup.build_syn_lookup(syn_lookup.MULTI, order=True, sort=True)
    assert int(mdesc[5]) == 29 + 12 and len(logup.Arguments.parse(mblob).records) == 3
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    code, full, out = syn_lookup.witness(TINY, po2, zk, seed=5, addr_range=1 << 12, order=True)
    for off, cols in (("limbs", list(range(2, 10))), ("order", [17, 18, 19, 20]), ("sort", [14, 15, 16]), ("count", [10])):
        kw = dict(order=True)
        kw[off] = False
        c2, d2, o2 = syn_lookup.witness(TINY, po2, zk, seed=5, addr_range=1 << 12, **kw)
        w, z = full.reshape(-1, n), d2.reshape(-1, n).copy()
        assert np.array_equal(code, c2) and not z[cols, :A].any() and w[cols, :A].any()
        z[cols, :A] = w[cols, :A]
        assert np.array_equal(w, z)                                         # every other word, the blinding rows included


# (edits of the blob of `_all()`, the message of the parser and of the C validator), in the order of the rules
BLOB_EDITS = [
    ([(_rec(0, 0), 3)], r"record 0: kind 3 \(1 = LIMBS, 2 = ORDER\)"),
    ([(_rec(1, 0), 0)], "record 1: kind 0"),
    ([(_rec(0, 1), 17)], r"record 0: 4 limbs of 17 bits \(1..8 limbs of 1..16 bits, at most 32 bits in all\)"),
    ([(_rec(0, 1), 0)], "record 0: 4 limbs of 0 bits"),
    ([(_rec(0, 1), 9)], "record 0: 4 limbs of 9 bits"),                                          # 36 bits
    ([(_rec(0, 2), 0)], "record 0: 0 limbs of 4 bits"),
    ([(_rec(0, 2), 9)], "record 0: 9 limbs of 4 bits"),
    ([(_rec(0, 3), 2)], r"record 0: 2 sources \(LIMBS: 1; ORDER: 1 or 2\)"),
    ([(_rec(0, 3), 0)], "record 0: 0 sources"),
    ([(_rec(2, 3), 3)], "record 2: 3 sources"),
    ([(_rec(2, 2), 8)], "record 2: an ORDER record with two keys has at most 7 limbs"),
    ([(_rec(0, 6), 1)], "record 0: a reserved word is not 0"),                                   # the unused source pair
    ([(_rec(0, 7), 1)], "record 0: a reserved word is not 0"),
    ([(_rec(0, 12), 5)], "record 0: a reserved word is not 0"),                                  # an unused destination word
    ([(_rec(2, 15), 1)], "record 2: a reserved word is not 0"),
    ([(_rec(2, 3), 1)], "record 2: a reserved word is not 0"),                                   # one key: its second pair and 4th destination
    ([(_rec(0, 4), GROUP_ACCUM)], r"record 0: source \(0, 0\) is not a code or data column"),
    ([(_rec(1, 4), 3)], r"record 1: source \(3, 1\) is not a code or data column"),
    ([(_rec(0, 9), 2)], r"record 0: its destination \(data 2\) appears twice"),
    ([(_rec(1, 5), 2)], r"record 1: its source \(data 2\) is a destination of record 0 \(records never chain\)"),
    ([(_rec(0, 5), 3)], r"record 0: its source \(data 3\) is a destination of record 0"),        # its own
    ([(_rec(1, 5), 19)], r"record 1: its source \(data 19\) is a destination of record 2"),
    ([(_rec(1, 5), 10)], r"record 1: its source \(data 10\) is the derived multiplicity of term 8"),
    ([(_rec(1, 8), 2)], r"record 0: its destination \(data 2\) is also written by record 1"),
    ([(_rec(1, 8), 14)], r"record 1: its destination \(data 14\) is written by the sorted copy term 10"),
    ([(_rec(1, 8), 10)], r"record 1: its destination \(data 10\) is the derived multiplicity of term 8"),
    ([(_rec(1, 8), 11)], r"record 1: its destination \(data 11\) is read by term 9, the source of a sorted copy \(the sort runs first\)"),
    ([(_term(0, 3), GROUP_DATA), (_term(0, 4), 6)], r"record 1: its destination \(data 6\) is the multiplicity of term 0"),
]
# ... and what only a validator that knows the circuit can refuse (the builder and the C validator)
SHAPE_EDITS = [
    ([(_rec(0, 5), 21)], r"record 0: source \(2, 21\) is not a code or data column"),
    ([(_rec(0, 4), GROUP_CODE), (_rec(0, 5), 7)], r"record 0: source \(1, 7\) is not a code or data column"),
    ([(_rec(1, 11), 21)], "record 1: destination 21 is not a data column"),
]
# ... and what the rules allow
GOOD_EDITS = [
    [(_rec(0, 4), GROUP_CODE), (_rec(0, 5), 6)],                                                 # a code source
    [(_rec(1, 5), 15)],                                                                          # a source that a sorted copy writes
    [(_rec(1, 5), 0)],                                                                           # two records read one source
    [(_rec(2, 3), 1), (_rec(2, 6), 0), (_rec(2, 7), 0), (_rec(2, 11), 0), (_term(13, 9), 17)],    # ORDER by one key, 3 limbs in 17..19
]


def _edited(blob, edit):
    bad = blob.copy()
    for w, v in edit:
        bad[w] = v
    return bad


def test_parser_refuses_every_rule():
    _, blob = _all()
    assert blob.size == _rec(3, 0) and blob[6] == 3
    for edit, msg in BLOB_EDITS:
        with pytest.raises(ValueError, match="ZKA1: " + msg):
            logup.Arguments.parse(_edited(blob, edit))
    for edit in GOOD_EDITS:
        a = logup.Arguments.parse(_edited(blob, edit))
        assert np.array_equal(a.blob(), _edited(blob, edit))
    for edit, msg in SHAPE_EDITS:                                           # with the circuit's widths the same function refuses these
        a = logup.Arguments.parse(_edited(blob, edit))
        assert logup.check_columns(a.terms, a.records) is None
        assert re.search(msg, logup.check_columns(a.terms, a.records, (20, 7, 21)))


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
    lib = zhal._lib
    assert not lib.zkh_circuit_derives_columns(hc.h) and _derived(hc) == []
    _c_set(hc, blob)
    assert lib.zkh_circuit_derives_columns(hc.h) and lib.zkh_circuit_derives_sorted(hc.h) and lib.zkh_circuit_derives_multiplicities(hc.h)
    assert _derived(hc) == list(range(2, 11)) + list(range(14, 21))
    for edit, msg in BLOB_EDITS + SHAPE_EDITS:
        with pytest.raises(HalError, match="set_arguments: " + msg):
            _c_set(hc, _edited(blob, edit))
    assert lib.zkh_circuit_derives_columns(hc.h)                             # a refused blob leaves the arguments as they were
    for edit in GOOD_EDITS:
        _c_set(hc, _edited(blob, edit))
    with pytest.raises(HalError, match="279 words for 14 terms and 3 records"):
        _c_set(hc, blob[:-1])
    # the rules of the terms come first, as in the parser
    both = _edited(blob, [(_term(10, 1), 0), (_rec(0, 0), 3)])
    with pytest.raises(HalError, match="term 10: a sorted copy needs sign -1"):
        _c_set(hc, both)
    with pytest.raises(ValueError, match="term 10: a sorted copy needs sign -1"):
        logup.Arguments.parse(both)
    # versions 1..3 carry no records: header word 6 is not read, and nothing is derived column-wise
    for other in (_ordered()[1], ):
        plain = logup.Arguments.parse(other).plain().blob()
        _c_set(hc, plain)
        assert not lib.zkh_circuit_derives_columns(hc.h) and _derived(hc) == []
    v3 = logup.Arguments(5, 0, 4, logup.Arguments.parse(blob).terms).blob()
    assert v3[1] == 3
    _c_set(hc, v3)
    assert not lib.zkh_circuit_derives_columns(hc.h) and _derived(hc) == [10, 14, 15, 16]
    _c_set(hc, _ordered()[1])                                                # the ORDER record alone
    assert _derived(hc) == [17, 18, 19, 20]
    few = np.zeros(2, dtype=np.uint32)
    n = zhal.C.c_size_t()
    with pytest.raises(HalError, match="derived_data_columns: 4 columns, room for 2"):
        zhal._check(lib.zkh_circuit_derived_data_columns(hc.h, zhal._ptr(few), 2, zhal.C.byref(n)))
    assert n.value == 4


BAD_RECORDS = [
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [5, 6], 17), "record 0: 2 limbs of 17 bits"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [], 4), "record 0: 0 limbs of 4 bits"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [5, 6, 7], 11), "record 0: 3 limbs of 11 bits"),
    (lambda b: b.derive_order([], [5], 4), "record 0: 0 sources"),
    (lambda b: b.derive_order([(GROUP_DATA, 0)] * 3, [5, 6], 4), "record 0: 3 sources"),
    (lambda b: b.derive_order([(GROUP_DATA, 2), (GROUP_DATA, 3)], list(range(5, 14)), 4), "record 0: an ORDER record with two keys has at most 7 limbs"),
    (lambda b: b.derive_limbs((GROUP_ACCUM, 0), [5], 4), r"record 0: source \(0, 0\) is not a code or data column"),
    (lambda b: b.derive_limbs((GROUP_CODE, 4), [5], 4), r"record 0: source \(1, 4\) is not a code or data column"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [16], 4), "record 0: destination 16 is not a data column"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [5, 5], 4), r"record 0: its destination \(data 5\) appears twice"),
    (lambda b: b.derive_limbs((GROUP_DATA, 5), [5, 6], 4), r"record 0: its source \(data 5\) is a destination of record 0"),
    (lambda b: b.derive_limbs((GROUP_DATA, 4), [5], 4), r"record 0: its source \(data 4\) is the derived multiplicity of term 2"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [2], 4), r"record 0: its destination \(data 2\) is written by the sorted copy term 1"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [4], 4), r"record 0: its destination \(data 4\) is the derived multiplicity of term 2"),
    (lambda b: b.derive_limbs((GROUP_DATA, 0), [1], 4), r"record 0: its destination \(data 1\) is read by term 0, the source of a sorted copy"),
]


@pytest.mark.parametrize("make,msg", BAD_RECORDS)
def test_builder_refuses_a_bad_record(make, msg):
    b = _builder()
    with pytest.raises(ValueError, match=msg):
        make(b)
    assert not b.records and b.args().version == 3


def test_builder_refuses_what_later_records_and_terms_break():
    b = _builder()
    b.derive_limbs((GROUP_DATA, 2), [5, 6], 4)                                # a sorted column as the source: allowed
    with pytest.raises(ValueError, match=r"record 1: its source \(data 6\) is a destination of record 0 \(records never chain\)"):
        b.derive_limbs((GROUP_DATA, 6), [7], 4)
    with pytest.raises(ValueError, match=r"record 0: its destination \(data 5\) is also written by record 1"):
        b.derive_limbs((GROUP_DATA, 0), [5], 4)
    with pytest.raises(ValueError, match=r"record 1: its source \(data 5\) is a destination of record 0"):
        b.derive_order([(GROUP_DATA, 5)], [7], 4)
    assert len(b.records) == 1
    with pytest.raises(ValueError, match=r"record 0: its destination \(data 5\) is the multiplicity of term 3"):
        b.term(1, [(GROUP_DATA, 8)], tag=0, mult=(GROUP_DATA, 5))
    with pytest.raises(ValueError, match=r"record 0: its destination \(data 5\) is the derived multiplicity of term 3"):
        b.term(1, [(GROUP_CODE, 1)], sign=-1, tag=2, mult=(GROUP_DATA, 5), derive=True)
    b.term(1, [(GROUP_DATA, 8)], tag=3)                                       # term 3
    with pytest.raises(ValueError, match=r"record 0: its destination \(data 6\) is written by the sorted copy term 4"):
        b.term(1, [(GROUP_DATA, 6)], sign=-1, tag=3, sorted_from=3, sort_keys=(0,))
    b.term(0, [(GROUP_DATA, 5)], tag=5)                                       # term 4, a lookup of a destination: the point
    with pytest.raises(ValueError, match=r"record 0: its destination \(data 5\) is read by term 4, the source of a sorted copy"):
        b.term(1, [(GROUP_DATA, 9)], sign=-1, tag=5, sorted_from=4, sort_keys=(0,))
    assert len(b.terms) == 5 and len(b.records) == 1
    with pytest.raises(ValueError, match=r"order_constraints: 2 limbs of 15 bits exceed 29 bits"):
        b.order_constraints(b.true(), b.derive_order([(GROUP_DATA, 0)], [10, 11], 15))
    with pytest.raises(ValueError, match="not an ORDER record"):
        b.order_constraints(b.true(), b.records[0])


# ---- the host reference ----
def _case(po2=6, zk=9):
    """LIMBS of a code and of a data column, ORDER by two keys and by one, over hand-made columns; -> (args, code, data)"""
    n, A = 1 << po2, (1 << po2) - zk
    rng = np.random.default_rng(7)
    b = logup.LogupBuilder((4, 2, 16), (4, 8))
    b.term(0, [(GROUP_DATA, 15)], tag=0)
    b.derive_limbs((GROUP_CODE, 1), [3, 4, 5], 4)                             # record 0: 12 bits
    b.derive_limbs((GROUP_DATA, 0), [6, 7], 16)                               # record 1: 32 bits, anything fits
    b.derive_order([(GROUP_DATA, 1), (GROUP_DATA, 2)], [8, 9, 10], 3)         # record 2: 6 bits
    b.derive_order([(GROUP_DATA, 1)], [11, 12], 2)                            # record 3: 4 bits
    code = rng.integers(0, P, (2, n), dtype=np.uint64).astype(np.uint32)
    data = rng.integers(0, P, (16, n), dtype=np.uint64).astype(np.uint32)
    code[1, :A] = _enc(rng.integers(0, 1 << 12, A))
    k0 = (np.arange(A) // 4) * 3                                              # runs of four equal first keys, steps of 3 between them
    k1 = (np.arange(A) % 4) * 5 + 1                                           # ... inside which the second key rises by 5
    data[1, :A], data[2, :A] = _enc(k0), _enc(k1)
    big = rng.random(A) < 0.3                                                 # the same residues as raw words >= P
    data[1, :A][big] += np.uint32(P)
    return b.args(), po2, zk, code, data, k0, k1


def test_reference_columns():
    args, po2, zk, code, data, k0, k1 = _case()
    n, A = 1 << po2, (1 << po2) - zk
    before = data.copy()
    got = logup.reference_columns(args, po2, zk, code.reshape(-1), data.reshape(-1)).reshape(-1, n)
    assert np.array_equal(data, before)                                       # a copy
    dec = lambda rows: logup._dec(rows).astype(np.int64)
    v = dec(code[1, :A])
    assert all(np.array_equal(dec(got[3 + j, :A]), (v >> (4 * j)) & 15) for j in range(3))
    v = dec(data[0, :A])
    assert np.array_equal(dec(got[6, :A]) + (dec(got[7, :A]) << 16), v)
    e = np.concatenate([[0], (k0[1:] == k0[:-1]).astype(np.int64)])
    d = np.concatenate([[0], np.where(e[1:] == 1, k1[1:] - k1[:-1], k0[1:] - k0[:-1] - 1)])
    assert e[5:8].all() and not e[8] and np.array_equal(dec(got[8, :A]), e)
    assert np.array_equal(dec(got[9, :A]) + 8 * dec(got[10, :A]), d)
    assert np.array_equal(dec(got[11, :A]) + 4 * dec(got[12, :A]), np.concatenate([[0], np.diff(k0)]))
    untouched = [0, 1, 2, 13, 14, 15]
    assert np.array_equal(got[untouched], data[untouched]) and np.array_equal(got[:, A:], data[:, A:])
    assert (got[3:13, :A] < P).all()


def test_reference_refusals_name_the_lowest_record_and_row():
    args, po2, zk, code, data, k0, k1 = _case()
    n, A = 1 << po2, (1 << po2) - zk
    ref = lambda c, d: logup.reference_columns(args, po2, zk, c.reshape(-1), d.reshape(-1))
    bad = code.copy()
    bad[1, 30] = _enc(1 << 12)
    bad[1, 17] = _enc(P - 1)
    with pytest.raises(logup.ReferenceError, match=r"record 0 at row 17: the value 2013265920 does not fit 3 limbs of 4 bits"):
        ref(bad, data)
    d2 = data.copy()
    d2[1, 19], d2[1, 20] = data[1, 20], data[1, 19]                           # first keys 12, 15 swapped: row 20 steps back
    with pytest.raises(logup.ReferenceError, match=r"record 2 at row 20: not ordered \(difference -4\)"):
        ref(code, d2)
    with pytest.raises(logup.ReferenceError, match=r"record 0 at row 17"):  # the lower record wins, whatever the row
        ref(bad, d2)
    d3 = data.copy()
    d3[2, 7] = _enc(int(k1[6]) - 1)                                           # the second key steps back inside a run of equal first keys
    with pytest.raises(logup.ReferenceError, match=r"record 2 at row 7: not ordered \(difference -1\)"):
        ref(code, d3)
    d4 = data.copy()
    d4[1, 40:A] = _enc(k0[40:] + 100)                                         # a jump of the first key: 6 bits do not hold it
    with pytest.raises(logup.ReferenceError, match=r"record 2 at row 40: the difference 102 does not fit 2 limbs of 3 bits"):
        ref(code, d4)
    d5 = data.copy()
    d5[1, A:] = _enc(0)                                                       # the blinding rows are not looked at
    assert np.array_equal(ref(code, d5).reshape(-1, n)[3:13, :A], ref(code, data).reshape(-1, n)[3:13, :A])


# ---- SYN-LOOKUP-ordered against the oracle's row checker ----
def _mix(seed):
    return np.random.default_rng(seed).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("po2,zk,addr_range", [(8, 40, 16), (10, 300, 1 << 12), (12, 1994, 5)])
def test_ordered_witness_satisfies_the_oracle_and_a_swap_fails_on_its_row(oracle, po2, zk, addr_range):
    desc, blob = _all()
    args = logup.Arguments.parse(blob)
    n, A = 1 << po2, (1 << po2) - zk
    code, data, out = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=addr_range, order=True)
    _, zero, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=addr_range, order=False, sort=False, count=False, limbs=False)
    chain = logup.reference_sorted(args, po2, zk, code, zero)
    chain = logup.reference_multiplicities(args, po2, zk, code, logup.reference_columns(args, po2, zk, code, chain))
    assert np.array_equal(chain, data)                                        # sorted -> columns -> multiplicities = the host-made witness
    mix = _mix(po2)
    accum, total = logup.reference_accumulate(args, po2, zk, code, data, mix)
    assert total == [0, 0, 0, 0]
    oc = zko.OracleCircuit(oracle, desc)
    assert oc.check_rows(po2, accum, code, data, out, mix) == -1
    row = A // 2
    swapped = syn_lookup.swap_sorted_rows(TINY, data, po2, row)
    assert not np.array_equal(swapped, data)
    accum, total = logup.reference_accumulate(args, po2, zk, code, swapped, mix)
    assert total == [0, 0, 0, 0]                                              # still a permutation: the bus balances
    assert oc.check_rows(po2, accum, code, swapped, out, mix) == row          # ... and only the order constraints object
    with pytest.raises(logup.ReferenceError, match=r"record 2 at row %d: not ordered" % (row + 1)):
        logup.reference_columns(args, po2, zk, code, swapped)
