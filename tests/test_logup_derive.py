"""Derived lookup multiplicities (ZKA1 version 2; zeth_amd/circuits/logup.py, csrc/arguments.hip): the builder and parser of the
version-2 blob, the rules a derived term must follow (in Python and in the C validator, on a GPU-less circuit), SYN-LOOKUP-derived
against the plain circuit, and the host reference of the count.  No GPU."""
import numpy as np
import pytest

from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError

P = 2013265921
TABLE = 8                                   # the table term's index in SYN-LOOKUP-TINY's blob (after 8 limb terms)


def _word(i, w):
    return logup.ARGS_HEADER + logup.TERM_WORDS * i + w


def _builder():
    b = logup.LogupBuilder((12, 4, 8), (4, 8))
    b.term(0, [(GROUP_DATA, 0)], tag=1)                                      # lookups of tag 1
    b.term(0, [(GROUP_DATA, 1), (GROUP_CODE, 2)], tag=2)                     # ... and of tag 2
    return b


def test_builder_round_trips_version_2():
    b = _builder()
    b.term(1, [(GROUP_CODE, 0)], sign=-1, sel=1, mult=(GROUP_DATA, 6), tag=1, derive=True)
    b.term(2, [(GROUP_CODE, 3)], sign=-1, mult=(GROUP_DATA, 7), tag=1, derive=True)       # a second table of the same tag
    b.term(2, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, mult=(GROUP_DATA, 5), tag=2, derive=True)
    blob = b.args().blob()
    assert blob[1] == 2
    assert [int(blob[_word(i, 7)]) for i in range(5)] == [0, 0, 1, 1, 1]
    a = logup.Arguments.parse(blob)
    assert a.version == 2 and [t.derive for t in a.terms] == [False, False, True, True, True]
    assert a.terms[2] == logup.Term(1, ((GROUP_CODE, 0),), -1, 1, (GROUP_DATA, 6), 1, True)
    assert np.array_equal(a.blob(), blob)
    plain = _builder().args()
    assert plain.version == 1 and plain.blob()[1] == 1
    assert np.array_equal(logup.Arguments.parse(plain.blob()).blob(), plain.blob())


@pytest.mark.parametrize("spec,msg", [
    (dict(tuple_cols=[(GROUP_CODE, 0)], sign=1, mult=(GROUP_DATA, 6), tag=1), "needs sign -1"),                       # (a)
    (dict(tuple_cols=[(GROUP_CODE, 0)], sign=-1, mult=(GROUP_CODE, 3), tag=1), "data-group column"),                  # (b)
    (dict(tuple_cols=[(GROUP_CODE, 0)], sign=-1, tag=1), "data-group column"),                                        # (b) no column
    (dict(tuple_cols=[(GROUP_CODE, 0)], sign=-1, mult=(GROUP_DATA, 0), tag=1), "read by the tuple of term 0"),         # (c) a tuple
    (dict(tuple_cols=[(GROUP_DATA, 6)], sign=-1, mult=(GROUP_DATA, 6), tag=1), "read by the tuple of term 2"),         # (c) its own
])
def test_builder_refuses_a_bad_derived_term(spec, msg):
    b = _builder()
    with pytest.raises(ValueError, match=msg):
        b.term(1, derive=True, **spec)
    assert len(b.terms) == 2


def test_builder_refuses_shared_columns_and_negative_lookups():
    b = _builder()
    b.term(1, [(GROUP_DATA, 4)], sign=-1, mult=(GROUP_DATA, 6), tag=1, derive=True)
    with pytest.raises(ValueError, match="also the multiplicity of term 3"):                                            # (c)
        b.term(1, [(GROUP_DATA, 2)], mult=(GROUP_DATA, 6), tag=2)
    with pytest.raises(ValueError, match="read by the tuple of term 3"):                                                # (c)
        b.term(1, [(GROUP_DATA, 6)], tag=2)
    with pytest.raises(ValueError, match="term 3 of its tag 1 has sign -1 and is not derived"):                          # (d)
        b.term(1, [(GROUP_DATA, 3)], sign=-1, tag=1)
    b.term(1, [(GROUP_DATA, 3)], sign=-1, tag=3)                                                                        # another tag: free
    b2 = _builder()
    b2.term(1, [(GROUP_DATA, 3)], sign=-1, tag=1)
    with pytest.raises(ValueError, match="term 2 of its tag 1 has sign -1"):                                            # (d), other order
        b2.term(1, [(GROUP_DATA, 4)], sign=-1, mult=(GROUP_DATA, 6), tag=1, derive=True)


def test_parse_refuses_reserved_bits_and_bad_derived_terms():
    _, blob = syn_lookup.syn_lookup_tiny_derived()
    for w, v, msg in [(7, 2, "word 7 is 2"), (1, 0, "needs sign -1"), (3, GROUP_CODE, "data-group")]:
        bad = blob.copy()
        bad[_word(TABLE, w)] = v
        with pytest.raises(ValueError, match=msg):
            logup.Arguments.parse(bad)
    plain = syn_lookup.syn_lookup_tiny()[1].copy()
    plain[_word(TABLE, 7)] = 7                                              # version 1: word 7 is not read
    assert not any(t.derive for t in logup.Arguments.parse(plain).terms)


def test_plain_blobs_stay_version_1_and_derived_differs_in_two_words():
    for shape in (syn_lookup.TINY, syn_lookup.FULL, syn_lookup.WIDE):
        desc, plain = syn_lookup.build_syn_lookup(shape)
        ddesc, derived = syn_lookup.build_syn_lookup(shape, derive=True)
        assert plain[1] == 1 and not plain[logup.ARGS_HEADER + 7::logup.TERM_WORDS].any()
        table = shape.n_words * shape.n_limbs
        assert list(np.nonzero(plain != derived)[0]) == [1, _word(table, 7)]
        assert derived[1] == 2 and derived[_word(table, 7)] == 1
        assert np.array_equal(desc, ddesc)                                  # the same ZKC1 description: the same control root
    assert np.array_equal(syn_lookup.syn_lookup_derived()[1], syn_lookup.build_syn_lookup(syn_lookup.FULL, derive=True)[1])


def _c_set(hc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))


def test_c_validator_on_a_gpu_less_circuit():
    desc, blob = syn_lookup.syn_lookup_tiny_derived()
    hc = zhal.HostCircuit(desc)                                             # zkh_circuit_load(NULL, ...)
    lib = zhal._lib
    assert not lib.zkh_circuit_derives_multiplicities(hc.h)
    _c_set(hc, blob)
    assert lib.zkh_circuit_derives_multiplicities(hc.h) and lib.zkh_circuit_has_arguments(hc.h)
    words, limbs, m, mem, perm = syn_lookup.layout(syn_lookup.TINY.n_words, syn_lookup.TINY.n_limbs, syn_lookup.TINY.n_mem)
    edits = [
        ([(_word(TABLE, 1), 0)], "term 8: a derived multiplicity needs sign -1"),                                      # (a)
        ([(_word(TABLE, 3), GROUP_CODE), (_word(TABLE, 4), 0)], "term 8: a derived multiplicity must be a data-group"),  # (b)
        ([(_word(0, 9), m)], "term 8: .* read by the tuple of term 0"),                                                 # (c) a tuple
        ([(_word(9, 3), GROUP_DATA), (_word(9, 4), m)], "term 8: .* also the multiplicity of term 9"),                  # (c) a multiplicity
        ([(_word(3, 1), 1)], "term 8: term 3 of its tag 0 has sign -1 and is not derived"),                             # (d)
        ([(_word(TABLE, 7), 2)], "term 8: word 7 is 2"),
        ([(_word(2, 7), 3)], "term 2: word 7 is 3"),
    ]
    for edit, msg in edits:
        bad = blob.copy()
        for w, v in edit:
            bad[w] = v
        with pytest.raises(HalError, match=msg):
            _c_set(hc, bad)
    with pytest.raises(HalError, match="ZKA1"):
        _c_set(hc, blob[:5])
    plain = syn_lookup.syn_lookup_tiny()[1].copy()
    plain[_word(TABLE, 7)] = 0xdead                                         # version 1 leaves word 7 unread
    _c_set(hc, plain)
    assert lib.zkh_circuit_has_arguments(hc.h) and not lib.zkh_circuit_derives_multiplicities(hc.h)


@pytest.mark.parametrize("po2,zk", [(8, 40), (10, 300), (12, 1994)])
def test_reference_equals_the_host_count(po2, zk):
    _, blob = syn_lookup.syn_lookup_tiny_derived()
    args = logup.Arguments.parse(blob)
    code, want, _ = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=po2)
    _, zero, _ = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=po2, count=False)
    assert not np.array_equal(zero, want)
    assert np.array_equal(logup.reference_multiplicities(args, po2, zk, code, zero), want)
    m = syn_lookup.layout(syn_lookup.TINY.n_words, syn_lookup.TINY.n_limbs, syn_lookup.TINY.n_mem)[2]
    n, A = 1 << po2, (1 << po2) - zk
    garbage = zero.reshape(-1, n).copy()
    garbage[m, :A] = np.random.default_rng(po2).integers(0, P, A, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(logup.reference_multiplicities(args, po2, zk, code, garbage.reshape(-1)), want)


def test_reference_follows_the_representative_rule():
    po2, zk = 6, 8
    n, A = 1 << po2, (1 << po2) - zk
    enc = lambda x: (np.asarray(x, dtype=np.uint64) * np.uint64((1 << 32) % P) % np.uint64(P)).astype(np.uint32)
    b = logup.LogupBuilder((8, 2, 4), (4, 8))
    b.term(0, [(GROUP_DATA, 0)])                                            # term 0: lookups
    b.term(0, [(GROUP_CODE, 0)], sign=-1, mult=(GROUP_DATA, 2), derive=True)   # term 1: table 0..3, repeated
    b.term(1, [(GROUP_CODE, 1)], sign=-1, sel=1, mult=(GROUP_DATA, 3), derive=True)   # term 2: another table, selector = its values
    args = b.args()
    code = np.zeros((2, n), np.uint32)
    code[0, :A] = enc(np.arange(A) % 4)
    code[1, :A] = enc(np.arange(A) < 2)                                     # selector / value 1 on rows 0, 1: key 1 at (2, 0), (2, 1)
    data = np.zeros((4, n), np.uint32)
    look = np.array([1, 1, 3, 0, 3, 3, 2] * 8)[:A]
    data[0, :A] = enc(look)
    data[0, 5] = enc(123456)                                                # not in any table ...
    data[1, :A] = enc(np.arange(A) % 3)                                     # (an unrelated column)
    sel_zero = np.ones(A, bool)
    b2 = logup.LogupBuilder((8, 3, 4), (4, 8))
    b2.term(0, [(GROUP_DATA, 0)], sel=2)                                    # ... but its row has weight 0 under this selector
    b2.term(0, [(GROUP_CODE, 0)], sign=-1, mult=(GROUP_DATA, 2), derive=True)
    b2.term(1, [(GROUP_CODE, 1)], sign=-1, sel=1, mult=(GROUP_DATA, 3), derive=True)
    code3 = np.zeros((3, n), np.uint32)
    code3[:2] = code
    sel_zero[5] = False
    code3[2, :A] = enc(sel_zero)
    with pytest.raises(logup.ReferenceError, match="lookup term 0 .tag 0. at row 5 has no table entry: key .123456, 0, 0, 0."):
        logup.reference_multiplicities(args, po2, zk, code.reshape(-1), data.reshape(-1))
    got = logup.reference_multiplicities(b2.args(), po2, zk, code3.reshape(-1), data.reshape(-1)).reshape(-1, n)
    counts = np.bincount(np.delete(look, 5), minlength=4)
    want2 = np.zeros(A, np.uint32)
    want2[:4] = enc(counts)                                                 # term 1 rows 0..3 represent keys 0..3 (term 1 < term 2)
    assert np.array_equal(got[2, :A], want2)
    assert not got[3, :A].any()                                             # term 2's entries of key 1 lose to (1, 1)
    assert np.array_equal(got[:, A:], data[:, A:])


def test_reference_raises_on_a_bad_witness():
    po2, zk = 10, 200
    _, blob = syn_lookup.syn_lookup_tiny_derived()
    args = logup.Arguments.parse(blob)
    code, data, _ = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=7, count=False)
    bad = syn_lookup.corrupt_limb(syn_lookup.TINY, data, po2, row=123, word=1)
    with pytest.raises(logup.ReferenceError, match=r"lookup term 4 \(tag 0\) at row 123 has no table entry"):
        logup.reference_multiplicities(args, po2, zk, code, bad)
    c = code.reshape(-1, 1 << po2).copy()
    c[5, 3] = 2 * ((1 << 32) % P) % P                                       # table selector 2
    with pytest.raises(logup.ReferenceError, match="table term 8 .tag 0. has selector 2 at row 3"):
        logup.reference_multiplicities(args, po2, zk, c.reshape(-1), data)
