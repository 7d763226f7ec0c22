"""Derived sorted copies (ZKA1 version 3; zeth_amd/circuits/logup.py, csrc/sort.hip, csrc/arguments.hip's validator): the builder and
parser of the version-3 blob, the rules a sorted copy must follow (in the builder, the parser and the C validator on a GPU-less
circuit), SYN-LOOKUP-sorted against the plain circuit, and the host reference of the sort.  No GPU."""
import numpy as np
import pytest

from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError

P = 2013265921
ONE = (1 << 32) % P
TINY = syn_lookup.TINY
MEM, PERM = 9, 10                           # SYN-LOOKUP-TINY's blob: 8 limb terms, the table (8), the memory tuple and its copy


def _word(i, w):
    return logup.ARGS_HEADER + logup.TERM_WORDS * i + w


def _enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def _flags(src, keys, derive=0):
    f = derive | 2 | len(keys) << 4 | src << 16
    for j, pos in enumerate(keys):
        f |= pos << (8 + 2 * j)
    return f


def _builder():
    b = logup.LogupBuilder((12, 4, 12), (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1), (GROUP_CODE, 2)], tag=1, sel=3)      # term 0: a source
    b.term(0, [(GROUP_DATA, 2)], tag=2)                                               # term 1: another source
    return b


def test_builder_round_trips_version_3():
    b = _builder()
    b.term(1, [(GROUP_DATA, 4), (GROUP_DATA, 5), (GROUP_DATA, 6)], sign=-1, tag=1, sel=3, sorted_from=0, sort_keys=(2, 0))
    b.term(1, [(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,))
    b.term(2, [(GROUP_DATA, 8)], tag=3)
    b.term(2, [(GROUP_CODE, 0)], sign=-1, mult=(GROUP_DATA, 9), tag=3, derive=True)   # a derived multiplicity in another tag
    blob = b.args().blob()
    assert blob[1] == 3
    assert [int(blob[_word(i, 7)]) for i in range(6)] == [0, 0, _flags(0, (2, 0)), _flags(1, (0,)), 0, 1]
    assert _flags(0, (2, 0)) == 0x222 and _flags(1, (0,)) == 0x10012
    a = logup.Arguments.parse(blob)
    assert a.version == 3
    assert [(t.sorted_from, t.sort_keys, t.derive) for t in a.terms] == [(None, (), False)] * 2 + [(0, (2, 0), False), (1, (0,), False),
                                                                                                 (None, (), False), (None, (), True)]
    assert np.array_equal(a.blob(), blob)
    assert logup.Term(0, ((GROUP_DATA, 0),)).sorted_from is None and logup.Term(0, ((GROUP_DATA, 0),)).sort_keys == ()
    plain = _builder().args()
    assert plain.version == 1 and plain.blob()[1] == 1


def test_source_indices_follow_the_column_order_of_the_blob():
    b = logup.LogupBuilder((12, 4, 12), (4, 8))
    b.term(2, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1)                              # builder term 0 -> blob term 2
    b.term(0, [(GROUP_DATA, 4), (GROUP_DATA, 5)], sign=-1, tag=1, sorted_from=0, sort_keys=(1,))   # builder 1 -> blob 0
    b.term(1, [(GROUP_DATA, 2)], tag=2)
    a = logup.Arguments.parse(b.args().blob())
    assert [t.col for t in a.terms] == [0, 1, 2]
    assert a.terms[0].sorted_from == 2 and a.terms[0].sort_keys == (1,)
    assert np.array_equal(a.blob(), b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))[1])


BAD_COPIES = [
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=1, tag=2, sorted_from=1, sort_keys=(0,)), "term 2: a sorted copy needs sign -1"),                   # (a)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,), derive=True, mult=(GROUP_DATA, 9)),
     "term 2: a sorted copy cannot also have a derived multiplicity"),                                                                       # (a)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=2, sort_keys=(0,)), "term 2: its source term 2 is not another term"),        # (a)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=5, sort_keys=(0,)), "term 2: its source term 5 is not another term"),        # (a)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=3, sorted_from=1, sort_keys=(0,)), "term 2: its source term 1 has another tag"),            # (b)
    (dict(tuple_cols=[(GROUP_DATA, 7), (GROUP_DATA, 8)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,)), "another tag, tuple width"),         # (b)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, sel=3, sorted_from=1, sort_keys=(0,)), "tuple width or selector"),                   # (b)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, mult=(GROUP_DATA, 9), sorted_from=1, sort_keys=(0,)), "constant multiplicity 1"),      # (b)
    (dict(tuple_cols=[(GROUP_CODE, 1)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,)), r"tuple column \(1, 1\) of a sorted copy must be a data"),   # (c)
    (dict(tuple_cols=[(GROUP_DATA, 2)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,)), r"sorted column \(data 2\) is read by the tuple of term 1"),  # (c)
    (dict(tuple_cols=[(GROUP_DATA, 1)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,)), r"sorted column \(data 1\) is read by the tuple of term 0"),  # (c)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=1, sort_keys=(1,)), "key positions must be distinct and below the tuple width 1"),  # (d)
    (dict(tuple_cols=[(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=1, sort_keys=()), "term 2: 0 sort keys"),                                   # (d)
    (dict(tuple_cols=[(GROUP_DATA, 4), (GROUP_DATA, 5), (GROUP_DATA, 6)], sign=-1, tag=1, sel=3, sorted_from=0, sort_keys=(0, 0)),
     "key positions must be distinct"),                                                                                                      # (d)
    (dict(tuple_cols=[(GROUP_DATA, 4), (GROUP_DATA, 5), (GROUP_DATA, 4)], sign=-1, tag=1, sel=3, sorted_from=0, sort_keys=(0,)),
     r"sorted column \(data 4\) appears twice"),                                                                                             # (c)
]


@pytest.mark.parametrize("spec,msg", BAD_COPIES)
def test_builder_refuses_a_bad_sorted_copy(spec, msg):
    b = _builder()
    with pytest.raises(ValueError, match=msg):
        b.term(1, **spec)
    assert len(b.terms) == 2


def test_builder_refuses_what_later_terms_break():
    b = _builder()
    b.term(1, [(GROUP_DATA, 7)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,))
    with pytest.raises(ValueError, match="term 2: its source term 1 is also the source of term 3"):                       # (a)
        b.term(1, [(GROUP_DATA, 8)], sign=-1, tag=2, sorted_from=1, sort_keys=(0,))
    with pytest.raises(ValueError, match="term 3: its source term 2 needs sign"):                                         # (a)
        b.term(1, [(GROUP_DATA, 8)], sign=-1, tag=2, sorted_from=2, sort_keys=(0,))
    with pytest.raises(ValueError, match=r"term 2: its sorted column \(data 7\) is read by the tuple of term 3"):         # (c)
        b.term(1, [(GROUP_DATA, 7)], tag=5)
    with pytest.raises(ValueError, match=r"term 2: its sorted column \(data 7\) is the multiplicity of term 3"):          # (c)
        b.term(1, [(GROUP_DATA, 8)], tag=5, mult=(GROUP_DATA, 7))
    with pytest.raises(ValueError, match="term 2: term 3 of its tag 2 has a derived multiplicity"):                       # (e)
        b.term(1, [(GROUP_CODE, 0)], sign=-1, mult=(GROUP_DATA, 9), tag=2, derive=True)
    b.term(1, [(GROUP_CODE, 0)], sign=-1, mult=(GROUP_DATA, 9), tag=4, derive=True)                                       # another tag: free
    b.term(2, [(GROUP_DATA, 10)], tag=4)
    with pytest.raises(ValueError, match="term 5: its source term 3 needs sign"):                                         # (a) a table
        b.term(2, [(GROUP_DATA, 11)], sign=-1, tag=4, sorted_from=3, sort_keys=(0,))
    with pytest.raises(ValueError, match="sort_keys belong to a sorted copy"):
        b.term(2, [(GROUP_DATA, 11)], sign=-1, tag=4, sort_keys=(0,))
    assert len(b.terms) == 5
    b4 = logup.LogupBuilder((12, 4, 12), (4, 8))
    b4.term(0, [(GROUP_DATA, c) for c in range(4)], tag=1)
    with pytest.raises(ValueError, match=r"term 1: 4 sort keys \(1..3"):                                                  # four keys: refused
        b4.term(0, [(GROUP_DATA, 4 + c) for c in range(4)], sign=-1, tag=1, sorted_from=0, sort_keys=(0, 1, 2, 3))


# (edits of SYN-LOOKUP-TINY-sorted's blob, the message of the parser and of the C validator)
BLOB_EDITS = [
    ([(_word(PERM, 1), 0)], "term 10: a sorted copy needs sign -1"),                                                       # (a)
    ([(_word(PERM, 7), _flags(MEM, (0, 2), derive=1))], "term 10: a sorted copy cannot also have a derived multiplicity"),  # (a)
    ([(_word(PERM, 7), _flags(PERM, (0, 2)))], "term 10: its source term 10 is not another term"),                          # (a)
    ([(_word(PERM, 7), _flags(11, (0, 2)))], "term 10: its source term 11 is not another term"),                            # (a)
    ([(_word(MEM, 1), 1)], "term 10: its source term 9 needs sign"),                                                        # (a)
    ([(_word(PERM, 7), _flags(8, (0,)))], "term 10: its source term 8 needs sign"),                                         # (a) the table, -1
    ([(_word(MEM, 7), 1)], "term 10: its source term 9 is itself derived or a sorted copy"),                                # (a) a flag
    ([(_word(MEM, 5), 2)], "term 10: its source term 9 has another tag, tuple width or selector"),                          # (b)
    ([(_word(MEM, 2), 0)], "term 10: its source term 9 has another tag, tuple width or selector"),                          # (b)
    ([(_word(MEM, 3), GROUP_CODE), (_word(MEM, 4), 3)], "term 10: a sorted copy and its source term 9 have the constant"),   # (b)
    ([(_word(PERM, 8), GROUP_CODE), (_word(PERM, 9), 3)], r"term 10: tuple column \(1, 3\) of a sorted copy must be a data"),  # (c)
    ([(_word(PERM, 11), 14)], r"term 10: its sorted column \(data 14\) appears twice"),                                     # (c)
    ([(_word(0, 9), 15)], r"term 10: its sorted column \(data 15\) is read by the tuple of term 0"),                        # (c)
    ([(_word(3, 3), GROUP_DATA), (_word(3, 4), 16)], r"term 10: its sorted column \(data 16\) is the multiplicity of term 3"),  # (c)
    ([(_word(PERM, 7), _flags(MEM, (0, 0)))], "term 10: its sort key positions must be distinct and below the tuple width 3"),  # (d)
    ([(_word(PERM, 7), _flags(MEM, (0, 3)))], "term 10: its sort key positions must be distinct and below the tuple width 3"),  # (d)
    ([(_word(PERM, 7), _flags(MEM, ()))], "term 10: 0 sort keys"),                                                          # (d)
    ([(_word(PERM, 7), _flags(MEM, (0, 2)) | 4)], "term 10: word 7 is 0x90826"),                                            # reserved bits
    ([(_word(PERM, 7), _flags(MEM, (0, 2)) | 0x80)], "term 10: word 7 is 0x908a2"),
    ([(_word(PERM, 7), _flags(MEM, (0, 2)) | 0x3000)], "term 10: word 7 is 0x93822"),                                       # an unused key position
    ([(_word(2, 7), 0x10)], "term 2: word 7 is 0x10"),                                                                      # fields without bit 1
    ([(_word(2, 7), 0x90000)], "term 2: word 7 is 0x90000"),
]


def test_parse_refuses_bad_sorted_copies_and_reserved_bits():
    _, blob = syn_lookup.syn_lookup_tiny_sorted()
    assert int(blob[_word(PERM, 7)]) == _flags(MEM, (0, 2)) == 0x90822
    for edit, msg in BLOB_EDITS:
        bad = blob.copy()
        for w, v in edit:
            bad[w] = v
        with pytest.raises(ValueError, match=msg):
            logup.Arguments.parse(bad)
    _, both = syn_lookup.build_syn_lookup(TINY, derive=True, sort=True)
    bad = both.copy()
    bad[_word(8, 5)] = 1                                                    # the derived table moves into the copies' tag
    with pytest.raises(ValueError, match="term 10: term 8 of its tag 1 has a derived multiplicity"):                        # (e)
        logup.Arguments.parse(bad)
    v2 = syn_lookup.syn_lookup_tiny_derived()[1].copy()
    v2[_word(PERM, 7)] = 2                                                  # version 2 knows no bit 1
    with pytest.raises(ValueError, match="word 7 is 2"):
        logup.Arguments.parse(v2)


def _c_set(hc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    zhal._check(zhal._lib.zkh_circuit_set_arguments(hc.h, zhal._ptr(b), b.size))


def test_c_validator_on_a_gpu_less_circuit():
    desc, blob = syn_lookup.syn_lookup_tiny_sorted()
    hc = zhal.HostCircuit(desc)
    lib = zhal._lib
    assert not lib.zkh_circuit_derives_sorted(hc.h)
    _c_set(hc, blob)
    assert lib.zkh_circuit_derives_sorted(hc.h) and lib.zkh_circuit_has_arguments(hc.h) and not lib.zkh_circuit_derives_multiplicities(hc.h)
    for edit, msg in BLOB_EDITS:
        bad = blob.copy()
        for w, v in edit:
            bad[w] = v
        with pytest.raises(HalError, match=msg):
            _c_set(hc, bad)
    _, both = syn_lookup.build_syn_lookup(TINY, derive=True, sort=True)
    _c_set(hc, both)
    assert lib.zkh_circuit_derives_sorted(hc.h) and lib.zkh_circuit_derives_multiplicities(hc.h)
    bad = both.copy()
    bad[_word(8, 5)] = 1
    with pytest.raises(HalError, match="term 10: term 8 of its tag 1 has a derived multiplicity"):                          # (e)
        _c_set(hc, bad)
    four = logup.LogupBuilder((4, 4, 12), (4, 8))
    four.term(0, [(GROUP_DATA, c) for c in range(4)], tag=1)
    four.term(0, [(GROUP_DATA, 4 + c) for c in range(4)], sign=-1, tag=1, sorted_from=0, sort_keys=(0, 1, 2))
    fb = four.args().blob()
    fb[_word(1, 7)] = _flags(0, (0, 1, 2, 3))
    hc4 = zhal.HostCircuit(four.finish(four.arguments(four.true(), four.get(GROUP_CODE, 0), four.get(GROUP_CODE, 1), four.get(GROUP_CODE, 2))))
    with pytest.raises(HalError, match=r"term 1: 4 sort keys \(1..3"):
        _c_set(hc4, fb)
    with pytest.raises(ValueError, match=r"term 1: 4 sort keys \(1..3"):
        logup.Arguments.parse(fb)
    v2 = syn_lookup.syn_lookup_tiny_derived()[1].copy()
    _c_set(hc, v2)
    assert not lib.zkh_circuit_derives_sorted(hc.h) and lib.zkh_circuit_derives_multiplicities(hc.h)
    v2[_word(PERM, 7)] = 2                                                  # version 2 still refuses word 7 = 2
    with pytest.raises(HalError, match="term 10: word 7 is 2"):
        _c_set(hc, v2)
    plain = syn_lookup.syn_lookup_tiny()[1].copy()
    plain[_word(PERM, 7)] = 0x90822                                         # version 1 leaves word 7 unread
    _c_set(hc, plain)
    assert lib.zkh_circuit_has_arguments(hc.h) and not lib.zkh_circuit_derives_sorted(hc.h)


def test_plain_and_derived_blobs_are_unchanged_and_sorted_differs_in_word_1_and_the_copies():
    for shape in (TINY, syn_lookup.FULL, syn_lookup.WIDE, syn_lookup.MULTI):
        desc, plain = syn_lookup.build_syn_lookup(shape)
        ddesc, derived = syn_lookup.build_syn_lookup(shape, derive=True)
        sdesc, srt = syn_lookup.build_syn_lookup(shape, sort=True)
        bdesc, both = syn_lookup.build_syn_lookup(shape, derive=True, sort=True)
        for d in (ddesc, sdesc, bdesc):
            assert np.array_equal(desc, d)                                  # the same ZKC1 description: the same control root
        table = shape.n_words * shape.n_limbs
        copies = [_word(table + 2 + 2 * i, 7) for i in range(shape.n_mem)]
        assert plain[1] == 1 and not plain[logup.ARGS_HEADER + 7::logup.TERM_WORDS].any()
        assert derived[1] == 2 and list(np.nonzero(plain != derived)[0]) == [1, _word(table, 7)] and derived[_word(table, 7)] == 1
        assert srt[1] == 3 and list(np.nonzero(plain != srt)[0]) == [1] + copies
        assert [int(srt[w]) for w in copies] == [_flags(table + 1 + 2 * i, (0, 2)) for i in range(shape.n_mem)]
        assert both[1] == 3 and list(np.nonzero(srt != both)[0]) == [_word(table, 7)] and both[_word(table, 7)] == 1
    assert np.array_equal(syn_lookup.syn_lookup_sorted()[1], syn_lookup.build_syn_lookup(syn_lookup.FULL, sort=True)[1])
    assert np.array_equal(syn_lookup.syn_lookup_tiny_sorted()[1], syn_lookup.build_syn_lookup(TINY, sort=True)[1])


def test_plain_and_version_2_blobs_are_the_recorded_words():
    """the blobs of the circuits that existed before version 3, pinned by digest: nothing of them moved"""
    import hashlib
    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()[:16]
    got = {name: digest(f()[1]) for name, f in (("tiny", syn_lookup.syn_lookup_tiny), ("full", syn_lookup.syn_lookup),
                                                 ("tiny_derived", syn_lookup.syn_lookup_tiny_derived), ("derived", syn_lookup.syn_lookup_derived))}
    assert got == RECORDED_BLOBS


RECORDED_BLOBS = {"tiny": "4d53ba1cd485fcbe", "full": "e4e9efc09cb220c4", "tiny_derived": "7458bf0359af39e4", "derived": "c9101c8b5f43ac43"}


def test_sort_false_changes_only_the_permuted_columns():
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    for shape in (TINY, syn_lookup.MULTI):
        perm = [c for cols in syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)[4] for c in cols]
        code, want, out = syn_lookup.witness(shape, po2, zk, seed=5)
        code2, zero, out2 = syn_lookup.witness(shape, po2, zk, seed=5, sort=False)
        assert np.array_equal(code, code2) and np.array_equal(out, out2)
        w, z = want.reshape(-1, n), zero.reshape(-1, n)
        assert not z[perm, :A].any() and w[perm, :A].any()
        z[perm, :A] = w[perm, :A]
        assert np.array_equal(w, z)                                         # every other word, the blinding rows included


@pytest.mark.parametrize("shape,po2,zk", [(TINY, 8, 40), (TINY, 10, 300), (TINY, 12, 1994), (syn_lookup.MULTI, 12, 1994)])
def test_reference_equals_the_host_sort(shape, po2, zk):
    args = logup.Arguments.parse(syn_lookup.build_syn_lookup(shape, sort=True)[1])
    code, want, _ = syn_lookup.witness(shape, po2, zk, seed=po2)
    _, zero, _ = syn_lookup.witness(shape, po2, zk, seed=po2, sort=False)
    assert not np.array_equal(zero, want)
    assert np.array_equal(logup.reference_sorted(args, po2, zk, code, zero), want)
    n, A = 1 << po2, (1 << po2) - zk
    garbage = zero.reshape(-1, n).copy()
    for cols in syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)[4]:
        garbage[cols, :A] = np.random.default_rng(po2).integers(0, P, (len(cols), A), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(logup.reference_sorted(args, po2, zk, code, garbage.reshape(-1)), want)
    assert np.array_equal(zero, syn_lookup.witness(shape, po2, zk, seed=po2, sort=False)[1])       # the input is not written


def test_reference_is_stable_on_equal_keys():
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    for shape in (TINY, syn_lookup.MULTI):
        args = logup.Arguments.parse(syn_lookup.build_syn_lookup(shape, sort=True, sort_keys=(0,))[1])
        code, want, _ = syn_lookup.witness_equal_keys(shape, po2, zk, seed=9)
        _, zero, _ = syn_lookup.witness_equal_keys(shape, po2, zk, seed=9, sort=False)
        got = logup.reference_sorted(args, po2, zk, code, zero)
        assert np.array_equal(got, want)
        _w, _l, _m, mem, perm = syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)
        g = got.reshape(-1, n)
        for i in range(shape.n_mem):
            addr, time = logup._dec(g[perm[i][0], :A]), logup._dec(g[perm[i][2], :A])
            assert len(np.unique(addr)) <= 5 and (np.diff(addr.astype(np.int64)) >= 0).all()
            src_time = logup._dec(g[mem[i][2], :A])
            where = np.empty(A, np.int64)
            where[src_time.astype(np.int64)] = np.arange(A)                  # times are a permutation: the source row of every copy row
            rows = where[time.astype(np.int64)]
            same = addr[1:] == addr[:-1]
            assert (np.diff(rows)[same] > 0).all()                           # equal keys keep the source order
            assert not (np.diff(time.astype(np.int64))[same] > 0).all()      # ... which the time order would not give


def _selector_case(sel_values):
    """one pair under a code selector, keys (v1, v0); -> (args, po2, zk, code, data)"""
    po2, zk = 6, 8
    n, A = 1 << po2, (1 << po2) - zk
    b = logup.LogupBuilder((4, 2, 5), (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_CODE, 1)], tag=7, sel=0)
    b.term(0, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, tag=7, sel=0, sorted_from=0, sort_keys=(1, 0))
    rng = np.random.default_rng(3)
    code = np.zeros((2, n), np.uint32)
    data = rng.integers(0, P, (5, n), dtype=np.uint64).astype(np.uint32)
    code[0, :A] = _enc(sel_values[:A])
    code[0, A:] = _enc(5)                                                   # blinding rows are not looked at
    code[1, :A] = _enc(rng.integers(0, 3, A))
    data[0, :A] = _enc(rng.integers(0, 4, A))
    return b.args(), po2, zk, code, data


def test_reference_with_a_selector_and_its_refusal():
    sel = (np.arange(64) % 3 != 1).astype(np.uint64)
    args, po2, zk, code, data = _selector_case(sel)
    n, A = 1 << po2, (1 << po2) - zk
    got = logup.reference_sorted(args, po2, zk, code.reshape(-1), data.reshape(-1)).reshape(-1, n)
    on = np.nonzero(sel[:A] == 1)[0]
    k1, k0 = logup._dec(code[1, on]), logup._dec(data[0, on])
    order = sorted(range(len(on)), key=lambda j: (int(k1[j]), int(k0[j]), j))
    assert np.array_equal(got[2, on], data[0, on[order]]) and np.array_equal(got[3, on], code[1, on[order]])
    off = np.nonzero(sel[:A] == 0)[0]
    assert not got[2, off].any() and not got[3, off].any()
    assert np.array_equal(got[:, A:], data[:, A:]) and np.array_equal(got[[0, 1, 4]], data[[0, 1, 4]])
    sel[17] = 2
    args, po2, zk, code, data = _selector_case(sel)
    with pytest.raises(logup.ReferenceError, match=r"sorted-copy term 1 \(tag 7\) has selector 2 at row 17, not 0 or 1"):
        logup.reference_sorted(args, po2, zk, code.reshape(-1), data.reshape(-1))


def test_accumulate_balances_on_the_derived_data_and_not_on_an_altered_row():
    po2, zk = 10, 300
    n = 1 << po2
    for shape, keys, wit in ((TINY, (0, 2), syn_lookup.witness), (syn_lookup.MULTI, (0,), syn_lookup.witness_equal_keys)):
        args = logup.Arguments.parse(syn_lookup.build_syn_lookup(shape, sort=True, sort_keys=keys)[1])
        code, zero, _ = wit(shape, po2, zk, seed=4, sort=False)
        mix = np.random.default_rng(1).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
        with pytest.raises(logup.ReferenceError, match="does not balance"):
            logup.reference_accumulate(args, po2, zk, code, zero, mix)
        data = logup.reference_sorted(args, po2, zk, code, zero)
        _, total = logup.reference_accumulate(args, po2, zk, code, data, mix)
        assert total == [0, 0, 0, 0]
        perm = syn_lookup.layout(shape.n_words, shape.n_limbs, shape.n_mem)[4]
        bad = data.reshape(-1, n).copy()
        bad[perm[-1][1], 77] = (int(bad[perm[-1][1], 77]) + ONE) % P            # one value of one sorted row
        with pytest.raises(logup.ReferenceError, match="does not balance"):
            logup.reference_accumulate(args, po2, zk, code, bad.reshape(-1), mix)
