"""Lookup and permutation arguments as data (zeth_amd/circuits/logup.py, SYN-LOOKUP): the builder, the ZKA1 blob, the host reference of
the accumulate against the oracle's own constraint check, and the bound verifier on SYN-LOOKUP's generated kernels.  No GPU."""
import os
import sys

import numpy as np
import pytest

import zko
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA, Circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2013265921


def _mix(seed):
    return np.random.default_rng(seed).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)


def test_builder_refuses_degree_above_five():
    b = logup.LogupBuilder((8, 4, 6), (4, 8))
    for _ in range(3):
        b.term(0, [(GROUP_DATA, 0)])                                        # 3 plain terms: degree 1 + (1 + 3) = 5
    with pytest.raises(ValueError, match="degree 6 exceeds 5"):
        b.term(0, [(GROUP_DATA, 1)])                                        # a fourth: 6
    assert len([t for t in b.terms if t.col == 0]) == 3                     # the refused term is not kept
    for _ in range(3):                                                      # selector x multiplicity: 1 + (2 + 3 - 1) = 5
        b.term(1, [(GROUP_DATA, 0)], sel=1, mult=(GROUP_DATA, 2))
    with pytest.raises(ValueError, match="degree 6"):
        b.term(1, [(GROUP_DATA, 1)], sel=1, mult=(GROUP_DATA, 3))
    assert logup.column_degree([logup.Term(0, ((GROUP_DATA, 0),), sel=1, mult=(GROUP_CODE, 2))] * 3) == 5
    with pytest.raises(ValueError, match="tuple width"):
        b.term(0, [(GROUP_DATA, i) for i in range(5)])
    with pytest.raises(ValueError, match="mix offset"):
        logup.LogupBuilder((8, 4, 6), (4, 6), alpha=0, beta=4)


def test_zka1_round_trip():
    b = logup.LogupBuilder((12, 5, 9), (4, 12), alpha=4, beta=8)
    b.term(2, [(GROUP_DATA, 1), (GROUP_CODE, 4), (GROUP_DATA, 8), (GROUP_DATA, 0)], sign=-1, sel=3, mult=(GROUP_DATA, 7), tag=9)
    b.term(0, [(GROUP_CODE, 0)], mult=(GROUP_CODE, 1), tag=1)
    b.term(1, [(GROUP_DATA, 2)])
    blob = b.args().blob()
    assert blob[0] == 0x5A4B4131 and blob[1] == 1 and blob[2] == 3 and blob[3] == 4 and blob[4] == 8 and blob[5] == 3
    assert blob.size == logup.ARGS_HEADER + 3 * logup.TERM_WORDS
    a = logup.Arguments.parse(blob)
    assert [t.col for t in a.terms] == [0, 1, 2]                            # sorted by column
    assert a.terms[2] == logup.Term(2, ((GROUP_DATA, 1), (GROUP_CODE, 4), (GROUP_DATA, 8), (GROUP_DATA, 0)), -1, 3, (GROUP_DATA, 7), 9)
    assert np.array_equal(a.blob(), blob)
    for shape in (syn_lookup.TINY, syn_lookup.FULL):
        desc, blob = syn_lookup.build_syn_lookup(shape)
        a = logup.Arguments.parse(blob)
        assert np.array_equal(a.blob(), blob)
        c = Circuit.parse(desc)
        assert c.group_sizes[0] == 4 * a.k and c.kind == 0 and c.global_sizes == (4, 8)
        assert len(a.terms) == shape.n_words * shape.n_limbs + 1 + 2 * shape.n_mem
    bad = blob.copy()
    bad[0] ^= 1
    with pytest.raises(ValueError):
        logup.Arguments.parse(bad)


def test_syn_lookup_full_shape():
    desc, blob = syn_lookup.syn_lookup()
    a = logup.Arguments.parse(blob)
    assert (a.k, len(a.terms), int(desc[5])) == (23, 67, 87)
    assert max(logup.column_degree(ts) for ts in a.by_column()) == 5


@pytest.mark.parametrize("po2,zk", [(8, 40), (10, 300), (12, 1994)])
def test_reference_accumulate_satisfies_the_oracle(oracle, po2, zk):
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    code, data, out = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=po2)
    mix = _mix(po2)
    noise = lambda col: np.full(zk, col + 1, dtype=np.uint32)             # any words: the blinding rows are not constrained
    accum, total = logup.reference_accumulate(args, po2, zk, code, data, mix, noise=noise)
    assert total == [0, 0, 0, 0]
    oc = zko.OracleCircuit(oracle, desc)
    assert oc.check_rows(po2, accum, code, data, out, mix) == -1
    # a different accum (one cell moved) is caught on its row
    bad = accum.copy()
    bad[(1 << po2) * 5 + 7] ^= 1
    assert oc.check_rows(po2, bad, code, data, out, mix) == 7


def test_corrupted_limb_unbalances_the_bus(oracle):
    po2, zk = 10, 200
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    code, data, out = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=7)
    mix = _mix(11)
    bad = syn_lookup.corrupt_limb(syn_lookup.TINY, data, po2, row=123, word=1)   # limb out of the table, word still = sum of limbs
    with pytest.raises(logup.ReferenceError, match="does not balance"):
        logup.reference_accumulate(args, po2, zk, code, bad, mix)
    accum, total = logup.reference_accumulate(args, po2, zk, code, bad, mix, check_balance=False)
    assert any(total)
    A = (1 << po2) - zk
    assert zko.OracleCircuit(oracle, desc).check_rows(po2, accum, code, bad, out, mix) == A - 1    # only the bus constraint objects


def test_reference_refuses_a_vanishing_denominator():
    po2, zk = 8, 40
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    code, data, out = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=3)
    mix = _mix(5).copy()
    mix[4:8] = [int((1 << 32) % P), 0, 0, 0]                                # beta = 1, alpha = the limb's own value on row 0
    d = data.reshape(-1, 1 << po2)
    mix[0:4] = [d[2, 0], 0, 0, 0]                                           # limb column 2 (word 0, limb 0) is term 0 of column 0
    with pytest.raises(logup.ReferenceError, match="row 0, accum column 0, term 0"):
        logup.reference_accumulate(args, po2, zk, code, data, mix)


def test_bound_verifier_accepts_syn_lookup_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_bounds
    for name, fn in (("syn_lookup_tiny", syn_lookup.syn_lookup_tiny), ("syn_lookup", syn_lookup.syn_lookup)):
        desc, _ = fn()
        violations, stats = check_bounds.check_desc(name, desc)
        assert violations == [], violations[:3]
        assert stats["kernels"] >= 1
