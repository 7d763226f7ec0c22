"""zkh_session_prove's refusals that return AFTER the caller's zkh_prove_info has been allocated (csrc/session.hip: one guard frees
it on every exit but the successful one), each taken once through the ABI: the struct comes back all zero, and the session is as
good as new — the next prove on it returns the seals of a fresh session (fixed noise keys)."""
import ctypes as C

import numpy as np
import pytest

from zeth_amd import hal as zhal
from zeth_amd.circuits import syn_air
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu


def refused(sess, segs, match, join_tree=0, host_traces=None):
    """one zkh_session_prove that must fail with `match`, on an info full of rubbish: every byte of it is zero afterwards"""
    lib = zhal.load_library()
    specs, keep = sess._specs(segs, host_traces)
    info = zhal.ProveInfo()
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    with pytest.raises(HalError, match=match):
        zhal._check(lib.zkh_session_prove(sess.h, specs, len(segs), join_tree, 13, None, C.byref(info)))
    assert bytes(info) == bytes(C.sizeof(info))
    lib.zkh_prove_info_free(C.byref(info))           # freeing a zeroed info is a no-op


def seals_of(sess, segs):
    comp, _, _ = sess.prove(segs, verify=True)
    return [r.seal for r in comp.segments]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals_after_info_is_allocated_leave_it_zero_and_the_session_usable(hal, monkeypatch):
    from zeth_amd.circuits import p2_join
    from zeth_amd.host import Session
    monkeypatch.setenv("ZKH_FOLD_LANES", "1")          # no fold-only contexts: nothing is folded here
    desc = syn_air.syn_small()
    segs = [Segment(index=i, po2=12, seed=3100 + i, noise_seed=0x61) for i in range(2)]
    fresh = Session(desc, devices=(0,), lanes_per_device=1)
    want = seals_of(fresh, segs)
    fresh.close()
    sp = SegmentProver(hal, desc)
    traces = []
    for seg in segs:
        code, data, out = sp.witgen(seg)
        traces.append((code.to_vec(), data.to_vec(), out))
    sess = Session(desc, devices=(0,), lanes_per_device=1, join_desc=p2_join.p2_join_circuit())

    # join_tree 1 on a session with assumption receipts
    arec = sp.prove_segment(Segment(index=0, po2=12, seed=3190, noise_seed=0x62))
    sess.set_assumptions(desc, [arec], {12: sp.control_root(12)})
    refused(sess, segs, "has assumption receipts", join_tree=1)
    sess.set_assumptions(desc, [], {})
    assert same(seals_of(sess, segs), want)

    # witness source 1 given a segment with public inputs, and one with host traces
    sess.set_witness_source(1, 1)
    refused(sess, [segs[0], Segment(index=1, po2=12, seed=3101, noise_seed=0x61, pub=(5,))], "witness source 1 takes segments described by their seed only")
    refused(sess, segs, "witness source 1 takes segments described by their seed only", host_traces=[None, traces[1]])
    sess.set_witness_source(0)
    assert same(seals_of(sess, segs), want)

    # join_tree 2 with a segment size the program set has no lift for
    sess.build_recursion([12], join3=False)
    refused(sess, [segs[0], Segment(index=1, po2=13, seed=3101, noise_seed=0x61)], "no lift program for po2-13 segments", join_tree=2)
    assert same(seals_of(sess, segs), want)
    sess.close()


def test_a_chained_session_refuses_host_traces_and_stays_usable(hal):
    from zeth_amd.host import Session
    desc = syn_air.syn_chain_small()
    segs = [Segment(index=i, po2=12, seed=3200 + i, noise_seed=0x63) for i in range(2)]
    fresh = Session(desc, devices=(0,), lanes_per_device=1)
    fresh.set_chained(True, 3)
    want = seals_of(fresh, segs)
    fresh.close()
    sess = Session(desc, devices=(0,), lanes_per_device=1)
    sess.set_chained(True, 3)
    words = np.zeros(8, dtype=np.uint32)               # refused before anything reads them
    refused(sess, segs, "a chained session takes segments described by their seed", host_traces=[None, (words, words, words)])
    assert same(seals_of(sess, segs), want)
    sess.close()
