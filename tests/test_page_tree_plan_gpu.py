"""zkh_page_tree_plan_device (csrc/page_tree.hip: k_plan_costs, k_plan_scan, k_plan_walk) on the GPU: the plan of P2-TREE over a table
where it lies.  Bare tables uploaded as buffers, no image and no tree; the words of a row behind its address are 0xffffffff and
0xfffffffe, which no kernel may take for an address.  The yardsticks: the host plan in C (hal.page_tree_plan), the greedy loop
p2_tree.parts, and page_tree_cases.node_count for the nodes of a part.

Shapes, the smallest at which the kernels can go wrong: every table of page_tree_cases.CASES (one workgroup, or a few); at (10, 500,
8192) rows 255 and 256, the last lane of one workgroup and the first of the next, in one pair of leaves, in two, and with a part cut
between them, and D = 0, 1, 256, 257; every address of 8192 words, 128 parts over 32 workgroups, more than the first read-back
brings along, and under a cap of 5; every address of 2^17 + 3 words, 513 workgroups, three sums a lane in the scan of the sums; the
refusals by message with the lowest row named across workgroups and across the scan's lanes; one small chain sealed under both plans."""
import ctypes as C
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import page_tree_cases as tc
import page_tree_plan_cases as pc
from args_gpu import image_buf
from zeth_amd import hal as zhal
from zeth_amd.circuits import p2_tree as G
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, verify_page_tree_chain

pytestmark = pytest.mark.gpu
WHO = "page_tree_plan_device"
SENTINEL = 0x5E471E1


def _upload(hal, addrs, at=0, short=0):
    """the table as a buffer: `at` words of filler, then the rows (address, 0xffffffff, 0xfffffffe), the last `short` words left off"""
    rows = np.empty((len(addrs), 3), dtype=np.uint32)
    rows[:, 0], rows[:, 1], rows[:, 2] = np.asarray(addrs, dtype=np.uint32), 0xFFFFFFFF, 0xFFFFFFFE
    words = np.concatenate([np.full(at, 0xDEADBEEF, dtype=np.uint32), rows.reshape(-1)])
    words = words[:words.size - short]
    return hal.copy_from("table", words if words.size else np.zeros(1, dtype=np.uint32))       # no rows: any buffer holds them


def _raw(hal, po2, zk, W, buf, at, D, cap):
    """the C call under a cap, every output behind a sentinel -> (message or None, parts, n_parts, nodes)"""
    parts, n, nodes = (C.c_size_t * (2 * cap + 2))(*[SENTINEL] * (2 * cap + 2)), C.c_size_t(SENTINEL), np.full(cap + 1, SENTINEL, dtype=np.uint32)
    try:
        zhal._check(zhal._lib.zkh_page_tree_plan_device(hal.ctx, po2, zk, W, buf.h, at, D, parts, cap, C.byref(n), zhal._ptr(nodes)))
        msg = None
    except HalError as e:
        msg = str(e)
    return msg, [int(v) for v in parts], n.value, [int(v) for v in nodes]


def _check_plan(hal, s, addrs, at=0):
    """the device plan of `addrs` is the host plan in C and the greedy loop's, its nodes are the ids counted -> the plan"""
    po2, zk, W = s
    want = G.parts(po2, zk, W, addrs)
    plan, nodes = hal.page_tree_plan_device(po2, zk, W, _upload(hal, addrs, at), at, len(addrs), nodes=True)
    assert plan == want and plan == hal.page_tree_plan(po2, zk, W, addrs)
    h = G.tree_height(W)
    assert nodes == [tc.node_count(h, addrs[first:first + count]) for first, count in want] and max(nodes) <= G.block_slots(po2, zk)
    return plan


@pytest.mark.parametrize("s,what", tc.CASES, ids=lambda v: str(v))
def test_the_device_plan_of_every_case(hal, s, what):
    t = tc.table(*s, what)
    assert _check_plan(hal, s, t["addrs"], at=11 if (s, what) == (tc.H12, "random") else 0) == t["plan"]


@pytest.mark.parametrize("name", list(pc.seams()))
def test_the_seams_of_the_costs_pass(hal, name):
    _check_plan(hal, pc.SEAM, pc.seams()[name], at=5 if name == "D = 257" else 0)


def test_many_parts_and_the_cap(hal):
    po2, zk, W = pc.MANY
    addrs = pc.every_address(W)
    want = [(64 * k, 64) for k in range(128)]
    assert _check_plan(hal, pc.MANY, addrs) == want                            # more parts than the first read-back brings along
    buf = _upload(hal, addrs)
    msg, parts, n, nodes = _raw(hal, po2, zk, W, buf, 0, W, 5)
    assert msg is None and n == 128
    assert parts == [v for part in want[:5] for v in part] + [SENTINEL] * 2 and nodes[5] == SENTINEL and all(v <= 16 for v in nodes[:5])
    msg, parts, n, nodes = _raw(hal, po2, zk, W, buf, 0, W, 0)                # a count alone
    assert msg is None and n == 128 and parts == [SENTINEL] * 2 and nodes == [SENTINEL]


def test_past_the_scan_of_the_workgroups_sums(hal):
    po2, zk, W = pc.WIDE
    addrs = pc.every_address(W)
    want = G.parts(po2, zk, W, addrs)
    plan, nodes = hal.page_tree_plan_device(po2, zk, W, _upload(hal, addrs), 0, W, nodes=True)
    assert len(want) == 147 and plan == want
    assert nodes == G.part_nodes(G.tree_height(W), addrs, want) and max(nodes) <= G.block_slots(po2, zk)      # part_nodes: checked on the CPU


def _refused(hal, s, addrs, message, at=0, short=0):
    po2, zk, W = s
    msg, parts, n, nodes = _raw(hal, po2, zk, W, _upload(hal, addrs, at, short), at, len(addrs), 3)
    assert msg == f"{WHO}: {message}"
    assert n == SENTINEL and parts == [SENTINEL] * 8 and nodes == [SENTINEL] * 4           # nothing is written on a refusal


def test_refusals(hal):
    po2, zk, W = pc.SEAM
    follow = lambda r, a, before: f"row {r}: address {a} does not follow a smaller one (row {r - 1}: address {before})"
    outside = lambda r, a, words: f"row {r}: address {a} outside the image of {words} words"
    # two refused rows in different workgroups: the lowest of the whole table is named, whichever lane and workgroup holds the other
    for low, high in ((300, 700), (511, 515), (255, 256), (0, 1023)):
        addrs = np.arange(0, 8 * 1024, 8, dtype=np.int64)
        addrs[high] = W + 5
        addrs[low] = addrs[low - 1] if low else W
        _refused(hal, pc.SEAM, addrs, follow(low, addrs[low], addrs[low - 1]) if low else outside(0, W, W))
    # ... and across the lanes of the scan of the sums (513 workgroups, three a lane)
    wide = pc.every_address(pc.WIDE[2])
    wide[100000] = wide[99999]
    wide[40001] = pc.WIDE[2]
    _refused(hal, pc.WIDE, wide, outside(40001, pc.WIDE[2], pc.WIDE[2]))
    _refused(hal, pc.SEAM, [3, W], outside(1, W, W))                                       # an address at W
    seam = pc.seams()["D = 257"].copy()
    seam[256] = seam[255]                                                                  # two equal addresses across the 255 / 256 seam
    _refused(hal, pc.SEAM, seam, follow(256, seam[255], seam[255]))
    _refused(hal, (po2, zk, 16), [3], "an image of 16 words has a single pair of leaves (W > 16: the root block is not a pair block)")
    _refused(hal, (10, 680, tc.H12[2]), [0], "no room for the h 12 nodes of one path in 11 block slots (po2 10, 680 zk_cycles)")
    _refused(hal, (31, zk, W), [3], f"po2 31 out of range for {zk} zk_cycles")
    good = pc.seams()["D = 257"]
    _refused(hal, pc.SEAM, good, f"a table of 257 rows of 3 words at word 0 does not fit a buffer of {3 * 257 - 1} words", short=1)
    _refused(hal, pc.SEAM, good, f"a table of 257 rows of 3 words at word 4 does not fit a buffer of {4 + 3 * 257 - 1} words", at=4, short=1)
    with pytest.raises(HalError, match=re.escape(f"{WHO}: {follow(256, seam[255], seam[255])}")):      # the wrapper hands the message on
        hal.page_tree_plan_device(po2, zk, W, _upload(hal, seam), 0, 257)
    _check_plan(hal, pc.SEAM, good)                                                        # the good call right after them


def test_a_chain_planned_on_the_device_is_the_chain_planned_on_the_host(hal):
    s, what = tc.H6, "random"
    po2, zk, W = s
    t = tc.table(*s, what)
    prover = SegmentProver(hal, G.p2_tree_circuit(), arguments=G.arguments())
    before, after = hal.image_commit(image_buf(hal, t["image"])), hal.image_commit(image_buf(hal, t["image_after"]))
    words = cases.host_proof(t["image"], t["addrs"], t["outs"], before.to_vec())
    proof = hal.copy_from("proof", words)
    assert len(t["plan"]) > 1
    segs = [Segment(index=p, po2=po2, zk_cycles=zk, noise_seed=tc.NOISE + p) for p in range(len(t["plan"]))]
    host = prover.seal_page_out_tree(segs, proof, words.size, before, after)
    device = prover.seal_page_out_tree(segs, proof, words.size, before, after, plan="device")
    assert len(device) == len(host) == len(segs)
    for a, b in zip(host, device):
        assert a.seal.tobytes() == b.seal.tobytes() and a.control_root.tobytes() == b.control_root.tobytes()
    root = prover.code_root(hal.page_tree_code(prover.circuit, po2, zk), po2)
    got = verify_page_tree_chain(device, root, t["h"], hal.image_root(before))
    assert np.array_equal(got[1], hal.image_root(after))
