"""The plan of P2-TREE as a prefix sum and a search (p2_tree.parts_by_scan, part_nodes: the numpy twins of zkh_page_tree_plan_device;
DESIGN.md "THE PLAN AS A SCAN"), on the CPU.  The yardsticks use nothing of the formulation: the greedy loop p2_tree.parts for the
plan, and page_tree_cases.node_count, which counts a part's dirty nodes from the set of their ids.  Over every table of
page_tree_cases.CASES, seeded random tables (random sets and dense runs, as the formulation was first checked) and the tables on the
device kernels' seams; then the same ValueErrors, and what of the new entry point can be checked without a GPU: the symbol, the
header, the binding, the wrapper's own refusals and seal_page_out_tree's."""
import os
import re
import subprocess

import numpy as np
import pytest

import page_tree_cases as tc
import page_tree_plan_cases as pc
from zeth_amd import hal as zhal
from zeth_amd.circuits import p2_tree as G
from zeth_amd.hal import HalError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _agree(po2, zk, W, addrs):
    """parts_by_scan is parts, and part_nodes counts the ids of every part -> the plan"""
    want = G.parts(po2, zk, W, addrs)
    assert G.parts_by_scan(po2, zk, W, addrs) == want
    h, B = G.tree_height(W), G.block_slots(po2, zk)
    nodes = G.part_nodes(h, addrs, want)
    assert nodes == [tc.node_count(h, addrs[first:first + count]) for first, count in want]
    assert max(nodes) <= B
    return want


@pytest.mark.parametrize("s,what", tc.CASES, ids=lambda v: str(v))
def test_the_scan_plans_every_case_as_the_greedy_loop(s, what):
    t = tc.table(*s, what)
    assert _agree(*s, t["addrs"]) == t["plan"]


def test_the_scan_plans_random_tables_as_the_greedy_loop():
    rng = np.random.default_rng(2623)
    several = 0
    for k in range(300):
        W = int(rng.integers(17, 1 << 15))
        h = G.tree_height(W)
        po2 = int(rng.integers(max(8, (31 * h).bit_length()), 13))
        zk = int(rng.integers(0, (1 << po2) - 31 * h + 1))                     # B >= h
        D = int(rng.integers(0, min(W, 3000 if k % 8 == 0 else 400) + 1))
        if k % 2:                                                              # dense runs: neighbours share pairs of leaves
            start = int(rng.integers(0, W - D + 1))
            addrs = np.arange(start, start + D, dtype=np.int64)
        else:
            addrs = np.sort(rng.choice(W, D, replace=False)).astype(np.int64)
        several += len(_agree(po2, zk, W, addrs)) > 1
    assert several > 100                                                       # the cut is what is under test


@pytest.mark.parametrize("name", list(pc.seams()))
def test_the_scan_plans_the_seam_tables(name):
    addrs = pc.seams()[name]
    plan = _agree(*pc.SEAM, addrs)
    if name == "rows 255 and 256 in one pair":
        assert addrs[255] >> 4 == addrs[256] >> 4 and not any(first == 256 for first, _ in plan)
    if name == "rows 255 and 256 in different pairs":
        assert addrs[255] >> 4 != addrs[256] >> 4
    if name == "a part boundary at row 256":
        assert (256, 64) in plan


def test_the_scan_plans_the_long_tables():
    assert _agree(*pc.MANY, pc.every_address(pc.MANY[2])) == [(64 * k, 64) for k in range(128)]
    assert len(G.parts_by_scan(*pc.WIDE, pc.every_address(pc.WIDE[2]))) == len(G.parts(*pc.WIDE, pc.every_address(pc.WIDE[2]))) == 147


@pytest.mark.parametrize("shape,addrs", [((10, 500, 16), [3]), ((10, 680, tc.H12[2]), [0]), ((10, 500, 1 << 31), [0])])
def test_the_same_value_errors_as_parts(shape, addrs):
    with pytest.raises(ValueError) as want:
        G.parts(*shape, addrs)
    with pytest.raises(ValueError) as got:
        G.parts_by_scan(*shape, addrs)
    assert str(got.value) == str(want.value)


def test_the_library_the_header_and_the_binding_have_the_entry_point():
    name = "zkh_page_tree_plan_device"
    exported = subprocess.run(["nm", "-D", "--defined-only", zhal.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(rf" T {name}$", exported, flags=re.M)
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "zkhal.h")).read(), flags=re.S)
    decl = re.search(rf"const char\* {name}\(([^;]*)\);", header)
    assert decl and len(decl.group(1).split(",")) == 11
    res, args = zhal.ABI[name]
    assert len(args) == 11 and getattr(zhal.load_library(), name).argtypes == args


def test_what_is_refused_without_a_gpu():
    lib = zhal.load_library()
    parts, n = (zhal.C.c_size_t * 2)(), zhal.C.c_size_t(77)
    with pytest.raises(HalError, match=r"^page_tree_plan_device: null argument$"):      # no context, no table: nothing is touched
        zhal._check(lib.zkh_page_tree_plan_device(None, 10, 500, 64, None, 0, 0, parts, 1, zhal.C.byref(n), None))
    assert n.value == 77
    hal = object.__new__(zhal.HipHal)                                          # the wrapper's own refusals come before it needs a context
    with pytest.raises(HalError, match="page_tree_plan_device: the table is a ndarray, not a device Buffer"):
        zhal.HipHal.page_tree_plan_device(hal, 10, 500, 64, np.zeros(3, dtype=np.uint32), 0, 1)
    table = object.__new__(zhal.Buffer)
    with pytest.raises(HalError, match=r"page_tree_plan_device: negative argument \(po2 10, zk_cycles 500, image_words 64, table_at -1, D 1\)"):
        zhal.HipHal.page_tree_plan_device(hal, 10, 500, 64, table, -1, 1)
    with pytest.raises(HalError, match=r"page_tree_plan_device: negative argument .*D -2\)"):
        zhal.HipHal.page_tree_plan_device(hal, 10, 500, 64, table, 0, -2)


def test_seal_page_out_tree_takes_the_plan_from_the_host_or_the_device():
    from zeth_amd.prover import SegmentProver
    with pytest.raises(HalError, match=re.escape('seal_page_out_tree: plan="other" (the plan is made on the "host" or on the "device")')):
        SegmentProver.seal_page_out_tree(object.__new__(SegmentProver), [], None, 0, None, None, plan="other")
