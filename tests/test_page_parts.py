"""P2-PAGE's parts on the host (p2_page.parts, p2_page.reference_page_part, zkh_page_circuit_slots): the plan of a table of D rows
against the slot arithmetic, the planner of the library against the Python one, and a table of D = 30 rows at h = 5, N = 13 (parts of
13, 13 and 4 updates): the middle part's trace and the last one's (the only one with no-op slots) against the circuit's own
constraints row by row (circuits/check.py), the chain of the parts' roots, and its two ends against the tree of the image before and
after the whole page-out (logup.reference_image_root: the library's host permutation, another implementation than the reference's)."""
import numpy as np
import pytest

import page_circuit_cases as cases
import page_parts_cases as pp
import zko
from zeth_amd import hal as zhal
from zeth_amd.circuits import check, logup, p2_page as G

P = cases.P
BLOCK = G.BLOCK_ROWS
PO2, ZK, W = pp.H5


def test_parts_follow_the_slot_arithmetic():
    N = G.slots(PO2, ZK, G.tree_height(W))
    assert N == 13 == ((1 << PO2) - ZK) // BLOCK // 5
    assert G.parts(PO2, ZK, W, 0) == [(0, 0)]
    assert G.parts(PO2, ZK, W, 5) == [(0, 5)]
    assert G.parts(PO2, ZK, W, N) == [(0, N)]
    assert G.parts(PO2, ZK, W, N + 1) == [(0, N), (N, 1)]
    assert G.parts(PO2, ZK, W, 3 * N) == [(0, N), (N, N), (2 * N, N)]
    for D in (0, 1, N - 1, N, N + 1, 30, 3 * N, 3 * N + 1):
        plan = G.parts(PO2, ZK, W, D)
        assert len(plan) == max(1, -(-D // N)) and sum(c for _, c in plan) == D
        assert all(f == p * N and c == min(N, D - f) for p, (f, c) in enumerate(plan))
        assert all(c == N for _, c in plan[:-1]), "only the last part has slots left over"
    with pytest.raises(ValueError, match="no path slot"):
        G.parts(PO2, ZK, 8, 3)
    with pytest.raises(ValueError, match="no path slot"):
        G.parts(8, 200, 1 << 20, 3)                                            # 56 active rows: one block, h = 17


def test_the_librarys_planner_is_the_python_one():
    lib = zhal.load_library()
    for po2, zk, w in [pp.H5, (10, 900, 16), (12, 1994, 64), (12, 200, 64), (20, 1994, 1 << 20), (20, 1994, 1 << 26), (13, 1994, 9), (24, 1994, 1 << 30)]:
        assert lib.zkh_page_circuit_slots(po2, zk, w) == G.slots(po2, zk, G.tree_height(w)) > 0, (po2, zk, w)
    assert lib.zkh_page_circuit_slots(20, 1994, 1 << 20) == 1985 and lib.zkh_page_circuit_slots(20, 1994, 1 << 26) == 1467
    # what zkh_page_circuit_code refuses: a single leaf, h > 27, no room for one path, a po2 out of range
    for po2, zk, w in [(12, 1994, 8), (12, 1994, 0), (24, 1994, (1 << 30) + 1), (8, 200, 1 << 20), (0, 0, 64), (31, 1994, 64), (10, 1023, 64)]:
        assert lib.zkh_page_circuit_slots(po2, zk, w) == 0, (po2, zk, w)


def _first_failure(oracle, data, out):
    mix = np.random.default_rng(7).integers(0, P, 4, dtype=np.uint64).astype(np.uint32)
    oc = zko.OracleCircuit(oracle, G.p2_page_circuit())
    accum = np.zeros(G.WA << PO2, np.uint32)
    oracle.zko_syn_accum(oc.h, PO2, ZK, zko.key_words(cases.NOISE), np.ascontiguousarray(data).reshape(-1), mix, accum)
    f = check.reference_check_rows(G.p2_page_circuit(), PO2, accum, G.reference_page_code(PO2, ZK, G.tree_height(W)), data, out, mix)
    row, step, _ = check.first_failure(f)
    return row, None if row < 0 else G.family_of(step)


@pytest.mark.parametrize("first", [13, 26])
def test_a_parts_reference_witness_satisfies_every_constraint(oracle, first):
    t = pp.table(PO2, ZK, W, 30)
    assert t["plan"] == [(0, 13), (13, 13), (26, 4)] and t["h"] == 5
    data, out = pp.part(PO2, ZK, W, 30, first)
    assert _first_failure(oracle, data, out) == (-1, None)
    # slot s holds update first + s; the slots past the part's count are no-ops of address 0 under the tree after the page-out
    count = dict(t["plan"])[first]
    enc = lambda a: a * cases.ONE % P
    for s in range(t["N"]):
        r = BLOCK * t["h"] * s
        a, w_in, w_out = t["table"][first + s] if s < count else (0, int(t["image_after"][0]) % P, int(t["image_after"][0]) % P)
        assert (int(data[G.D_ADDR, r]), int(data[G.D_W_IN, r]), int(data[G.D_W_OUT, r])) == (enc(a), w_in, w_out), f"slot {s}"
    # the part's out is not the whole page-out's: with the first root of part 0 the first path does not open it
    wrong = out.copy()
    wrong[:8] = pp.part(PO2, ZK, W, 30, 0)[1][:8]
    assert _first_failure(oracle, data, wrong) == (0, "roots")


def test_the_parts_roots_chain_from_the_tree_before_to_the_tree_after():
    t = pp.table(PO2, ZK, W, 30)
    outs = [pp.part(PO2, ZK, W, 30, first)[1] for first, _ in t["plan"]]
    for p in range(len(outs) - 1):
        assert np.array_equal(outs[p][8:], outs[p + 1][:8]), f"part {p + 1} does not open the root part {p} left"
        assert not np.array_equal(outs[p][:8], outs[p][8:])
    assert np.array_equal(outs[0][:8], logup.reference_image_root(t["image"]))
    assert np.array_equal(outs[-1][8:], logup.reference_image_root(t["image_after"]))
    for (first, count), out in zip(t["plan"], outs):                           # and every root in between is the tree's at that point
        assert np.array_equal(out[:8], logup.reference_image_root(pp.image_at(t, first)))
        assert np.array_equal(out[8:], logup.reference_image_root(pp.image_at(t, first + count)))


def test_the_reference_refuses_a_first_past_the_table():
    t = pp.table(PO2, ZK, W, 30)
    for first in (30, 31):
        with pytest.raises(ValueError, match=f"first {first}, but the table has 30 rows"):
            G.reference_page_part(PO2, ZK, W, t["table"], t["image"], first)
    data, root_before, root_after = G.reference_page_part(PO2, ZK, W, [], t["image"], 0)       # the empty table's one part
    assert np.array_equal(root_before, root_after) and np.array_equal(root_before, logup.reference_image_root(t["image"]))
