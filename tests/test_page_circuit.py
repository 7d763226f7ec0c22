"""P2-PAGE on the host (zeth_amd/circuits/p2_page.py): the circuit that proves a page-out of the committed memory image from root to root.
The description and its degree bound; the Python reference's code and data traces against the circuit's own constraints row by row
(circuits/check.py: the definition, no mix, no probability) for every shape and D in {0, 1, 3, N}; its roots against the tree of the
image before and after (logup.reference_image_tree, which hashes through the library's host permutation: another implementation than
the reference's hash_pair_words) and against the walk of the ZKU1 proof of the same table (zkh_image_proof_verify); and seven tampered
witnesses, each refused on the row and by the constraint family that owns the tampered cell."""
import json
import os

import numpy as np
import pytest

import page_circuit_cases as cases
import zko
from zeth_amd import hal as zhal
from zeth_amd.circuits import check, logup, p2_join, p2_page as G
from zeth_amd.circuits.desc import Circuit
from zeth_amd.prover import desc_key

P = cases.P
ONE = cases.ONE
BLOCK = G.BLOCK_ROWS


def _mix(seed=7):
    return np.random.default_rng(seed).integers(0, P, 4, dtype=np.uint64).astype(np.uint32)


def _accum(oracle, po2, zk, data, mix):
    """P2-JOIN's accum argument by the oracle: one Fp4 running product of (mix + data column 0)"""
    oc = zko.OracleCircuit(oracle, G.p2_page_circuit())
    accum = np.zeros(G.WA << po2, np.uint32)
    oracle.zko_syn_accum(oc.h, po2, zk, zko.key_words(cases.NOISE), np.ascontiguousarray(data).reshape(-1), mix, accum)
    return accum


def _first_failure(oracle, c, data=None, out=None):
    """(lowest failing row or -1, the constraint family of its lowest failing step) of the case's witness, with `data` / `out` replaced"""
    data = c["data"] if data is None else data
    out = c["out"] if out is None else out
    mix = _mix()
    f = check.reference_check_rows(G.p2_page_circuit(), c["po2"], _accum(oracle, c["po2"], c["zk"], data, mix), c["code"], data, out, mix)
    row, step, _ = check.first_failure(f)
    return row, None if row < 0 else G.family_of(step)


def test_description_shape_and_degree():
    desc = G.p2_page_circuit()
    c = Circuit.parse(desc)
    assert c.group_sizes == (G.WA, G.WC, G.WD) == (4, 39, 125) and c.global_sizes == (16, 4) and c.kind == G.KIND_P2_PAGE == 5
    assert all(back <= 1 for _, _, back in c.taps), "every constraint is local: backs 0 and 1"
    deg = G.constraint_degrees(desc)
    assert len(deg) > 300 and max(deg) == 3, "degree <= 3 before the selector (the cubes and the x^7 links reach it)"
    assert [name for name, _, _ in G.FAMILIES] == ["rounds", "leaf_in", "node_in", "carry", "top_out", "roots", "accum", "sanity"]
    # the degree check on constraints whose degree is known: P2-JOIN's are <= 3 too, a hand-made product of four taps is 4
    assert max(G.constraint_degrees(p2_join.p2_join_circuit())) == 3
    from zeth_amd.circuits.desc import GROUP_DATA, CircuitBuilder
    b = CircuitBuilder((0, 0, 4), (1, 1))
    x = [b.get(GROUP_DATA, i) for i in range(4)]
    assert G.constraint_degrees(b.finish(b.and_eqz(b.true(), b.mul(b.mul(x[0], x[1]), b.mul(x[2], x[3]))))) == [4]


def test_p2_join_description_is_unchanged():
    """P2-JOIN's blob, word for word: its hash is the key of its pinned control roots"""
    with open(os.path.join(os.path.dirname(zhal.__file__), "circuits", "control_roots.json")) as fh:
        names = json.load(fh)["names"]
    assert names.get(desc_key(p2_join.p2_join_circuit())) == "p2_join"


@pytest.mark.parametrize("what", [0, 1, 3, "N"])
@pytest.mark.parametrize("po2,zk,W", cases.SHAPES)
def test_reference_witness_satisfies_every_constraint_and_its_roots_are_the_trees(oracle, po2, zk, W, what):
    c = cases.case(po2, zk, W, what)
    D = len(c["addrs"])
    assert D == (c["N"] if what == "N" else what) and c["N"] == ((1 << po2) - zk) // BLOCK // c["h"]
    assert _first_failure(oracle, c) == (-1, None)
    before, after = logup.reference_image_tree(c["image"]), logup.reference_image_tree(c["image_after"])
    assert np.array_equal(c["out"][:8], before[1]) and np.array_equal(c["out"][8:], after[1])
    proof = cases.host_proof(c["image"], c["addrs"], c["outs"], before)
    assert np.array_equal(zhal.image_proof_verify(proof, c["out"][:8]), c["out"][8:])
    if D == 0:
        assert np.array_equal(c["out"][:8], c["out"][8:])
    # rows past the last path are zero, and the code group selects nothing there
    rows = BLOCK * c["h"] * c["N"]
    assert not c["data"][:, rows:].any() and not c["code"][3:, rows:].any()


def test_the_reference_refuses_what_it_cannot_lay_out():
    po2, zk, W = cases.SHAPES[1]
    N = cases.slots(po2, zk, W)
    image = np.arange(1, W + 1, dtype=np.uint32)
    with pytest.raises(ValueError, match=f"D {N + 1} updates, but h 5 at po2 12 leaves N {N} path slots"):
        G.reference_page_trace(po2, zk, W, [(a, a + 1, 0) for a in range(N + 1)], image)
    with pytest.raises(ValueError, match="W > 8"):
        G.reference_page_trace(po2, zk, 8, [], image[:8])
    with pytest.raises(ValueError, match="row 1: address 4 does not follow 9"):
        G.reference_page_trace(po2, zk, W, [(9, 10, 0), (4, 5, 0)], image)
    with pytest.raises(ValueError, match="row 0: in 77 at address 9, but the tree holds 10"):
        G.reference_page_trace(po2, zk, W, [(9, 77, 0)], image)


# ---- tampered witnesses: one cell (or one column along one path) changed; the lowest failing row and its constraint family ----
def _bump(w):
    return np.uint32((int(w) + ONE) % P)


@pytest.fixture(scope="module")
def tamper_case():
    return cases.case(*cases.SHAPES[1], 3)                       # h = 5, N = 13, D = 3: slots 3 .. 12 are no-ops


def _path(c, slot):
    return BLOCK * c["h"] * slot


def test_tamper_sibling_on_the_new_side_only(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = _path(c, 1) + BLOCK * 2                                  # the input row of block 2 of slot 1
    bit = int(data[G.D_B, r] == ONE)
    data[G.D_SN + (0 if bit else 8) + 5, r] = _bump(data[G.D_SN + (0 if bit else 8) + 5, r])
    assert _first_failure(oracle, c, data) == (r, "node_in")


def test_tamper_path_bit_flipped(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = _path(c, 0) + BLOCK * 3
    data[G.D_B, r] = ONE - data[G.D_B, r]
    assert _first_failure(oracle, c, data) == (r, "node_in")


def test_tamper_second_e_set(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = _path(c, 2)
    j = (int(c["addrs"][2]) + 1) & 15
    assert data[G.D_E + j, r] == 0
    data[G.D_E + j, r] = ONE
    assert _first_failure(oracle, c, data) == (r, "leaf_in")


def test_tamper_w_in(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = _path(c, 1)
    data[G.D_W_IN, r:r + BLOCK * c["h"]] = _bump(data[G.D_W_IN, r])              # along the whole path: `carry` holds, the opening does not
    assert _first_failure(oracle, c, data) == (r, "leaf_in")


def test_tamper_cur_in_the_middle_of_a_path(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = _path(c, 1) + BLOCK * 2 + 7
    data[G.D_CUR + 3, r] = _bump(data[G.D_CUR + 3, r])
    assert _first_failure(oracle, c, data) == (r, "carry")


def test_tamper_root_after_in_out(oracle, tamper_case):
    c, out = tamper_case, tamper_case["out"].copy()
    out[8] = _bump(out[8])
    assert _first_failure(oracle, c, out=out) == (_path(c, c["N"]) - 1, "roots")         # the last path's output row


def test_tamper_w_out_of_a_no_op_slot(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    slot = len(c["addrs"]) + 2
    r = _path(c, slot)
    assert data[G.D_W_OUT, r] == data[G.D_W_IN, r] == c["image_after"][0] % P and data[G.D_ADDR, r] == 0
    data[G.D_W_OUT, r:r + BLOCK * c["h"]] = _bump(data[G.D_W_OUT, r])
    assert _first_failure(oracle, c, data) == (r, "leaf_in")
