"""P2-PAGE-ordered on the host (zeth_amd/circuits/p2_page_ordered.py): P2-PAGE plus the constraint that a page-out's addresses strictly
increase.  The description's shape, and P2-PAGE's blob word for word beside it; the Python reference's code and data traces against the
circuit's own constraints row by row (circuits/check.py) over page_ordered_cases.GRID, with out[16:18] against the plain formula; the
gap this closes: two witnesses that P2-PAGE's constraints accept (addresses that decrease, one address written twice), each refused by
the `order` family on the offending slot's gend row; six tampered witnesses, each refused on the named row by `order`; and
prover.verify_page_ordered_chain on seals made by the CPU oracle's prover: the chain of three parts, and one message per cause."""
import numpy as np
import pytest

import page_circuit_cases as cases
import page_ordered_cases as oc
import zko
from zeth_amd.circuits import check, p2_page, p2_page_ordered as G
from zeth_amd.circuits.desc import Circuit
from zeth_amd.prover import desc_key

P = cases.P
ONE = cases.ONE
BLOCK = p2_page.BLOCK_ROWS


def _mix(seed=7):
    return np.random.default_rng(seed).integers(0, P, 4, dtype=np.uint64).astype(np.uint32)


def _first_failure(oracle, desc, family_of, po2, zk, code, data, out):
    """(lowest failing row or -1, the constraint family of its lowest failing step) of a witness of `desc`; the accum group is
    P2-JOIN's argument by the oracle, as for P2-PAGE"""
    mix = _mix()
    circuit = zko.OracleCircuit(oracle, desc)
    accum = np.zeros(4 << po2, np.uint32)
    oracle.zko_syn_accum(circuit.h, po2, zk, zko.key_words(cases.NOISE), np.ascontiguousarray(data).reshape(-1), mix, accum)
    f = check.reference_check_rows(desc, po2, accum, code, data, out, mix)
    row, step, _ = check.first_failure(f)
    return row, None if row < 0 else family_of(step)


def _ordered(oracle, po2, zk, code, data, out):
    return _first_failure(oracle, G.p2_page_ordered_circuit(), G.family_of, po2, zk, code, data, out)


def test_description_shape_and_p2_page_is_unchanged():
    desc = G.p2_page_ordered_circuit()
    c = Circuit.parse(desc)
    assert c.group_sizes == (G.WA, G.WC, G.WD) == (4, 42, 129) and c.global_sizes == (18, 4) and c.kind == G.KIND_P2_PAGE_ORDERED == 6
    assert all(back <= 1 for _, _, back in c.taps), "every constraint is local: backs 0 and 1"
    deg = p2_page.constraint_degrees(desc)
    assert max(deg) == 3 and len(deg) == 328 + 12, "P2-PAGE's 328 constraints and the 12 of `order`"
    names = [name for name, _, _ in G.FAMILIES]
    assert names == ["rounds", "leaf_in", "node_in", "carry", "top_out", "roots", "order", "accum", "sanity"]
    # `order` alone: degree <= 2 before the selector
    lo, hi = next((lo, hi) for name, lo, hi in G.FAMILIES if name == "order")
    and_eqz = [i for i, s in enumerate(c.steps) if s[0] == 8]
    assert max(d for i, d in zip(and_eqz, deg) if lo <= i < hi) == 2
    assert G.MAX_H == 26 == p2_page.MAX_H - 1 and G.GAP_BITS == 29
    # P2-PAGE beside it: the same blob as before the two builders shared their constraint text
    page = p2_page.p2_page_circuit()
    assert desc_key(page) == "e2f98890c416e4a2" and page.size == 13303 and len(p2_page.constraint_degrees(page)) == 328
    assert [name for name, _, _ in p2_page.FAMILIES] == [n for n in names if n != "order"]


def test_it_is_shipped_after_p2_page():
    from zeth_amd.circuits import codegen
    names = list(codegen.shipped())
    assert names[-2:] == ["p2_page", "p2_page_ordered"]
    assert np.array_equal(codegen.shipped()["p2_page_ordered"], G.p2_page_ordered_circuit())


@pytest.mark.parametrize("g", oc.GRID, ids=oc.grid_id)
def test_reference_witness_satisfies_every_constraint(oracle, g):
    (po2, zk, W), what, first = g
    t = oc.table(po2, zk, W, what)
    data, out, code = oc.part(po2, zk, W, what, first)
    assert _ordered(oracle, po2, zk, code, data, out) == (-1, None)
    lo, hi = oc.bounds(t, first)
    assert [G.decode(out[16]), G.decode(out[17])] == [lo, hi] and (int(out[16]), int(out[17])) == (lo * ONE % P, hi * ONE % P)
    # columns 0 .. 124 and code columns 0 .. 38 are P2-PAGE's
    if (po2, zk, W) in cases.SHAPES and what in (0, 1, 3, "N", "first_last"):  # the cases page_circuit_cases holds: same image, same table
        c = cases.case(po2, zk, W, what)
        assert np.array_equal(data[:p2_page.WD], c["data"]) and np.array_equal(out[:16], c["out"])
    assert np.array_equal(code[:p2_page.WC], p2_page.reference_page_code(po2, zk, t["h"]))
    # live slots first, then dead ones; the new columns are zero past the last path, and the new selectors too
    path = BLOCK * t["h"]
    count = min(t["N"], len(t["addrs"]) - first)
    live = data[G.D_LIVE, 0:path * t["N"]:path]
    assert live.tolist() == [ONE] * count + [0] * (t["N"] - count)
    assert not data[G.D_LIVE:, path * t["N"]:].any() and not code[G.C_GSEL:, path * t["N"]:].any()


def test_the_gap_bits_reach_2_to_the_13th_and_the_gap_of_zero():
    po2, zk, W = oc.H12
    data, _, _ = oc.part(po2, zk, W, "first_last")
    path = BLOCK * 12
    g = W - 2                                                                 # [0, W - 1]: slot 1's gap is W - 1 - 1
    assert g >> 13 and [int(data[G.D_GBIT, path + 1 + k] == ONE) for k in range(G.GAP_BITS)] == [(g >> k) & 1 for k in range(G.GAP_BITS)]
    assert int(data[G.D_GACC, path + G.GAP_BITS]) == g * ONE % P and data[G.D_GACC, path + G.GAP_BITS + 1] == 0 == data[G.D_GACC, path]
    data, _, _ = oc.part(*cases.SHAPES[1], "adjacent")
    path = BLOCK * 5
    assert not data[G.D_GBIT:, path:3 * path].any(), "[5, 6, 7]: slots 1 and 2 follow at a gap of 0"
    assert G.decode(data[G.D_GACC, G.GAP_BITS]) == 5 and G.decode(data[G.D_GACC, 3 * path + G.GAP_BITS]) == cases.SHAPES[1][2] - 1 - 8


def test_the_reference_refuses_what_it_cannot_lay_out():
    with pytest.raises(ValueError, match="h 27"):
        G.reference_ordered_code(12, 1994, 27)
    assert G.reference_ordered_code(12, 100, 26).shape == (42, 4096)
    with pytest.raises(ValueError, match="first 3, but the table has 3 rows"):
        t = oc.table(*cases.SHAPES[1], 3)
        G.reference_ordered_part(*cases.SHAPES[1], t["table"], t["image"], 3)


# ---- the gap this closes: witnesses P2-PAGE accepts and the ordered circuit refuses ----
def _stitched(po2, zk, W, image, updates):
    """P2-PAGE's 125 columns and 16 outputs of the updates [(a, out), ...] applied in THAT order, whatever their addresses: every path is
    self-contained, so slot s is slot 0 of a single-update reference trace over the image as the updates before it left it, and the
    no-op slots are those of the last such trace"""
    h = p2_page.tree_height(W)
    N, path, n = p2_page.slots(po2, zk, h), BLOCK * h, 1 << po2
    data = np.zeros((p2_page.WD, n), dtype=np.uint32)
    image = np.array(image, dtype=np.uint32)
    for s, (a, w_out) in enumerate(updates):
        active, before, after = p2_page.reference_page_trace(po2, zk, W, [(a, int(image[a]) % P, w_out)], image)
        data[:, path * s:path * (s + 1)] = active[:, :path]
        if s == 0:
            root_before = before
        image[a] = w_out
    rest = N - len(updates)
    data[:, path * len(updates):path * N] = active[:, path:path * (1 + rest)]
    return data, np.concatenate([root_before, after]).astype(np.uint32)


def _best_order_columns(po2, zk, h, addrs):
    """the new columns the best a prover can for live updates at `addrs`, in order: lo as the constraints force it, the gap's bits the
    low 29 bits of (addr - lo) mod P -> ((4, n), lo of slot 0, hi)"""
    n = 1 << po2
    N, path = p2_page.slots(po2, zk, h), BLOCK * h
    cols = np.zeros((4, n), dtype=np.uint32)
    lo = 0
    for s in range(N):
        live = s < len(addrs)
        g = ((addrs[s] - lo) % P) & ((1 << G.GAP_BITS) - 1) if live else 0
        r0 = path * s
        cols[0, r0:r0 + path] = ONE * live
        cols[1, r0:r0 + path] = lo * ONE % P
        for k in range(1, G.GAP_BITS + 1):
            cols[2, r0 + k] = ONE * ((g >> (k - 1)) & 1)
            cols[3, r0 + k] = (g % (1 << k)) * ONE % P
        if live:
            lo = addrs[s] + 1
    return cols, 0, lo


@pytest.mark.parametrize("addrs", [[77, 20], [77, 77], [20, 77]], ids=["decreasing", "twice", "increasing"])
def test_p2_page_accepts_an_unordered_table_and_the_ordered_circuit_refuses_it(oracle, addrs):
    po2, zk, W = cases.SHAPES[1]
    t = oc.table(po2, zk, W, 3)
    h, path = t["h"], BLOCK * t["h"]
    page, out16 = _stitched(po2, zk, W, t["image"], [(addrs[0], 1111), (addrs[1], 2222)])
    # the hole as it stands: every P2-PAGE constraint holds
    assert _first_failure(oracle, p2_page.p2_page_circuit(), p2_page.family_of, po2, zk, p2_page.reference_page_code(po2, zk, h), page, out16) == (-1, None)
    cols, lo, hi = _best_order_columns(po2, zk, h, addrs)
    data = np.concatenate([page, cols])
    out = np.concatenate([out16, [lo * ONE % P, hi * ONE % P]]).astype(np.uint32)
    want = (-1, None) if addrs[0] < addrs[1] else (path + G.GAP_BITS, "order")   # slot 1's gend row
    assert _ordered(oracle, po2, zk, oc.code_of(po2, zk, h), data, out) == want


# ---- tampered witnesses: the lowest failing row and its constraint family ----
def _bump(w):
    return np.uint32((int(w) + ONE) % P)


@pytest.fixture(scope="module")
def tamper_case():
    po2, zk, W = cases.SHAPES[1]                                             # h = 5, N = 13, D = 3: slots 3 .. 12 are dead
    data, out, code = oc.part(po2, zk, W, 3)
    return {"po2": po2, "zk": zk, "path": BLOCK * 5, "N": 13, "data": data, "out": out, "code": code}


def _tampered(oracle, c, data=None, out=None):
    return _ordered(oracle, c["po2"], c["zk"], c["code"], c["data"] if data is None else data, c["out"] if out is None else out)


def test_tamper_lo_along_a_path(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = c["path"]
    data[G.D_LO, r:r + c["path"]] = _bump(data[G.D_LO, r])                    # `carry` holds; slot 1 no longer starts after slot 0's address
    assert _tampered(oracle, c, data) == (r, "order")


def test_tamper_one_gbit(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = 2 * c["path"] + 4
    data[G.D_GBIT, r] = ONE - data[G.D_GBIT, r]
    assert _tampered(oracle, c, data) == (r, "order")


def test_tamper_live_set_on_the_first_dead_slot(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = 3 * c["path"]
    assert data[G.D_LIVE, r] == 0 and data[G.D_LIVE, r - 1] == ONE
    data[G.D_LIVE, r:r + c["path"]] = ONE                                     # a no-op of address 0 below lo: no gap of 29 bits reaches it
    assert _tampered(oracle, c, data) == (r + G.GAP_BITS, "order")


def test_tamper_live_cleared_on_a_real_slot(oracle, tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    r = 2 * c["path"]
    assert data[p2_page.D_W_IN, r] != data[p2_page.D_W_OUT, r]
    data[G.D_LIVE, r:r + c["path"]] = 0                                       # a dead slot that changes a word
    assert _tampered(oracle, c, data) == (r, "order")


def test_tamper_hi_in_out(oracle, tamper_case):
    c, out = tamper_case, tamper_case["out"].copy()
    out[17] = _bump(out[17])
    assert _tampered(oracle, c, out=out) == (c["path"] * c["N"] - 1, "order")  # the last path's top row


def test_tamper_lo_in_out(oracle, tamper_case):
    c, out = tamper_case, tamper_case["out"].copy()
    out[16] = _bump(out[16])
    assert _tampered(oracle, c, out=out) == (0, "order")


# ---- the chain verifier on seals made by the CPU oracle (its prover takes any code / data / out; the accum group is its own) ----
H5 = cases.SHAPES[1]


def _fmt(r):
    return " ".join(f"{int(w):08x}" for w in r)


def _oracle_seal(circuit, index, code, data, out):
    from zeth_amd.prover import SegmentReceipt
    po2, zk, _ = H5
    return SegmentReceipt(seal=circuit.prove_traces(po2, code, data, out, zk_cycles=zk, noise_seed=cases.NOISE + index), index=index, po2=po2)


@pytest.fixture(scope="module")
def chain(oracle):
    """the three parts of the table of 29 rows at h = 5, sealed -> (receipts, the control root, the table)"""
    po2, zk, W = H5
    circuit = zko.OracleCircuit(oracle, G.p2_page_ordered_circuit())
    recs = []
    for p, first in enumerate((0, 13, 26)):
        data, out, code = oc.part(po2, zk, W, "2N+3", first)
        recs.append(_oracle_seal(circuit, p, code, data, out))
    return recs, circuit.root_of_code(po2, oc.code_of(po2, zk, 5)), oc.table(po2, zk, W, "2N+3"), circuit


def test_the_chain_of_seals_gives_both_roots_and_hi(chain):
    from zeth_amd.circuits import logup
    from zeth_amd.prover import verify_page_ordered_chain
    recs, root, t, _ = chain
    root_before, root_after = logup.reference_image_root(t["image"]), logup.reference_image_root(t["image_after"])
    for given in (root_before, None):
        got = verify_page_ordered_chain(recs, root, given)
        assert np.array_equal(got[0], root_before) and np.array_equal(got[1], root_after) and got[2] == int(t["addrs"][-1]) + 1
    got = verify_page_ordered_chain(recs[:1], root)                            # a chain may stop early: it says where it stopped
    assert np.array_equal(got[1], recs[1].seal[:8]) and got[2] == int(t["addrs"][12]) + 1


def test_the_chain_verifier_refuses_one_message_per_cause(chain):
    from zeth_amd.hal import HalError
    from zeth_amd.prover import SegmentReceipt, verify_page_ordered_chain
    recs, root, t, circuit = chain
    po2, zk, W = H5
    # every seal is good, the chain is not: two parts swapped, a part dropped, another first root
    with pytest.raises(HalError, match=f"part 0 starts at lo {int(t['addrs'][12]) + 1}, not 0"):
        verify_page_ordered_chain([recs[1], recs[0], recs[2]], root)
    for broken in ([recs[0], recs[2], recs[1]], [recs[0], recs[2]]):
        with pytest.raises(HalError, match=f"part 1 opens root {_fmt(recs[2].seal[:8])}, but part 0 left root {_fmt(recs[0].seal[8:16])}"):
            verify_page_ordered_chain(broken, root)
    with pytest.raises(HalError, match=f"part 0 opens root {_fmt(recs[0].seal[:8])}, not root_before {_fmt(recs[2].seal[8:16])}"):
        verify_page_ordered_chain(recs, root, recs[2].seal[8:16])
    with pytest.raises(HalError, match="no receipt"):
        verify_page_ordered_chain([], root)
    # a seal with `lo` altered, and another control root: the verifier of the seal refuses
    bad = recs[1].seal.copy()
    bad[16] = recs[0].seal[16]
    with pytest.raises(HalError, match="verify_segment: "):
        verify_page_ordered_chain([recs[0], SegmentReceipt(seal=bad, index=1, po2=po2), recs[2]], root)
    with pytest.raises(HalError, match="verify_segment: "):
        verify_page_ordered_chain(recs, circuit.root_of_code(po2, oc.code_of(po2, zk, 3)))
    # P2-PAGE's seal of the same part is not an ordered seal
    page = zko.OracleCircuit(circuit.lib, p2_page.p2_page_circuit())
    data, out, code = oc.part(po2, zk, W, "2N+3", 0)
    plain = _oracle_seal(page, 0, code[:p2_page.WC], data[:p2_page.WD], out[:16])
    with pytest.raises(HalError, match="verify_segment: "):
        verify_page_ordered_chain([plain], page.root_of_code(po2, code[:p2_page.WC]))


def test_two_seals_whose_roots_link_but_whose_addresses_go_back(chain):
    """updates that write the word already there leave the root as it is, so any two single-part seals over one image link by their
    roots: what P2-PAGE's chain accepted in any order, and what lo = hi refuses"""
    from zeth_amd.hal import HalError
    from zeth_amd.prover import verify_page_ordered_chain
    _, root, t, circuit = chain
    po2, zk, W = H5
    recs = []
    for p, a in enumerate((77, 20)):
        w = int(t["image"][a]) % P
        data, out = G.reference_ordered_part(po2, zk, W, [(a, w, w)], t["image"])
        full = np.zeros((G.WD, 1 << po2), dtype=np.uint32)
        full[:, :(1 << po2) - zk] = data
        assert np.array_equal(out[:8], out[8:16]) and [G.decode(out[16]), G.decode(out[17])] == [0, a + 1]
        recs.append(_oracle_seal(circuit, p, oc.code_of(po2, zk, 5), full, out))
    with pytest.raises(HalError, match="part 1 starts at lo 0, but part 0 left hi 78"):
        verify_page_ordered_chain(recs, root)
    with pytest.raises(HalError, match="part 1 starts at lo 0, but part 0 left hi 21"):
        verify_page_ordered_chain(recs[::-1], root)
    assert verify_page_ordered_chain(recs[:1], root)[2] == 78


def test_a_lo_the_order_check_is_not_sound_for_is_refused_by_the_chain_verifier(oracle, chain):
    """a part with no live update satisfies every constraint for ANY lo = hi, also one above 2^29: the circuit's induction starts from a
    checked out[16], and the chain verifier is who checks it"""
    from zeth_amd.hal import HalError
    from zeth_amd.prover import verify_page_ordered_chain
    _, root, _, circuit = chain
    po2, zk, W = H5
    data, out, code = oc.part(po2, zk, W, 0)
    data, out = data.copy(), out.copy()
    x = (1 << 29) + 1
    data[G.D_LO, :BLOCK * 5 * 13] = x * ONE % P
    out[16] = out[17] = x * ONE % P
    assert _ordered(oracle, po2, zk, code, data, out) == (-1, None)
    with pytest.raises(HalError, match=f"part 0: lo {x} is above 2\\^29"):
        verify_page_ordered_chain([_oracle_seal(circuit, 0, code, data, out)], root)
    data[G.D_LO, :BLOCK * 5 * 13] = out[16] = out[17] = np.uint32((1 << 29) * ONE % P)     # 2^29 itself is in range: then lo != 0 is the refusal
    with pytest.raises(HalError, match=f"part 0 starts at lo {1 << 29}, not 0"):
        verify_page_ordered_chain([_oracle_seal(circuit, 0, code, data, out)], root)
