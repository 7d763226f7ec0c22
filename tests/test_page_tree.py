"""P2-TREE on the host (zeth_amd/circuits/p2_tree.py): a page-out sealed by its dirty nodes.  The description's shape; the Python
reference's code and data traces against the circuit's own constraints row by row (circuits/check.py) over page_tree_cases.grid(), the
accum group from logup.reference_accumulate, with the roots against logup.reference_image_tree and the bus against logup.reference_bus;
the plan; tampered witnesses, each refused in the named family or by the bus; what the chain verifier checks of the parts' outputs; and
the roots against P2-PAGE-ordered's reference for the same tables.

The CPU oracle's prover builds P2-JOIN's accum group and has no bus, so it cannot seal a P2-TREE witness: the chain verifier runs on
real seals in tests/test_page_tree_gpu.py, and here its linking rules (prover.link_page_tree_chain, everything it does after the seals
are verified) run on the reference's outputs."""
import numpy as np
import pytest

import page_tree_cases as tc
from zeth_amd.circuits import check, logup, p2_page, p2_page_ordered, p2_tree as G
from zeth_amd.circuits.desc import Circuit

P = tc.P
ONE = tc.ONE
BLOCK = p2_page.BLOCK_ROWS


def _mix(seed=7):
    return np.random.default_rng(seed).integers(0, P, G.MIX_WORDS, dtype=np.uint64).astype(np.uint32)


def _first_failure(po2, zk, code, data, out):
    """(lowest failing row or -1, the constraint family of its lowest failing step); the accum group is the bus's running sums as they
    come out, balanced or not"""
    mix = _mix()
    accum, _ = logup.reference_accumulate(tc.args(), po2, zk, code, data, mix, check_balance=False)
    f = check.reference_check_rows(G.p2_tree_circuit(), po2, accum, code, data, out, mix)
    row, step, _ = check.first_failure(f)
    return row, None if row < 0 else G.family_of(step)


def test_description_shape():
    desc = G.p2_tree_circuit()
    c = Circuit.parse(desc)
    assert c.group_sizes == (G.WA, G.WC, G.WD) == (24, 41, 106) and c.global_sizes == (18, 8) and c.kind == G.KIND_P2_TREE == 7
    assert all(back <= 1 for _, _, back in c.taps), "every constraint is local: backs 0 and 1"
    names = [name for name, _, _ in G.FAMILIES]
    assert names == ["rounds", "in_row", "carry", "order", "root", "bus", "sanity"]
    deg = p2_page.constraint_degrees(desc)
    and_eqz = [i for i, s in enumerate(c.steps) if s[0] == 8]
    assert len(and_eqz) == len(deg)
    bus = next((lo, hi) for name, lo, hi in G.FAMILIES if name == "bus")
    assert max(d for i, d in zip(and_eqz, deg) if not bus[0] <= i < bus[1]) == 3, "degree at most 3 outside the bus"
    a = tc.args()
    assert a.k == 6 and len(a.terms) == 18 and not a.records and (a.alpha, a.beta) == (0, 4) and a.version == 1
    assert sorted({t.tag for t in a.terms}) == [1, 2, 3, 4, 5, 6] and [len(t.tuple_cols) for t in a.terms] == [4] * 15 + [2] * 3
    for col in a.by_column():
        assert [(t.sign, t.sel, t.mult[1]) for t in col] == [(-1, G.C_OUT_ROW, G.D_UP), (1, G.C_IN_ROW, G.D_DL), (1, G.C_IN_ROW, G.D_DR)]
        assert logup.column_degree(col) == logup.MAX_DEGREE
    # P2-PAGE and P2-PAGE-ordered beside it share the round constraints' text and are the blobs they were
    from zeth_amd.prover import desc_key
    assert desc_key(p2_page.p2_page_circuit()) == "e2f98890c416e4a2" and desc_key(p2_page_ordered.p2_page_ordered_circuit()) == "73f180df9134546b"


@pytest.mark.parametrize("g", tc.grid(), ids=tc.grid_id)
def test_reference_witness_satisfies_every_constraint(g):
    (po2, zk, W), what, p = g
    t = tc.table(po2, zk, W, what)
    data, out, code = tc.part(po2, zk, W, what, p)
    assert _first_failure(po2, zk, code, data, out) == (-1, None)
    assert logup.reference_bus(tc.args(), po2, zk, code, data)["row"] == -1
    first, count = t["plan"][p]
    # the roots are those of plain trees over the image with the table's rows [0, first) and [0, first + count) applied
    before, after = np.array(t["image"]), np.array(t["image"])
    before[t["addrs"][:first]] = t["outs"][:first]
    after[t["addrs"][:first + count]] = t["outs"][:first + count]
    assert np.array_equal(out[:8], logup.reference_image_root(before)) and np.array_equal(out[8:16], logup.reference_image_root(after))
    # lo and hi by the plain formula over the table
    half = 1 << (t["h"] - 1)
    lo = half + (int(t["addrs"][first - 1]) >> 4) + 1 if first else half
    hi = half + (int(t["addrs"][first + count - 1]) >> 4) + 1 if count else lo
    assert [G.decode(out[16]), G.decode(out[17])] == [lo, hi]
    # the live blocks are the dirty nodes, the root is the last slot, and nothing lies past the blocks
    B = t["B"]
    ids = [G.decode(w) for w in data[G.D_ID, 0:BLOCK * B:BLOCK]]
    assert ids[-1] == 1 and sum(i > 0 for i in ids) == tc.node_count(t["h"], t["addrs"][first:first + count]) and len(set(i for i in ids if i)) == sum(i > 0 for i in ids)
    pairs = [i for i in ids if i >= half]
    assert pairs == sorted(pairs) == ids[:len(pairs)]
    assert not data[:, BLOCK * B:].any() and not code[3:G.C_LAST, BLOCK * B:].any()


def test_the_code_group_does_not_depend_on_the_image():
    code = tc.code_of(10, 500)
    B = 16
    assert code[G.C_IN_ROW].tolist().count(ONE) == B and int(np.flatnonzero(code[G.C_LAST_TOP])[0]) == BLOCK * B - 1
    assert np.flatnonzero(code[G.C_LAST]).tolist() == [(1 << 10) - 500 - 1]
    assert [G.decode(w) for w in code[G.C_GPOW, 1:30]] == [1 << k for k in range(29)] and code[G.C_GEND, 29] == ONE


# ---- the plan ----
@pytest.mark.parametrize("s,what", tc.CASES, ids=lambda v: str(v))
def test_the_plan_covers_the_table_once_in_parts_that_fit(s, what):
    po2, zk, W = s
    t = tc.table(po2, zk, W, what)
    a, plan, h, B = t["addrs"], t["plan"], t["h"], t["B"]
    assert plan[0][0] == 0 and sum(c for _, c in plan) == len(a) and all(plan[p + 1][0] == plan[p][0] + plan[p][1] for p in range(len(plan) - 1))
    for p, (first, count) in enumerate(plan):
        assert count > 0 or len(a) == 0
        assert tc.node_count(h, a[first:first + count]) <= B
        if first:
            assert a[first - 1] >> 4 != a[first] >> 4, "a part splits a pair of leaves"
        if p + 1 < len(plan):                                                  # one more pair would overflow
            nxt = plan[p + 1][0]
            more = nxt + int(np.sum(a[nxt:] >> 4 == a[nxt] >> 4))
            assert tc.node_count(h, a[first:more]) > B


def test_the_plan_of_every_word_of_512_is_one_part_where_p2_page_takes_26():
    assert G.parts(12, 200, 512, list(range(512))) == [(0, 512)]
    assert len(p2_page.parts(12, 200, 512, 512)) == 26
    assert len(tc.table(*tc.H6, "all")["plan"]) > 1 and len(tc.table(*tc.H12, "random")["plan"]) > 1 and len(tc.table(*tc.H8, "all")["plan"]) > 1


@pytest.mark.parametrize("s,what", tc.CASES, ids=lambda v: str(v))
def test_the_plan_in_c_is_the_plan_in_python(s, what):
    from zeth_amd import hal as zhal
    po2, zk, W = s
    assert zhal.page_tree_plan(po2, zk, W, tc.table(po2, zk, W, what)["addrs"]) == tc.table(po2, zk, W, what)["plan"]


def test_the_plan_in_c_refuses_by_message():
    from zeth_amd import hal as zhal
    with pytest.raises(zhal.HalError, match=r"page_tree_plan: an image of 16 words has a single pair of leaves \(W > 16"):
        zhal.page_tree_plan(10, 500, 16, [3])
    with pytest.raises(zhal.HalError, match=r"page_tree_plan: no room for the h 12 nodes of one path in 11 block slots \(po2 10, 680 zk_cycles\)"):
        zhal.page_tree_plan(10, 680, tc.H12[2], [0])
    with pytest.raises(zhal.HalError, match="page_tree_plan: row 1: address 3 does not follow a smaller one"):
        zhal.page_tree_plan(10, 500, 64, [12, 3])
    with pytest.raises(zhal.HalError, match="page_tree_plan: row 0: address 64 does not follow"):
        zhal.page_tree_plan(10, 500, 64, [64])


def test_the_plan_and_the_reference_refuse_what_cannot_be_laid_out():
    with pytest.raises(ValueError, match="W > 16"):
        G.parts(10, 500, 16, [0])
    with pytest.raises(ValueError, match="no room for the h 12 nodes of one path in 11 block slots"):
        G.parts(10, 680, tc.H12[2], [0])
    t = tc.table(*tc.H5, 3)
    with pytest.raises(ValueError, match="exceed the 16 block slots"):
        G.reference_tree_part(*tc.H6, tc.table(*tc.H6, "all")["table"], tc.table(*tc.H6, "all")["image"], 0, 512)
    with pytest.raises(ValueError, match="splits the pair of leaves 0"):
        G.reference_tree_part(*tc.H5, tc.table(*tc.H5, "one_pair")["table"], tc.table(*tc.H5, "one_pair")["image"], 0, 1)
    with pytest.raises(ValueError, match=r"the part \[0, 0\) of a table of 3 rows"):
        G.reference_tree_part(*tc.H5, t["table"], t["image"], 0, 0)


# ---- tampered witnesses: the lowest failing row and its family, or the key the bus names ----
def _bump(w):
    return np.uint32((int(w) + ONE) % P)


def _enc(x):
    return np.uint32(x % P * ONE % P)


@pytest.fixture(scope="module")
def tamper_case():
    po2, zk, W = tc.H5                                                        # B 67, h 5; `random`: 40 addresses, one part
    t = tc.table(po2, zk, W, "random")
    assert len(t["plan"]) == 1
    data, out, code = tc.part(po2, zk, W, "random")
    ids = [G.decode(w) for w in data[G.D_ID, 0:BLOCK * t["B"]:BLOCK]]
    return {"po2": po2, "zk": zk, "h": t["h"], "B": t["B"], "data": data, "out": out, "code": code, "ids": ids, "pairs": sum(i >= 16 for i in ids)}


def _tampered(c, data=None, out=None):
    return _first_failure(c["po2"], c["zk"], c["code"], c["data"] if data is None else data, c["out"] if out is None else out)


def _bus(c, data):
    return logup.reference_bus(tc.args(), c["po2"], c["zk"], c["code"], data)


def _block(slot):
    return slice(BLOCK * slot, BLOCK * (slot + 1))


def _best_order_columns(data, slot, lo):
    """lo, gbit, gacc of a pair block the best a prover can: lo as the constraints force it, the low 29 bits of (id - lo) mod P"""
    r0 = BLOCK * slot
    g = ((G.decode(data[G.D_ID, r0]) - lo) % P) & ((1 << G.GAP_BITS) - 1)
    data[G.D_LO, _block(slot)] = _enc(lo)
    data[G.D_GBIT:, _block(slot)] = 0
    for k in range(1, G.GAP_BITS + 1):
        data[G.D_GBIT, r0 + k] = ONE * ((g >> (k - 1)) & 1)
        data[G.D_GACC, r0 + k] = _enc(g % (1 << k))
    data[G.D_GACC, r0 + BLOCK - 1] = _enc(g)


def test_tamper_an_inner_node_flagged_leaf(tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    m = c["pairs"]
    assert 1 < c["ids"][m] < 16, "the first block behind the pair blocks is an inner node"
    data[G.D_LEAF, _block(m)] = ONE
    data[G.D_DL:G.D_DR + 1, _block(m)] = 0                                      # leaf dl = leaf dr = 0 holds; it comes right after a pair block
    assert _tampered(c, data) == (BLOCK * m + G.GAP_BITS, "order")            # its id is below lo: no gap of 29 bits reaches it


def test_tamper_pair_ids_out_of_order(tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    data[:, _block(0)], data[:, _block(1)] = c["data"][:, _block(1)], c["data"][:, _block(0)]
    _best_order_columns(data, 0, 16)
    _best_order_columns(data, 1, c["ids"][1] + 1)
    assert _bus(c, data)["row"] == -1, "the two blocks only changed places: the bus still balances"
    assert _tampered(c, data) == (BLOCK + G.GAP_BITS, "order")


def test_tamper_a_pair_id_repeated(tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    data[:, _block(1)] = c["data"][:, _block(0)]
    _best_order_columns(data, 1, c["ids"][0] + 1)
    assert _tampered(c, data) == (BLOCK + G.GAP_BITS, "order")


def test_tamper_a_clean_sibling_that_differs_between_old_and_new(tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    slot = next(s for s, i in enumerate(c["ids"]) if 1 <= i < 16 and data[G.D_DR, BLOCK * s] == 0)
    r = BLOCK * slot
    data[G.D_SN + 8 + 3, r] = _bump(data[G.D_SN + 8 + 3, r])
    assert _tampered(c, data) == (r, "in_row")


def test_tamper_a_child_digest_changed_on_the_consumer(tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    slot = next(s for s, i in enumerate(c["ids"]) if 1 <= i < 16 and data[G.D_DL, BLOCK * s] == ONE)
    r = BLOCK * slot
    data[G.D_SO + 1, r] = _bump(data[G.D_SO + 1, r])                            # X[1]: the tuple of tag 1
    assert _tampered(c, data) == (r + 1, "rounds")                            # the row only sees its own permutation go wrong ...
    bus = _bus(c, data)                                                       # ... the bus names the child whose digest nobody produced
    assert bus["row"] >= 0 and bus["tag"] == 1 and bus["key"][0] == 2 * c["ids"][slot] and bus["unbalanced_keys"] == 2
    assert f"key (tag 1; {2 * c['ids'][slot]}, " in logup.describe_bus(bus, tc.args())
    with pytest.raises(logup.ReferenceError, match="the bus does not balance"):
        logup.reference_accumulate(tc.args(), c["po2"], c["zk"], c["code"], data, _mix())


def test_tamper_a_second_producer_of_one_id(tamper_case):
    c, data = tamper_case, tamper_case["data"].copy()
    dead = c["ids"].index(0)
    data[:, _block(dead)] = c["data"][:, _block(0)]                            # pair block 0 once more, where a dead block was
    data[G.D_LEAF, _block(dead)] = 0                                           # (not as a pair block: `order` would object first)
    bus = _bus(c, data)
    assert bus["row"] >= 0 and bus["key"][0] == c["ids"][0] and bus["net"] == P - 1 and bus["unbalanced_keys"] == 6
    line = logup.describe_bus(bus, tc.args())
    assert f"key (tag 1; {c['ids'][0]}, " in line and "has 2 entries" in line


def test_tamper_the_root_block(tamper_case):
    c = tamper_case
    root = _block(c["B"] - 1)
    last = BLOCK * c["B"] - 1
    data = c["data"].copy()
    data[G.D_ID, root], data[G.D_IDL, root], data[G.D_IDR, root] = _enc(2), _enc(4), _enc(5)
    assert _tampered(c, data) == (last, "root")
    data = c["data"].copy()
    data[G.D_UP, root] = ONE
    assert _tampered(c, data) == (last, "root")
    out = c["out"].copy()
    out[9] = _bump(out[9])
    assert _tampered(c, out=out) == (last, "root")


def test_tamper_lo_and_hi_in_out(tamper_case):
    c = tamper_case
    out = c["out"].copy()
    out[16] = _bump(out[16])
    assert _tampered(c, out=out) == (0, "order")
    out = c["out"].copy()
    out[17] = _bump(out[17])
    assert _tampered(c, out=out) == (BLOCK * c["B"] - 1, "order")


# ---- the chain verifier's linking rules, on the reference's outputs ----
def _fmt(r):
    return " ".join(f"{int(w):08x}" for w in r)


@pytest.fixture(scope="module")
def chain():
    t = tc.table(*tc.H6, "all")
    return [tc.part(*tc.H6, "all", p)[1] for p in range(len(t["plan"]))], t


def test_the_chain_links_and_gives_both_roots_and_hi(chain):
    from zeth_amd.prover import link_page_tree_chain
    outs, t = chain
    assert len(outs) >= 3
    root_before, root_after = logup.reference_image_root(t["image"]), logup.reference_image_root(t["image_after"])
    for given in (root_before, None):
        got = link_page_tree_chain(outs, 6, given)
        assert np.array_equal(got[0], root_before) and np.array_equal(got[1], root_after) and got[2] == 64
    got = link_page_tree_chain(outs[:1], 6)                                    # a chain may stop early: it says where it stopped
    assert np.array_equal(got[1], outs[1][:8]) and got[2] == G.decode(outs[1][16])
    empty = tc.part(*tc.H6, 0)[1]
    assert link_page_tree_chain([empty], 6)[2] == 32 and np.array_equal(empty[:8], empty[8:16])


def test_the_chain_verifier_refuses_one_message_per_cause(chain):
    from zeth_amd.hal import HalError
    from zeth_amd.prover import link_page_tree_chain, verify_page_tree_chain
    outs, t = chain
    with pytest.raises(HalError, match=f"part 0 starts at lo {G.decode(outs[1][16])}, not 2\\^5 = 32"):
        link_page_tree_chain([outs[1], outs[0]] + outs[2:], 6)                 # two parts swapped
    with pytest.raises(HalError, match=f"part 1 opens root {_fmt(outs[2][:8])}, but part 0 left root {_fmt(outs[0][8:16])}"):
        link_page_tree_chain([outs[0]] + outs[2:], 6)                          # a part dropped: the roots do not link
    forged = outs[1].copy()
    forged[16] = outs[2][16]
    with pytest.raises(HalError, match=f"part 1 starts at lo {G.decode(outs[2][16])}, but part 0 left hi {G.decode(outs[0][17])}"):
        link_page_tree_chain([outs[0], forged] + outs[2:], 6)                  # the roots link, lo / hi do not
    with pytest.raises(HalError, match="part 0 starts at lo 32, not 2\\^6 = 64"):
        link_page_tree_chain(outs, 7)                                          # told another h
    with pytest.raises(HalError, match=f"part 0 opens root {_fmt(outs[0][:8])}, not root_before {_fmt(outs[0][8:16])}"):
        link_page_tree_chain(outs, 6, outs[0][8:16])
    high = tc.part(*tc.H6, 0)[1].copy()
    high[17] = np.uint32(65 * ONE % P)
    with pytest.raises(HalError, match="the last part leaves hi 65, above 2\\^6 = 64"):
        link_page_tree_chain([high], 6)
    high[17] = np.uint32(((1 << 29) + 1) * ONE % P)
    with pytest.raises(HalError, match="part 0: hi 536870913 is above 2\\^29"):
        link_page_tree_chain([high], 6)
    with pytest.raises(HalError, match="no receipt"):
        link_page_tree_chain([], 6)
    with pytest.raises(HalError, match="no receipt"):
        verify_page_tree_chain([], np.zeros(8, np.uint32), 6)


# ---- the same tables under P2-PAGE-ordered ----
@pytest.mark.parametrize("s", [tc.H3, tc.H5], ids=str)
@pytest.mark.parametrize("what", [1, 3, "first_last", "adjacent", "one_pair"], ids=str)
def test_the_roots_are_p2_page_ordereds(s, what):
    _, _, W = s
    t = tc.table(*s, what)
    _, ordered = p2_page_ordered.reference_ordered_part(12, 200, W, t["table"], t["image"], 0)      # h <= 5 at (12, 200): 25 slots and more
    first, last = tc.part(*s, what, 0)[1], tc.part(*s, what, len(t["plan"]) - 1)[1]
    assert np.array_equal(first[:8], ordered[:8]) and np.array_equal(last[8:16], ordered[8:16])
