"""zkh_check_bus (csrc/bus.hip) against its definition's host twin (circuits/logup.py reference_bus), field for field: the scalar
fields, the per-term table and the line describe_bus makes of them.  Honest SYN-LOOKUP witnesses of every variant after their derives
on the device; the forged witnesses of the logup suites; hand-built pairs for the report order, the representative, residues, weights
and zero-padding; rows that fall onto one slot, onto distinct slots and across wave and workgroup edges; the table that stays and the
table that grows; purity; SegmentProver.check_bus and seal_host_witness(check=True); every refusal.

Mutants built as library variants and run against this file (never committed), and the cases each one failed: integer instead of
residue comparison in the scan — test_hand_built_pairs[sum_of_p] alone; the report ordered by (row, term) — test_hand_built_pairs
[report_order], test_forged_witnesses_field_for_field[sorted_value_multi] and test_growth; no zero-padding in the key — all 55 cases;
the wave combining dropping the last lane of a group — 41 cases: every SYN-LOOKUP witness, sum_of_p, few_keys, below_a_wave, the
growth, purity and prover cases; a growth that keeps the old key count — the six cases whose table grows (multi_sorted at the three
sizes, sorted_value_multi, unsorted_multi, test_growth)."""
import ctypes as C
import re

import numpy as np
import pytest

from args_gpu import circuit as _circuit, seal_host as _seal_host
import check_bus_cases as cases
import zko
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
NOISE = 0x0B05


def _agree(hal, case, circuit=None):
    """the library's answer = the reference's, with and without the per-term table; -> the reference's dict"""
    desc, blob, po2, zk, code, data = case[:6]
    c = circuit if circuit is not None else _circuit(hal, desc, blob)
    want = cases.reference(case)
    dc, dd = hal.copy_from("code", code), hal.copy_from("data", data)
    got = hal.check_bus(c, po2, zk, dc, dd, per_term=True)
    cases.same(got, want)
    args = logup.Arguments.parse(blob)
    assert logup.describe_bus(got, args) == logup.describe_bus(want, args)
    bare = hal.check_bus(c, po2, zk, dc, dd)
    assert bare.pop("per_term") is None and bare == {k: v for k, v in got.items() if k != "per_term"}
    return want


# ---- 1. honest witnesses, after their derives on the device ----
@pytest.mark.parametrize("variant", sorted(cases.VARIANTS))
@pytest.mark.parametrize("po2,zk", cases.SIZES)
def test_honest_witnesses_after_their_derives(hal, variant, po2, zk):
    desc, blob, po2, zk, code, data, uploaded = cases.honest(variant, po2, zk)
    c = _circuit(hal, desc, blob)
    dc, dd = hal.copy_from("code", code), hal.copy_from("data", uploaded)
    for derives, derive in ((c.derives_sorted, hal.derive_sorted), (c.derives_columns, hal.derive_columns), (c.derives_links, hal.derive_links),
                            (c.derives_multiplicities, hal.derive_multiplicities)):
        if derives():
            derive(c, po2, zk, dc, dd)
    assert np.array_equal(dd.to_vec(), data)
    want = cases.reference((desc, blob, po2, zk, code, data))
    got = hal.check_bus(c, po2, zk, dc, dd, per_term=True)
    cases.same(got, want)
    assert (got["term"], got["row"], got["unbalanced_keys"]) == (-1, -1, 0) and got["distinct_keys"] == want["distinct_keys"] > 0


# ---- 2. the forged witnesses ----
@pytest.mark.parametrize("kind", cases.FORGERIES)
def test_forged_witnesses_field_for_field(hal, kind):
    want = _agree(hal, cases.forgery(kind))
    assert (want["unbalanced_keys"] > 0) == (kind not in cases.BALANCED)


@pytest.mark.parametrize("variant", ["derived", "ordered", "linked", "reads"])
def test_a_witness_before_its_derives(hal, variant):
    desc, blob, po2, zk, code, _data, uploaded = cases.honest(variant, 10, 300)
    assert _agree(hal, (desc, blob, po2, zk, code, uploaded))["unbalanced_keys"] > 0


# ---- 3 .. 7. the hand-built pairs: report order, representative, residues, weights, padding ----
@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_built_pairs(hal, name):
    want = _agree(hal, cases.hand(name))
    term, row, key, net, unbalanced, distinct = cases.HAND[name]
    assert (want["term"], want["row"], want["key"], want["net"], want["unbalanced_keys"], want["distinct_keys"]) == (term, row, key, net, unbalanced, distinct)


# ---- 8. contention and lanes ----
@pytest.mark.parametrize("name", cases.CONTENTION)
def test_contention_and_lane_edges(hal, name):
    want = _agree(hal, cases.contention(name))
    if name == "one_key":
        assert (want["distinct_keys"], want["unbalanced_keys"]) == (1, 0)
    if name == "one_row":
        assert (want["term"], want["row"], want["net"], want["slots"]) == (0, 0, 1, 64)


# ---- 9. the table that stays and the table that grows ----
def test_growth(hal):
    start = logup.bus_slots(724, 0)
    tiny = _agree(hal, cases.honest("plain", 10, 300)[:6])
    multi = _agree(hal, cases.honest("multi_sorted", 10, 300)[:6])
    assert tiny["distinct_keys"] <= start // 2 < multi["distinct_keys"]
    assert tiny["slots"] == start and multi["slots"] == 4 * start
    grown_and_forged = _agree(hal, cases.forgery("sorted_value_multi"))                    # an answer found in a table that grew
    assert grown_and_forged["slots"] > start and grown_and_forged["unbalanced_keys"] == 2


# ---- 10. determinism and purity ----
def test_two_calls_agree_and_the_traces_are_not_written(hal):
    desc, blob, po2, zk, code, data = cases.forgery("wrong_pval")
    c = _circuit(hal, desc, blob)
    dc, dd = hal.copy_from("code", code), hal.copy_from("data", data)
    a = hal.check_bus(c, po2, zk, dc, dd, per_term=True)
    b = hal.check_bus(c, po2, zk, dc, dd, per_term=True)
    cases.same(a, b)
    assert a["unbalanced_keys"] == 2
    assert dc.to_vec().tobytes() == code.tobytes() and dd.to_vec().tobytes() == data.tobytes()


# ---- 11. the prover ----
@pytest.mark.parametrize("kind", ["corrupt_limb", "wrong_pval"])
def test_seal_host_witness_with_check_names_the_key(hal, oracle, kind):
    """under the flag-free blob (nothing derived: the host's columns are what is sealed) the forged witness reaches the accumulate"""
    desc, blob, po2, zk, code, forged = cases.forgery(kind)
    args = logup.Arguments.parse(blob).plain()
    plain = args.blob()
    honest = cases.honest("plain" if kind == "corrupt_limb" else "linked", po2, zk)[5]
    out = np.zeros(4, dtype=np.uint32)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    prover = SegmentProver(hal, desc, arguments=plain)
    line = logup.describe_bus(logup.reference_bus(args, po2, zk, code, forged), args)
    assert line.startswith("bus: key (tag ")
    with pytest.raises(HalError) as unchecked:
        _seal_host(hal, prover, seg, code, forged, out)
    today = str(unchecked.value)
    assert re.fullmatch(r"accumulate: the bus does not balance: total \(\d+, \d+, \d+, \d+\) over the \d+ accum columns, not zero: the witness "
                        r"is refused", today)
    with pytest.raises(HalError) as checked:
        _seal_host(hal, prover, seg, code, forged, out, check=True)
    assert str(checked.value) == today + "; " + line
    # the same line without any seal
    dc, dd = hal.copy_from("code", code), hal.copy_from("data", forged)
    with pytest.raises(HalError) as alone:
        prover.check_bus(seg, dc, dd)
    assert str(alone.value) == line
    # the honest witness: check_bus is quiet, and check=True changes no byte of the seal
    prover.check_bus(seg, dc, hal.copy_from("data", honest))
    a = _seal_host(hal, prover, seg, code, honest, out, check=True)
    b = _seal_host(hal, prover, seg, code, honest, out)
    assert np.array_equal(a.seal, b.seal)
    oc = zko.OracleCircuit(oracle, desc)
    assert oc.verify(a.seal, oc.root_of_code(po2, code)) is None


# ---- 12. refusals: host-side argument checks that return before any launch ----
def test_refusals(hal):
    desc, blob, po2, zk, code, data = cases.hand("balanced")
    c = _circuit(hal, desc, blob)
    dc, dd = hal.copy_from("code", code), hal.copy_from("data", data)
    assert hal.check_bus(c, po2, zk, dc, dd)["row"] == -1
    bare = hal.load_circuit(desc, jit=False)
    with pytest.raises(HalError, match=r"check_bus: the circuit has no arguments \(zkh_circuit_set_arguments\)"):
        hal.check_bus(bare, po2, zk, dc, dd)
    with pytest.raises(HalError, match="check_bus: the raw code trace is required"):
        hal.check_bus(c, po2, zk, None, dd)
    with pytest.raises(HalError, match="check_bus: buffer shape mismatch"):
        hal.check_bus(c, po2 - 1, zk, dc, dd)
    with pytest.raises(HalError, match="check_bus: buffer shape mismatch"):
        hal.check_bus(c, po2, zk, dd, dd)
    with pytest.raises(HalError, match="check_bus: po2 0 out of range"):
        hal.check_bus(c, 0, 0, dc, dd)
    with pytest.raises(HalError, match="check_bus: zk_cycles 512 leaves no active row"):
        hal.check_bus(c, po2, 1 << po2, dc, dd)
    res, terms = zhal.CheckBusResult(), (zhal.BusTerm * 3)()
    with pytest.raises(HalError, match="check_bus: the per-term array has 3 records, the arguments have 2 terms"):
        zhal._check(zhal._lib.zkh_check_bus(hal.ctx, c.h, po2, zk, dc.h, dd.h, terms, 3, C.byref(res)))
    with pytest.raises(HalError, match="check_bus: null argument"):
        zhal._check(zhal._lib.zkh_check_bus(hal.ctx, c.h, po2, zk, dc.h, dd.h, None, 0, None))
    other = zhal.HipHal(0)
    try:
        foreign = _circuit(other, desc, blob)
        with pytest.raises(HalError, match="check_bus: circuit was not loaded on this context"):
            hal.check_bus(foreign, po2, zk, dc, dd)
        h, foreign.h = foreign.h, None                   # released while its context lives
        zhal._lib.zkh_circuit_destroy(h)
    finally:
        other.close()
