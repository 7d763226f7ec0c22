"""zkh_check_rows (csrc/check_rows.hip) against its definition's host twin (circuits/check.py reference_check_rows), word for word: the
per-row buffer, (row, step), failing_rows and value.  Random constraint systems with nested conditions, Fp4 values and backs up to 3 on
traces where nearly every row fails and on traces where the failing step varies by row; single planted failures on lane, wave and
workgroup edges; two failures whose lower row carries the higher step; windows; the forged SYN-LOOKUP witnesses through
SegmentProver.seal_host_witness(check=True); SYN-HEAVY small and KECCAK-F; every error path.

Mutants built as library variants and run against this file (never committed), and the cases each one failed: the interpreter's stride
of 4 left in the tap read — all 37 cases; F as "first in chain order" instead of the minimum — test_hand_built_descriptions alone
(hand_two_failures: the random circuits do not tell the two apart); the condition test dropped from and_cond — 29 cases: every
witness whose constraints sit under selectors (syn_tiny, SYN-LOOKUP, SYN-HEAVY, KECCAK-F, the seals), hand_cond, random seeds 4, 7, 10
and 11; the wave minimum keyed by the step before the row — 12 cases: the four of
test_the_lower_row_is_named_although_its_step_is_higher, test_hand_built_descriptions, random seeds 2, 3, 4, 5, 7, 10 and 11."""
import re

import numpy as np
import pytest

from args_gpu import seal_host as _seal_host
import check_rows_cases as cases
import zko
from zeth_amd.circuits import check, logup, syn_heavy, syn_random
from zeth_amd.circuits.desc import Circuit, P
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
NONE = check.NONE
NOISE = 0x0C05


def _upload(hal, *arrays):
    return [hal.copy_from("trace", a) for a in arrays]


def _agree(hal, desc, po2, accum, code, data, out, mix, row_lo=0, row_hi=None, circuit=None):
    """the library's answer = the reference's, word for word; -> (row, step, failing_rows)"""
    c = circuit if circuit is not None else hal.load_circuit(desc, jit=False)
    want = check.reference_check_rows(desc, po2, accum, code, data, out, mix, row_lo, row_hi)
    row, step, count = check.first_failure(want)
    got = hal.check_rows(c, po2, *_upload(hal, accum, code, data), out, mix, row_lo, row_hi, per_row=True)
    assert np.array_equal(got["per_row"], want)
    assert (got["row"], got["step"], got["failing_rows"]) == (row, step, count)
    value = check.reference_value(desc, po2, accum, code, data, out, mix, row, step) if row >= 0 else (0, 0, 0, 0)
    assert got["value"] == value
    bare = hal.check_rows(c, po2, *_upload(hal, accum, code, data), out, mix, row_lo, row_hi)          # without the per-row buffer
    assert bare["per_row"] is None and {k: bare[k] for k in ("row", "step", "failing_rows", "value")} == {k: got[k] for k in ("row", "step", "failing_rows", "value")}
    return row, step, count


# ---- random constraint systems ----
def _random_traces(c, seed, po2):
    """-> (dense, sparse): every word uniform over all 32-bit words (a raw word >= P is its residue), so that nearly every row fails
    on its lowest steps; zeros with a few percent of random cells, raw P among them, so that the failing step varies by row"""
    rng = np.random.default_rng(1000 * po2 + seed)
    n = 1 << po2
    dense = [rng.integers(0, 1 << 32, size=w * n, dtype=np.uint64).astype(np.uint32) for w in c.group_sizes]
    sparse = []
    for w in c.group_sizes:
        t = np.zeros(w * n, dtype=np.uint32)
        hit = rng.random(w * n) < 0.03
        t[hit] = rng.integers(1, P + 1, size=int(hit.sum()), dtype=np.uint64).astype(np.uint32)
        sparse.append(t)
    return dense, sparse


@pytest.mark.parametrize("seed", range(12))
def test_random_circuits_word_for_word(hal, seed):
    desc = syn_random.random_circuit(seed)
    c = Circuit.parse(desc)
    circuit = hal.load_circuit(desc, jit=False)
    for po2 in (8, 10):
        n = 1 << po2
        out, mix = cases.mix_words(seed, c.global_sizes[0]), cases.mix_words(seed + 50, c.global_sizes[1])
        dense, sparse = _random_traces(c, seed, po2)
        _row, _step, count = _agree(hal, desc, po2, *dense, out, mix, circuit=circuit)
        assert count > n // 2
        # seeds 2, 3, 4, 5, 7, 10 and 11 name 3 to 14 different steps over the rows of the sparse trace; in the others a constraint on
        # a bare constant is the lowest failing step of every row (rows that pass: the planted failures below)
        for o, m in ((out, mix), (np.zeros_like(out), np.zeros_like(mix))):
            _agree(hal, desc, po2, *sparse, o, m, circuit=circuit)


# ---- planted failures on an otherwise honest syn_tiny witness, po2 9 ----
PO2, ZK = 9, 40
N, A = 1 << PO2, (1 << PO2) - ZK


def _planted(rows_cols):
    """the honest witness with data[col][row] ^= 1 for every (row, col); the first blinding row takes the `active` code flag instead"""
    desc, accum, code, data, out, mix = cases.syn_tiny_witness(PO2, ZK)
    code, data = np.array(code), np.array(data)
    for row, col in rows_cols:
        if row >= A:
            code[0 * N + row] = cases.ONE                # a blinding row that claims to be active: its noise meets the constraints
        else:
            data[col * N + row] ^= 1
    return desc, accum, code, data, out, mix


def test_an_honest_witness_is_clean(hal):
    desc, accum, code, data, out, mix = cases.syn_tiny_witness(PO2, ZK)
    assert _agree(hal, desc, PO2, accum, code, data, out, mix) == (-1, NONE, 0)


@pytest.mark.parametrize("row", [0, 63, 64, 127, 128, N - 1, A])
def test_one_planted_failure_on_lane_wave_and_workgroup_edges(hal, row):
    desc, accum, code, data, out, mix = _planted([(row, 3)])
    if row == N - 1:                                     # the last row is a blinding row as well
        assert row >= A
    got_row, step, count = _agree(hal, desc, PO2, accum, code, data, out, mix)
    assert got_row == row and count == 1
    # windows: the row alone, everything below it (clean), everything above it (clean)
    circuit = hal.load_circuit(desc, jit=False)
    assert _agree(hal, desc, PO2, accum, code, data, out, mix, row, row + 1, circuit) == (row, step, 1)
    if row > 0:
        assert _agree(hal, desc, PO2, accum, code, data, out, mix, 0, row, circuit) == (-1, NONE, 0)
    if row + 1 < N:
        assert _agree(hal, desc, PO2, accum, code, data, out, mix, row + 1, N, circuit) == (-1, NONE, 0)


@pytest.mark.parametrize("low,high", [(70, 75), (63, 64), (100, 300), (127, 128)])
def test_the_lower_row_is_named_although_its_step_is_higher(hal, low, high):
    """data 9 breaks step 31, data 0 breaks step 13: same wave, neighbouring waves, two workgroups"""
    desc, accum, code, data, out, mix = _planted([(low, 9), (high, 0)])
    want = check.reference_check_rows(desc, PO2, accum, code, data, out, mix)
    assert want[low] > want[high] != NONE
    row, step, count = _agree(hal, desc, PO2, accum, code, data, out, mix)
    assert (row, step, count) == (low, int(want[low]), 2)
    assert _agree(hal, desc, PO2, accum, code, data, out, mix, low + 1, N) == (high, int(want[high]), 1)


# ---- F on the hand-built descriptions, on the device ----
def test_hand_built_descriptions(hal):
    po2 = cases.HAND_PO2
    n = 1 << po2
    desc, step = cases.hand_cond()
    assert _agree(hal, desc, po2, *cases.hand_trace(d0=7, d1=[0, 1, 0, 2, 0, P - 1, 0, 0]), cases.HAND_OUT, cases.HAND_MIX) == (1, step, 3)
    desc, step = cases.hand_cond(ext_cond=True)
    assert _agree(hal, desc, po2, *cases.hand_trace(d0=7, d1=[0, 0, 0, 2, 0, 0, 0, 4]), cases.HAND_OUT, cases.HAND_MIX) == (3, step, 2)
    desc, step, _conds = cases.hand_nested()
    assert _agree(hal, desc, po2, *cases.hand_trace(d0=[1, 2, 3, 4, 0, 6, 7, 8], d1=[0, 0, 1, 1, 5, 0, 9, 3], d2=[0, 1, 0, 1, 6, 2, 0, 4]),
                  cases.HAND_OUT, cases.HAND_MIX) == (3, step, 2)
    desc, step = cases.hand_ext_value()
    accum, code, data = cases.hand_trace(d0=[0, 0, 0, 9, 0, 0, P - 1, 0])
    assert _agree(hal, desc, po2, accum, code, data, cases.HAND_OUT, cases.HAND_MIX) == (3, step, 2)
    got = hal.check_rows(hal.load_circuit(desc, jit=False), po2, *_upload(hal, accum, code, data), cases.HAND_OUT, cases.HAND_MIX)
    assert got["value"] == (0, 0, 0, 9)                                        # non-zero in component 3 alone
    desc, low, high = cases.hand_two_failures()
    assert _agree(hal, desc, po2, *cases.hand_trace(d0=[0, 0, 1, 0, 0, 0, 0, 0], d1=[0, 1, 1, 0, 0, 0, 0, 0]), cases.HAND_OUT, cases.HAND_MIX) == (1, high, 2)
    assert _agree(hal, desc, po2, *cases.hand_trace(d0=1, d1=1), cases.HAND_OUT, cases.HAND_MIX) == (0, low, n)
    desc, step = cases.hand_cond()                                             # raw P is zero, raw P + 1 is not
    accum, code, data = cases.hand_trace(d0=7, d1=0)
    data = np.array(data)
    data[1 * n + 2], data[1 * n + 3] = P, P + 1
    assert _agree(hal, desc, po2, accum, code, data, cases.HAND_OUT, cases.HAND_MIX) == (3, step, 1)
    desc, step = cases.hand_back3()                                            # rows 0..2 read rows n - 3 .. n - 1
    d1 = np.array([11, 12, 13, 14, 15, 16, 17, 18])
    accum, code, data = cases.hand_trace(d0=np.roll(d1, 3), d1=d1)
    assert _agree(hal, desc, po2, accum, code, data, cases.HAND_OUT, cases.HAND_MIX) == (-1, NONE, 0)
    for r in range(3):
        bad = np.array(data)
        bad[1 * n + (n - 3 + r)] = cases.enc(99)
        assert _agree(hal, desc, po2, accum, code, bad, cases.HAND_OUT, cases.HAND_MIX) == (r, step, 1)
    desc, step = cases.hand_globals()                                          # globals are read as residues, too
    codev = [1, 2, 3, 4, 5, 6, 7, 8]
    accum, code, data = cases.hand_trace(d0=[(7 * v) * pow(4, -1, P) % P for v in codev], code=codev)
    out = np.array(cases.HAND_OUT)
    out[1] = int(out[1]) + P
    assert _agree(hal, desc, po2, accum, code, data, out, cases.HAND_MIX) == (-1, NONE, 0)
    assert _agree(hal, desc, po2, accum, code, data, out, cases.enc([5, 6, 8, 8])) == (0, step, n)


# ---- the forged SYN-LOOKUP witnesses ----
@pytest.mark.parametrize("kind", cases.FORGERIES)
def test_forged_syn_lookup_witnesses_word_for_word(hal, kind):
    po2, zk = 10, 300
    variant, accum, code, data, out, mix, want_row, _columns = cases.lookup_forgery(kind, po2, zk)
    row, _step, _count = _agree(hal, cases.lookup_circuit(variant)[0], po2, accum, code, data, out, mix)
    assert row == want_row


@pytest.mark.parametrize("kind", ["swap_sorted_rows", "relink_row", "misread_row"])
def test_seal_host_witness_with_check_names_the_row_before_any_seal(hal, oracle, kind):
    """under the flag-free blob (nothing derived: the host's columns are what is sealed) the forged witness passes the accumulate — its
    bus balances — and only the constraints object"""
    po2, zk = 10, 300
    variant, _accum, code, forged, out, _mix, row, _columns = cases.lookup_forgery(kind, po2, zk)
    desc, blob = cases.lookup_circuit(variant)
    plain = logup.Arguments.parse(blob).plain().blob()
    honest_data = cases.lookup_witness(variant, po2, zk)[1]
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    prover = SegmentProver(hal, desc, arguments=plain)
    # the step and what it reads do not depend on the mix the seal draws
    f = check.reference_check_rows(desc, po2, _accum, code, forged, out, _mix)
    step = int(f[row])
    want = f"witness: row {row} fails constraint step {step} (value "
    with pytest.raises(HalError, match=re.escape(want)) as err:
        _seal_host(hal, prover, seg, code, forged, out, check=True)
    msg = str(err.value)
    assert f"; reads {check.describe_reads(desc, step)}; " in msg and re.search(r"; \d+ rows? fail\)$", msg), msg
    # check=False: today's behaviour — the seal is spent, and the refusal (or a seal no verifier accepts) names nothing
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    try:
        receipt = _seal_host(hal, prover, seg, code, forged, out)
    except HalError as e:
        assert "witness: row" not in str(e) and "DEEP quotient has a non-zero remainder" in str(e)
    else:
        assert oc.verify(receipt.seal, root) is not None
    # the honest witness: check=True changes nothing, byte for byte
    a = _seal_host(hal, prover, seg, code, honest_data, out, check=True)
    b = _seal_host(hal, prover, seg, code, honest_data, out)
    assert np.array_equal(a.seal, b.seal)
    assert oc.verify(a.seal, root) is None


def test_check_witness_is_clean_on_a_built_in_witness_and_seal_with_accum_takes_check(hal):
    from zeth_amd.circuits import syn_air
    prover = SegmentProver(hal, syn_air.syn_tiny())
    seg = Segment(index=0, po2=PO2, zk_cycles=ZK, noise_seed=NOISE)
    code, data, out = prover.witgen(seg)
    a = prover.seal_with_accum(seg, code, data, out, prover.syn_accumulate(seg, data), check=True)
    b = prover.seal_with_accum(seg, code, data, out, prover.syn_accumulate(seg, data))
    assert np.array_equal(a.seal, b.seal)
    broken = data.to_vec()
    broken[3 * N + 77] ^= 1
    data.write(broken)
    with pytest.raises(HalError, match=r"witness: row 77 fails constraint step 19 \(value \d+; reads data\[3\]@0, data\[4\]@0, data\[5\]@0; 1 rows fail\)"):
        prover.seal_with_accum(seg, code, data, out, prover.syn_accumulate(seg, data), check=True)


# ---- further circuits ----
def test_syn_heavy_small_fp4_constraints(hal):
    desc = syn_heavy.syn_heavy_small()
    c = Circuit.parse(desc)
    po2 = 8
    n = 1 << po2
    rng = np.random.default_rng(5)
    traces = [rng.integers(0, P, size=w * n, dtype=np.uint64).astype(np.uint32) for w in c.group_sizes]
    out, mix = cases.mix_words(1, c.global_sizes[0]), cases.mix_words(2, c.global_sizes[1])
    row, step, count = _agree(hal, desc, po2, *traces, out, mix)
    assert row == 0 and count > n // 2
    # an honest witness of the built-in generator: clean, and one broken product cell is found
    prover = SegmentProver(hal, desc)
    seg = Segment(index=0, po2=po2, zk_cycles=40, noise_seed=NOISE)
    code, data, out = prover.witgen(seg)
    mix = cases.mix_words(3, c.global_sizes[1])
    accum = prover.syn_accumulate(seg, data)(mix)
    host = [b.to_vec() for b in (accum, code, data)]
    assert _agree(hal, desc, po2, *host, out, mix) == (-1, NONE, 0)
    host[2][2 * n + 65] ^= 1
    assert _agree(hal, desc, po2, *host, out, mix)[0] == 65


def test_keccak_f(hal):
    desc, accum, code, data, out, claimed, mix, bind_row = cases.keccak_witness()
    circuit = hal.load_circuit(desc, jit=False)
    assert _agree(hal, desc, 8, accum, code, data, out, mix, circuit=circuit) == (-1, NONE, 0)
    assert _agree(hal, desc, 8, accum, code, data, claimed, mix, circuit=circuit)[::2] == (bind_row, 1)
    flipped = np.array(data)
    flipped[1000 * 256 + 30] ^= cases.ONE                                      # one state bit of row 30
    assert _agree(hal, desc, 8, accum, code, flipped, out, mix, circuit=circuit)[0] in (29, 30)


# ---- error paths ----
def test_error_paths(hal):
    desc, accum, code, data, out, mix = cases.syn_tiny_witness(PO2, ZK)
    c = hal.load_circuit(desc, jit=False)
    da, dc, dd = _upload(hal, accum, code, data)
    assert hal.check_rows(c, PO2, da, dc, dd, out, mix)["row"] == -1
    for lo, hi in ((0, 0), (5, 5), (7, 3), (0, N + 1), (N, N + 1), (N, N)):
        with pytest.raises(HalError, match=r"check_rows: window \[\d+, \d+\) is empty or outside \[0, 512\]"):
            hal.check_rows(c, PO2, da, dc, dd, out, mix, lo, hi)
    with pytest.raises(HalError, match="check_rows: group 2 has 5632 words, expected 2816"):
        hal.check_rows(c, PO2 - 1, da.slice(0, accum.size // 2), dc.slice(0, code.size // 2), dd, out, mix)
    with pytest.raises(HalError, match="check_rows: group 0 has"):
        hal.check_rows(c, PO2, dc, dc, dd, out, mix)
    with pytest.raises(HalError, match="check_rows: po2 0 out of range"):
        hal.check_rows(c, 0, da, dc, dd, out, mix)
    import ctypes as C
    from zeth_amd import hal as zhal
    groups = (C.c_void_p * 3)(da.h, dc.h, dd.h)
    res = zhal.CheckRowsResult()
    out_words, mix_words = np.array(out), np.array(mix)
    o, m = zhal._ptr(out_words), zhal._ptr(mix_words)
    with pytest.raises(HalError, match="check_rows: expected 3 register groups"):
        zhal._check(zhal._lib.zkh_check_rows(hal.ctx, c.h, PO2, groups, 2, o, m, 0, N, None, C.byref(res)))
    with pytest.raises(HalError, match="check_rows: the per-row buffer has 100 words, expected 512"):
        zhal._check(zhal._lib.zkh_check_rows(hal.ctx, c.h, PO2, groups, 3, o, m, 0, N, hal.alloc_elem("short", 100).h, C.byref(res)))
    with pytest.raises(HalError, match="check_rows: the globals"):
        zhal._check(zhal._lib.zkh_check_rows(hal.ctx, c.h, PO2, groups, 3, None, m, 0, N, None, C.byref(res)))
    with pytest.raises(HalError, match="check_rows: null argument"):
        zhal._check(zhal._lib.zkh_check_rows(hal.ctx, c.h, PO2, groups, 3, o, m, 0, N, None, None))
    # a circuit loaded on another context, or on none
    other = zhal.HipHal(0)
    try:
        foreign = other.load_circuit(desc, jit=False)
        with pytest.raises(HalError, match="check_rows: circuit was not loaded on this context"):
            hal.check_rows(foreign, PO2, da, dc, dd, out, mix)
        h, foreign.h = foreign.h, None                   # released while its context lives
        zhal._lib.zkh_circuit_destroy(h)
    finally:
        other.close()
    with pytest.raises(HalError, match="check_rows: circuit was not loaded on this context"):
        hal.check_rows(zhal.HostCircuit(desc), PO2, da, dc, dd, out, mix)
    # more live values than the interpreter's LDS holds: refused in words, like eval_check's interpreter
    big = hal.load_circuit(cases.live_ext_desc(400), jit=False)
    n = 1 << cases.HAND_PO2
    traces = _upload(hal, *cases.hand_trace(d0=1))
    with pytest.raises(HalError, match="check_rows: the step list has more live values than the interpreter's LDS holds"):
        hal.check_rows(big, cases.HAND_PO2, *traces, cases.HAND_OUT, cases.HAND_MIX)
    # ... while one that needs more than 64 KiB but fits is served (the dynamic-LDS attribute)
    desc40 = cases.live_ext_desc(40)                                           # 40 x 16 bytes x 128 lanes = 80 KiB
    accum, code, data = cases.hand_trace(d0=[0, 1, 0, 0, 0, 0, 0, 2])
    assert _agree(hal, desc40, cases.HAND_PO2, accum, code, data, cases.HAND_OUT, cases.HAND_MIX)[::2] == (1, 2)
