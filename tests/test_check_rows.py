"""The row-by-row constraint check (zeth_amd/circuits/check.py: reference_check_rows, explain_step), the definition's host twin of
zkh_check_rows, against the independent oracle (oracle/recursion.c zko_check_rows, one fixed mix, a row only): all-NONE on the honest
witnesses of every circuit family, the oracle's row on every forgery with a named step that reads the forged column, and the failure
function F itself on hand-built descriptions.  No GPU."""
import numpy as np
import pytest

import check_rows_cases as cases
import zko
from zeth_amd.circuits import check, recursion as R
from zeth_amd.circuits.desc import GLOBAL_OUT, GROUP_CODE, GROUP_DATA, OP_AND_EQZ, Circuit, P

NONE = check.NONE


def _first(desc, po2, accum, code, data, out, mix):
    return check.first_failure(check.reference_check_rows(desc, po2, accum, code, data, out, mix))


# ---- honest witnesses: no row fails, and the oracle agrees ----
@pytest.mark.parametrize("po2,zk", cases.SIZES)
def test_honest_syn_tiny(oracle, po2, zk):
    desc, accum, code, data, out, mix = cases.syn_tiny_witness(po2, zk)
    assert zko.OracleCircuit(oracle, desc).check_rows(po2, accum, code, data, out, mix) == -1
    f = check.reference_check_rows(desc, po2, accum, code, data, out, mix)
    assert f.shape == (1 << po2,) and f.dtype == np.uint32 and (f == NONE).all()


@pytest.mark.parametrize("po2,zk", cases.SIZES)
@pytest.mark.parametrize("variant", cases.LOOKUP_VARIANTS)
def test_honest_syn_lookup(oracle, variant, po2, zk):
    desc, _blob = cases.lookup_circuit(variant)
    code, data, out, mix = cases.lookup_witness(variant, po2, zk)
    accum = cases.lookup_accum(variant, po2, zk, code, data, mix)
    assert zko.OracleCircuit(oracle, desc).check_rows(po2, accum, code, data, out, mix) == -1
    assert _first(desc, po2, accum, code, data, out, mix) == (-1, NONE, 0)


def test_honest_keccak_f_and_the_forged_input_claim(oracle):
    desc, accum, code, data, out, claimed, mix, bind_row = cases.keccak_witness()
    po2 = 8
    oc = zko.OracleCircuit(oracle, desc)
    assert oc.check_rows(po2, accum, code, data, out, mix) == -1
    assert _first(desc, po2, accum, code, data, out, mix) == (-1, NONE, 0)
    # the same output with another input claimed: the bind row objects, and the named step reads a claimed input limb
    assert oc.check_rows(po2, accum, code, data, claimed, mix) == bind_row
    row, step, count = _first(desc, po2, accum, code, data, claimed, mix)
    assert (row, count) == (bind_row, 1)
    e = check.explain_step(desc, step)
    assert Circuit.parse(desc).steps[step][0] == OP_AND_EQZ and len(e["globals"]) == 1 and e["globals"][0][0] == GLOBAL_OUT
    limb = e["globals"][0][1]
    assert 100 <= limb < 200 and claimed[limb] != out[limb] and not (claimed[100:limb] != out[100:limb]).any()     # the first forged limb
    assert all(g == GROUP_DATA and c < 64 and back == 0 for g, c, back in e["taps"])                              # lane 0 of the state
    assert len(e["conds"]) == 1                                                                                   # under the bind selector


def test_honest_recursion_and_a_forged_wire(oracle):
    desc, po2, accum, code, data, out, mix = cases.recursion_witness()
    rec = zko.OracleCircuit(oracle, desc)
    assert rec.check_rows(po2, accum, code, data, out, mix) == -1
    assert _first(desc, po2, accum, code, data, out, mix) == (-1, NONE, 0)
    n = 1 << po2
    gate = int(np.nonzero(code.reshape(R.WC, n)[R.C_QM])[0][0])                # a row of the general gate: it reads wire 3 (data 12..15)
    forged = np.array(data)
    forged[13 * n + gate] = (int(forged[13 * n + gate]) + 1) % P
    faccum = rec.rec_accum(po2, code, forged, mix, 50)                         # the copy argument's accum of the forged trace
    want = rec.check_rows(po2, faccum, code, forged, out, mix)
    row, step, _count = _first(desc, po2, faccum, code, forged, out, mix)
    assert want == gate and row == want
    assert any(g == GROUP_DATA and c == 13 for g, c, _back in check.explain_step(desc, step)["taps"])
    o2 = np.array(out)
    o2[3] = (int(o2[3]) + 1) % P                                               # the out globals are bound to the PUB row
    row, step, _count = _first(desc, po2, accum, code, data, o2, mix)
    assert row == rec.check_rows(po2, accum, code, data, o2, mix) >= 0
    assert (GLOBAL_OUT, 3) in check.explain_step(desc, step)["globals"]


# ---- forged SYN-LOOKUP witnesses: the oracle's row, and a named step that reads the forged column ----
@pytest.mark.parametrize("po2,zk", cases.SIZES)
@pytest.mark.parametrize("kind", cases.FORGERIES)
def test_forged_syn_lookup(oracle, kind, po2, zk):
    variant, accum, code, data, out, mix, want_row, columns = cases.lookup_forgery(kind, po2, zk)
    desc, _blob = cases.lookup_circuit(variant)
    assert zko.OracleCircuit(oracle, desc).check_rows(po2, accum, code, data, out, mix) == want_row
    f = check.reference_check_rows(desc, po2, accum, code, data, out, mix)
    row, step, count = check.first_failure(f)
    assert row == want_row and count >= 1
    assert Circuit.parse(desc).steps[step][0] == OP_AND_EQZ
    e = check.explain_step(desc, step)
    assert {(g, c) for g, c, _back in e["taps"]} & set(columns), (e, columns)
    assert len(e["conds"]) >= 1                                               # every constraint of SYN-LOOKUP sits under a selector
    value = check.reference_value(desc, po2, accum, code, data, out, mix, row, step)
    assert 0 < value[0] < P and value[1:] == (0, 0, 0)                        # a base-field constraint: zero upper components
    # the windows around the row
    assert check.first_failure(check.reference_check_rows(desc, po2, accum, code, data, out, mix, 0, row)) == (-1, NONE, 0)
    one = check.reference_check_rows(desc, po2, accum, code, data, out, mix, row, row + 1)
    assert one[row] == step and (np.delete(one, row) == NONE).all()


# ---- F itself ----
def _f(desc, accum, code, data, out=cases.HAND_OUT, mix=cases.HAND_MIX, **kw):
    return check.reference_check_rows(desc, cases.HAND_PO2, accum, code, data, out, mix, **kw)


def test_f_a_zero_condition_masks_its_inner_failure():
    desc, step = cases.hand_cond()
    d1 = [0, 1, 0, 2, 0, P - 1, 0, 0]                                          # the condition, row by row
    f = _f(desc, *cases.hand_trace(d0=7, d1=d1))                               # d0 != 0 on every row
    assert f.tolist() == [step if c else NONE for c in d1]
    assert (_f(desc, *cases.hand_trace(d0=0, d1=d1)) == NONE).all()            # nothing to mask
    e = check.explain_step(desc, step)
    assert e["taps"] == [(GROUP_DATA, 0, 0)] and e["conds"] == [len(Circuit.parse(desc).steps) - 1]


def test_f_nested_conditions():
    desc, step, conds = cases.hand_nested()
    d1, d2 = [0, 0, 1, 1, 5, 0, 9, 3], [0, 1, 0, 1, 6, 2, 0, 4]
    f = _f(desc, *cases.hand_trace(d0=[1, 2, 3, 4, 0, 6, 7, 8], d1=d1, d2=d2))
    assert f.tolist() == [NONE, NONE, NONE, step, NONE, NONE, NONE, step]      # both conditions non-zero and d0 != 0
    assert check.explain_step(desc, step)["conds"] == conds                    # outermost first


def test_f_an_fp4_value_is_nonzero_when_any_component_is():
    desc, step = cases.hand_ext_value()
    d0 = [0, 1, 0, 9, 0, 0, P - 1, 0]
    accum, code, data = cases.hand_trace(d0=d0)
    f = _f(desc, accum, code, data)
    assert f.tolist() == [step if v else NONE for v in d0]
    assert check.reference_value(desc, cases.HAND_PO2, accum, code, data, cases.HAND_OUT, cases.HAND_MIX, 3, step) == (0, 0, 0, 9)


def test_f_an_fp4_condition():
    desc, step = cases.hand_cond(ext_cond=True)
    d1 = [0, 1, 0, 2, 0, 0, 0, 4]
    assert _f(desc, *cases.hand_trace(d0=7, d1=d1)).tolist() == [step if c else NONE for c in d1]


def test_f_is_the_minimum_over_failing_steps_not_the_first_in_chain_order():
    desc, low, high = cases.hand_two_failures()
    assert low < high
    d0, d1 = [1, 0, 1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0]
    assert _f(desc, *cases.hand_trace(d0=d0, d1=d1)).tolist()[:4] == [low, high, low, NONE]


def test_f_a_raw_cell_p_is_zero():
    desc, step = cases.hand_cond()
    accum, code, data = cases.hand_trace(d0=7, d1=0)
    n = 1 << cases.HAND_PO2
    data = np.array(data)
    data[1 * n + 2] = P                                                        # the condition's raw word on row 2: the residue 0
    data[1 * n + 3] = P + 1                                                    # ... and on row 3 the residue 1
    data[0 * n + 5] = P                                                        # d0's raw word on row 5 (its condition is 0 anyway)
    assert _f(desc, accum, code, data).tolist() == [NONE, NONE, NONE, step, NONE, NONE, NONE, NONE]
    desc, step = cases.hand_ext_value()
    accum, code, data = cases.hand_trace(d0=1)
    data = np.array(data)
    data[0 * n + 4] = P
    assert _f(desc, accum, code, data).tolist() == [step] * 4 + [NONE] + [step] * 3


def test_f_a_tap_of_back_3_wraps_on_the_first_rows():
    desc, step = cases.hand_back3()
    n = 1 << cases.HAND_PO2
    d1 = np.array([11, 12, 13, 14, 15, 16, 17, 18])
    accum, code, data = cases.hand_trace(d0=np.roll(d1, 3), d1=d1)             # d0[r] = d1[r - 3 mod n]
    assert (_f(desc, accum, code, data) == NONE).all()
    for r in range(3):                                                         # rows 0..2 read rows n - 3 .. n - 1
        bad = np.array(data)
        bad[1 * n + (n - 3 + r)] = cases.enc(99)
        assert _f(desc, accum, code, bad).tolist() == [step if q == r else NONE for q in range(n)]
    assert check.explain_step(desc, step)["taps"] == [(GROUP_DATA, 0, 0), (GROUP_DATA, 1, 3)]


def test_f_globals_and_windows():
    desc, step = cases.hand_globals()
    code = [1, 2, 3, 4, 5, 6, 7, 8]
    d0 = [(7 * c) * pow(4, -1, P) % P for c in code]                           # d0 * out[1] = mix[2] * code: out[1] = 4, mix[2] = 7
    accum, code_t, data = cases.hand_trace(d0=d0, code=code)
    assert (_f(desc, accum, code_t, data) == NONE).all()
    out = np.array(cases.HAND_OUT)
    out[1] = int(out[1]) + P                                                   # a global word is read as its residue, too
    assert (_f(desc, accum, code_t, data, out=out) == NONE).all()
    assert (_f(desc, accum, code_t, data, mix=cases.enc([5, 6, 8, 8])) == step).all()
    assert _f(desc, accum, code_t, data, mix=cases.enc([5, 6, 8, 8]), row_lo=2, row_hi=5).tolist() == [NONE] * 2 + [step] * 3 + [NONE] * 3
    e = check.explain_step(desc, step)
    assert e["globals"] == [(0, 1), (1, 2)] and e["taps"] == [(GROUP_CODE, 0, 0), (GROUP_DATA, 0, 0)]
    assert check.describe_reads(desc, step) == "code[0]@0, data[0]@0, out[1], mix[2]"
    for lo, hi in ((0, 0), (3, 3), (5, 4), (0, 9), (-1, 4)):
        with pytest.raises(AssertionError, match="window"):
            _f(desc, accum, code_t, data, row_lo=lo, row_hi=hi)
    with pytest.raises(AssertionError, match="no and_eqz"):
        check.explain_step(desc, step - 1)
