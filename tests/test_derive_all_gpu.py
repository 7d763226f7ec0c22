"""zkh_derive_all on the GPU (csrc/arguments.hip: the stage table): one call takes the bare witness of SYN-LOOKUP TINY — everything the
library derives left out — to the host-made full witness, word for word, and to what the guarded stage calls in their order leave,
on three circuits that each hold one dependency between stages: the multiplicities count the derived limbs; the ORDER record reads
the sorted copy; the link limbs are counted.  Sizes: (po2 8, zk 40), A = 216 active rows, no multiple of a wave, and (po2 12, zk 1994).
Under a blob that derives nothing the call is a no-op.  A refusal is the refusing stage's own, string for string, and leaves `data`
as the stages before it left it.

Mutants these cases catch (never committed): a stage table with the multiplicities first fails all six chain cases (the limbs it
counts are still zero: the 16 words of the multiplicity column differ) and the refusals of columns, links and multiplicities (what
the call leaves is not what the stages before the refusing one leave); one with the columns before the sorted copies fails both
sizes of the circuit with the ORDER record (it reads a copy that is not there yet) and the refusals of sorted and columns."""
import numpy as np
import pytest

from args_gpu import circuit as _circuit, enc as _enc, upload as _upload
from conftest import rand_fp
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError

pytestmark = pytest.mark.gpu
TINY = syn_lookup.TINY
SIZES = [(8, 40), (12, 1994)]
STAGES = ("sorted", "columns", "links", "multiplicities")
# build_syn_lookup's switches, the witness generator's for the full witness and for the bare one
CIRCUITS = {
    "limbs_counted": (dict(derive=True, sort=True, limbs=True), dict(), dict(sort=False, count=False, limbs=False)),
    "order_reads_sorted": (dict(derive=True, sort=True, limbs=True, order=True), dict(order=True),
                           dict(sort=False, count=False, limbs=False, order=False)),
    "link_limbs_counted": (dict(derive=True, limbs=True, link=True, reads=True), dict(link=True, reads=True),
                           dict(count=False, limbs=False, link=False, reads=True)),
}


def _stage_calls(hal, c, upto=None):
    """the guarded stage calls in their order, those before `upto` (None: all)"""
    return [getattr(hal, "derive_" + s) for s in STAGES[:STAGES.index(upto) if upto else None] if getattr(c, "derives_" + s)()]


@pytest.mark.parametrize("po2,zk", SIZES)
@pytest.mark.parametrize("name", CIRCUITS)
def test_one_call_makes_the_full_witness_from_the_bare_one(hal, name, po2, zk):
    flags, full_kw, bare_kw = CIRCUITS[name]
    desc, blob = syn_lookup.build_syn_lookup(TINY, **flags)
    code, full, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=16, **full_kw)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=16, **bare_kw)
    assert not np.array_equal(bare, full)
    c = _circuit(hal, desc, blob)
    dcode, ddata = _upload(hal, code, bare)
    hal.derive_all(c, po2, zk, dcode, ddata)
    got = ddata.to_vec()
    bad = np.nonzero(got != full)[0]
    n = 1 << po2
    assert bad.size == 0, f"{bad.size} words differ from the host-made witness, first at column {bad[0] // n}, row {bad[0] % n}"
    calls = _stage_calls(hal, c)
    assert len(calls) == 3
    _, staged = _upload(hal, code, bare)
    for call in calls:
        call(c, po2, zk, dcode, staged)
    assert np.array_equal(got, staged.to_vec())
    assert np.array_equal(dcode.to_vec(), code)


def test_nothing_to_derive_is_a_no_op(hal):
    po2, zk = SIZES[0]
    flags, _, bare_kw = CIRCUITS["limbs_counted"]
    desc, blob = syn_lookup.build_syn_lookup(TINY, **flags)
    code, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=3, addr_range=16, **bare_kw)
    c = _circuit(hal, desc, logup.Arguments.parse(blob).plain().blob())
    assert c.has_arguments() and c.derived_data_columns() == []
    dcode, ddata = _upload(hal, code, bare)
    hal.derive_all(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), bare) and np.array_equal(dcode.to_vec(), code)


def _selected_sort_then_limbs(po2, zk):
    """the smallest circuit whose sort can refuse — SYN-LOOKUP's copies have no selector —: a copy of (data 0, data 1) under the code
    selector 3 sorted into (data 2, data 3), and a LIMBS record after it, data 4 into data 5 .. 8.  The selector is 2 on row 77."""
    rng = np.random.default_rng(po2)
    n, A = 1 << po2, (1 << po2) - zk
    code, data = rand_fp(rng, 4, n), rand_fp(rng, 9, n)
    code[3, :A] = _enc(rng.random(A) < 0.5)
    code[3, 77] = _enc(2)
    data[4, :A] = _enc(rng.integers(0, 1 << 16, A))
    b = logup.LogupBuilder((4, 4, 9), (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1, sel=3)
    b.term(0, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, tag=1, sel=3, sorted_from=0, sort_keys=[0])
    b.derive_limbs((GROUP_DATA, 4), [5, 6, 7, 8], 4)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code.reshape(-1), data.reshape(-1)


def _refusing(stage, po2, zk):
    """-> (desc, blob, code, data that `stage` refuses, what the stages before it leave: the host reference's chain up to there)"""
    n = 1 << po2
    if stage == "sorted":
        desc, blob, code, data = _selected_sort_then_limbs(po2, zk)
        return desc, blob, code, data, data
    if stage == "links":                                                     # a write flag that is no flag, under the read rule
        flags, _, bare_kw = CIRCUITS["link_limbs_counted"]
        edit = (syn_lookup.reads_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0], 100, 2)
    elif stage == "columns":                                                 # a word of 2^16 or more does not fit TINY's 4 limbs of 4 bits
        flags, _, bare_kw = CIRCUITS["limbs_counted"]
        edit = (1, 123, (1 << 16) + 5)
    else:                                                                    # host-made limbs, one of them outside the table
        flags, bare_kw, edit = dict(derive=True, sort=True), dict(sort=False, count=False), None
    desc, blob = syn_lookup.build_syn_lookup(TINY, **flags)
    code, data, _ = syn_lookup.witness(TINY, po2, zk, seed=9, addr_range=16, **bare_kw)
    if edit is None:
        data = syn_lookup.corrupt_limb(TINY, data, po2, row=123, word=1)
    else:
        col, row, value = edit
        data = data.copy()
        data.reshape(-1, n)[col, row] = _enc(value)
    args = logup.Arguments.parse(blob)
    before = logup.reference_columns(args, po2, zk, code, data) if stage == "links" else logup.reference_sorted(args, po2, zk, code, data)
    return desc, blob, code, data, before


@pytest.mark.parametrize("stage", STAGES)
def test_a_refusal_is_the_stage_s_own_and_earlier_stages_stay_written(hal, stage):
    po2, zk = SIZES[0]
    desc, blob, code, data, before = _refusing(stage, po2, zk)
    c = _circuit(hal, desc, blob)
    assert getattr(c, "derives_" + stage)()
    dcode, staged = _upload(hal, code, data)
    earlier = _stage_calls(hal, c, upto=stage)
    assert len(earlier) == (0 if stage == "sorted" else 1)
    for call in earlier:
        call(c, po2, zk, dcode, staged)
    assert np.array_equal(staged.to_vec(), before)
    with pytest.raises(HalError) as want:
        getattr(hal, "derive_" + stage)(c, po2, zk, dcode, staged)
    assert str(want.value).startswith(f"derive_{stage}: ") and "the witness is refused" in str(want.value)
    _, ddata = _upload(hal, code, data)
    with pytest.raises(HalError) as got:
        hal.derive_all(c, po2, zk, dcode, ddata)
    assert str(got.value) == str(want.value)
    assert np.array_equal(ddata.to_vec(), before)
