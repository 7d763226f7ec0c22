"""One rule for a witness from the accumulate to the seal (DESIGN.md §2 ARGUMENTS): a trace cell is read as its residue, raw % P, and raw
words >= P are legal.  For every entry point that takes a caller's trace the result on a trace T' equals the result on T = T' % P: what
zkh_accumulate writes and refuses, what zkh_derive_multiplicities counts, and the seal that SegmentProver.seal_host_witness and a session
with host traces make of it, byte for byte.  T' comes from raw_words.raise_words (30 % of the words raised by P or 2 P, the edge words
P, 2 P, R1 + P and 0xFFFFFFFF planted where the witness allows), and every test asserts that of the traces it uploads.

Mutants these cases are meant to catch:
  * a selector or multiplicity negated as P - word: the sign -1 terms of test_accumulate_equals_the_reference_on_raised_traces (R1 + P
    negates to 0: the term drops out, the bus does not balance);
  * a product of two raw words, or of a raw numerator with a denominator, past the Montgomery bound: the terms with a raised selector and
    a raised multiplicity on one row, and the three-term columns, of the same test;
  * a denominator compared or folded from raw tuple words: test_a_denominator_that_vanishes_through_a_raised_word_is_refused;
  * the trace committed as the caller left it: every case of test_the_seal_is_a_function_of_the_residues (the inverse NTT's butterflies
    take reduced words: the seal of T' differs, and no verifier accepts it); po2 13 runs the strided pass next to the low-12 kernel;
  * the reduction on the path of device-made traces: test_the_built_in_path_launches_what_it_launched."""
import re

import numpy as np
import pytest

import check_bus_cases as bus_cases
import raw_words as rw
import zko
from args_gpu import circuit as _circuit, image_buf as _image, profiled, seal_host as _seal_host, upload as _upload
from conftest import rand_fp
from test_logup_derive_gpu import _random_case
from test_logup_gpu import _noise_fn, _random_arguments, _traces
from test_logup_pages_gpu import _paged
from zeth_amd.circuits import logup, syn_air, syn_lookup
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = rw.P
NOISE = 0x0C07
SHARE = 0.3
TINY = syn_lookup.TINY


def _raised(rng, a, n):
    """a flat trace of n-row columns with 30 % of its words raised, active and blinding rows alike -> flat"""
    return rw.raise_words(np.asarray(a).reshape(-1, n), rng, SHARE).reshape(-1)


def _accumulate(hal, c, po2, zk, code, data, mix, k):
    dcode, ddata = _upload(hal, code, data)
    acc = hal.alloc_elem("accum", 4 * k << po2)
    hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)
    return acc.to_vec()


# ---- 1. zkh_accumulate against reference_accumulate ----
# A = 219: no multiple of a wave; 1013; 1078: one full block of ARGS_THREADS * ARGS_BATCH rows and a partial one; 2102
ACC_GRID = [(8, 37, 3), (10, 11, 2), (11, 970, 7), (12, 1994, 4)]


def test_accumulate_equals_the_reference_on_raised_traces(hal):
    seen = set()
    for po2, zk, k in ACC_GRID:
        n, A = 1 << po2, (1 << po2) - zk
        desc, blob = _random_arguments(po2 * 100 + k, k)
        c = _circuit(hal, desc, blob)
        args = logup.Arguments.parse(blob)
        rng = np.random.default_rng(po2 + 17 * k)
        code, data = _traces(rng, 6, 10, n)
        code, data = rw.plant(code.reshape(-1, n), rng, rows=np.arange(A)).reshape(-1), rw.plant(data.reshape(-1, n), rng, rows=np.arange(A)).reshape(-1)
        mix = rand_fp(rng, 12)
        want, total = logup.reference_accumulate(args, po2, zk, code, data, mix, noise=_noise_fn(NOISE)(po2, zk))
        assert total == [0, 0, 0, 0]
        code2, data2 = _raised(rng, code, n), _raised(rng, data, n)
        rw.assert_raised(code2.reshape(-1, n), code.reshape(-1, n), rows=np.arange(A))
        rw.assert_raised(data2.reshape(-1, n), data.reshape(-1, n), rows=np.arange(A))
        assert rw.planted(code2.reshape(-1, n)[:, :A]) == rw.planted(data2.reshape(-1, n)[:, :A]) == set(rw.EDGE_WORDS)
        # what the argument set and the raised cells exercise
        groups = {1: code2.reshape(-1, n)[:, :A] >= P, 2: data2.reshape(-1, n)[:, :A] >= P}
        for t in args.terms:
            sel = groups[1][t.sel] if t.sel is not None else np.zeros(A, dtype=bool)
            mult = groups[t.mult[0]][t.mult[1]] if t.mult is not None else np.zeros(A, dtype=bool)
            seen |= {"neg_sel"} if t.sign == -1 and sel.any() else set()
            seen |= {"neg_mult"} if t.sign == -1 and mult.any() else set()
            seen |= {"sel_and_mult_on_a_row"} if (sel & mult).any() else set()
        seen |= {"three_terms"} if any(len(ts) == 3 for ts in args.by_column()) else set()
        got = _accumulate(hal, c, po2, zk, code2, data2, mix, k)
        assert (got < P).all(), f"po2 {po2}: {int((got >= P).sum())} accum words are not reduced"
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"po2 {po2}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n} (A = {A})"
    assert seen == {"neg_sel", "neg_mult", "sel_and_mult_on_a_row", "three_terms"}, seen


def test_a_denominator_that_vanishes_through_a_raised_word_is_refused(hal):
    po2, zk = 10, 200
    n = 1 << po2
    desc, blob = syn_lookup.syn_lookup_tiny()
    c = _circuit(hal, desc, blob)
    args = logup.Arguments.parse(blob)
    code, data, _out = syn_lookup.witness(TINY, po2, zk, seed=7)
    rng = np.random.default_rng(3)
    mix = rand_fp(rng, 8)
    mix[4:8] = [rw.R1, 0, 0, 0]                                              # beta = 1, alpha = limb 0 of word 0 on row 0
    mix[0:4] = [data.reshape(-1, n)[2, 0], 0, 0, 0]
    code2, data2 = _raised(rng, code, n), _raised(rng, data, n).reshape(-1, n)
    data2[2, 0] = data.reshape(-1, n)[2, 0] + np.uint32(P)                   # the tuple word of the vanishing denominator, raised
    data2 = data2.reshape(-1)
    rw.assert_raised(code2, code)
    rw.assert_raised(data2, data)
    with pytest.raises(logup.ReferenceError) as ref:
        logup.reference_accumulate(args, po2, zk, code2, data2, mix)
    row, col, term = (int(x) for x in re.fullmatch(r"denominator vanishes at row (\d+), accum column (\d+), term (\d+)", str(ref.value)).groups())
    assert (row, col, term) == (0, 0, 0)
    dcode, ddata = _upload(hal, code2, data2)
    acc = hal.alloc_elem("accum", 16 << po2)
    with pytest.raises(HalError, match=re.escape(f"a denominator vanishes at row {row}, accum column {col} (Fp columns {4 * col}..{4 * col + 3}), term {term} of the column")):
        hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)
    assert not acc.to_vec().any()                                            # no accum is left behind
    mix[0] = (int(mix[0]) + 1) % P                                           # another alpha: the same raised witness is accepted
    hal.accumulate(c, po2, zk, NOISE, dcode, ddata, mix, acc)
    want, _ = logup.reference_accumulate(args, po2, zk, code, data, mix, noise=_noise_fn(NOISE)(po2, zk))
    assert np.array_equal(acc.to_vec(), want)


# ---- 2. zkh_accumulate and zkh_check_bus agree ----
def test_accumulate_accepts_the_raw_words_witness_of_check_bus(hal):
    desc, blob, po2, zk, code, data = bus_cases.hand("raw_words")[:6]
    n = 1 << po2
    args = logup.Arguments.parse(blob)
    c = _circuit(hal, desc, blob)
    assert (code >= P).any() and (data >= P).any()                           # the witness as check_bus_cases makes it: + P on every third row
    dcode, ddata = _upload(hal, code, data)
    assert hal.check_bus(c, po2, zk, dcode, ddata)["term"] == -1             # zkh_check_bus calls it balanced
    mix = rand_fp(np.random.default_rng(2), 8)
    reduced = _accumulate(hal, c, po2, zk, code % P, data % P, mix, args.k)
    want, total = logup.reference_accumulate(args, po2, zk, code % P, data % P, mix, noise=_noise_fn(NOISE)(po2, zk))
    assert total == [0, 0, 0, 0] and np.array_equal(reduced, want)
    assert np.array_equal(_accumulate(hal, c, po2, zk, code, data, mix, args.k), reduced)
    rng = np.random.default_rng(9)                                           # ... and the same residues raised the suite's way
    code2, data2 = _raised(rng, code % P, n), _raised(rng, data % P, n)
    rw.assert_raised(code2, code % P)
    rw.assert_raised(data2, data % P)
    assert np.array_equal(_accumulate(hal, c, po2, zk, code2, data2, mix, args.k), reduced)


# ---- 3. zkh_derive_multiplicities against reference_multiplicities ----
# the shapes of test_logup_derive_gpu's random test at po2 8 and 12 (at most 4096 distinct keys: the LDS count) and its smallest shape
# with more (po2 13, 6198 keys: the global count)
@pytest.mark.parametrize("po2,zk,big", [(8, 37, False), (12, 1994, False), (13, 1994, True)])
def test_multiplicities_of_raised_traces(hal, po2, zk, big):
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data = _random_case(po2 * 7 + zk, po2, zk, big)
    c = _circuit(hal, desc, blob)
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(po2)
    reduced = logup.reference_multiplicities(args, po2, zk, code, data)
    code2, data2 = _raised(rng, code, n), _raised(rng, data, n)
    rw.assert_raised(code2, code)
    rw.assert_raised(data2, data)
    want = logup.reference_multiplicities(args, po2, zk, code2, data2)
    dcode, ddata = _upload(hal, code2, data2)
    prof = profiled(hal, lambda: hal.derive_multiplicities(c, po2, zk, dcode, ddata))
    assert ("derive_count_global" if big else "derive_count_lds") in prof, set(prof)
    got = ddata.to_vec()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"po2 {po2}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
    m = sorted(t.mult[1] for t in args.terms if t.derive)
    g, untouched = got.reshape(-1, n), data2.reshape(-1, n).copy()
    assert np.array_equal(g[m, :A], reduced.reshape(-1, n)[m, :A]) and g[m, :A].any()      # the counts of the reduced trace, word for word
    untouched[m, :A] = g[m, :A]
    assert np.array_equal(g, untouched) and np.array_equal(dcode.to_vec(), code2)          # nothing else touched


# ---- 4. the seal is a function of the residues ----
def _lookup_case(po2, zk, flags, full_kw, bare_kw):
    desc, blob = syn_lookup.build_syn_lookup(TINY, **flags)
    code, _full, out = syn_lookup.witness(TINY, po2, zk, seed=po2, **full_kw)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, **{**full_kw, **bare_kw})
    return desc, blob, code, bare, out


SEAL_CASES = {
    "plain": lambda: (10, 200) + _lookup_case(10, 200, {}, {}, {}),                                          # host-made columns
    "derived_sorted": lambda: (12, 1994) + _lookup_case(12, 1994, dict(derive=True, sort=True), {}, dict(sort=False, count=False)),
    "reads": lambda: (12, 1994) + _lookup_case(12, 1994, dict(derive=True, limbs=True, link=True, reads=True), dict(addr_range=300, link=True, reads=True),
                                                dict(count=False, limbs=False, link=False)),
}


def _seal_both(hal, oracle, desc, blob, seg, code, data, out, rng):
    """seal the reduced witness and its raised twin with one Segment -> (the receipt, the raised twin's): the same seal, accepted by both
    verifiers under the control root of the reduced code"""
    n = 1 << seg.po2
    code2, data2 = _raised(rng, code, n), _raised(rng, data, n)
    rw.assert_raised(code2, code)
    rw.assert_raised(data2, data)
    A = n - seg.zk_cycles
    assert (data2.reshape(-1, n)[:, :A] >= P).any() and (data2.reshape(-1, n)[:, A:] >= P).any()             # active rows and blinding rows
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, data, out)
    twin = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code2, data2, out)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(seg.po2, code)
    dcode, _ = _upload(hal, code, data)
    assert np.array_equal(SegmentProver(hal, desc, arguments=blob).code_root(dcode, seg.po2), root)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None
    assert np.array_equal(twin.seal, receipt.seal), f"{int((twin.seal != receipt.seal).sum())} of {receipt.seal.size} seal words differ"
    twin.verify(desc, root)
    assert oc.verify(twin.seal, root) is None
    return receipt, twin


@pytest.mark.parametrize("name", list(SEAL_CASES))
def test_the_seal_is_a_function_of_the_residues(hal, oracle, name):
    po2, zk, desc, blob, code, bare, out = SEAL_CASES[name]()
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    _seal_both(hal, oracle, desc, blob, seg, code, bare, out, np.random.default_rng(po2))


# po2 13: the inverse NTT runs its strided pass as well as the low-12 kernel; SYN-LOOKUP-paged's clocks (3 limbs of 4 bits) hold A < 4096
@pytest.mark.parametrize("po2,zk,W,page_out", [(8, 40, 64, False), (13, 4200, 300, True)])
def test_the_seal_of_a_paging_circuit_is_a_function_of_the_residues(hal, oracle, po2, zk, W, page_out):
    desc, blob, _plain, image, code, _full, bare, out = _paged(po2, zk, W, po2)
    rng = np.random.default_rng(po2)
    image2 = rw.raise_words(image, rng, SHARE)                               # the image raised as pages_cases' `big` does, and by 2 P
    rw.assert_raised(image2, image)
    images = (_image(hal, image), _image(hal, image2))
    trees = [hal.image_commit(im) for im in images] if page_out else [None, None]
    if page_out:
        assert np.array_equal(hal.image_root(trees[0]), hal.image_root(trees[1]))
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    n = 1 << po2
    code2, data2 = _raised(rng, code, n), _raised(rng, bare, n)
    rw.assert_raised(code2, code)
    rw.assert_raised(data2, bare)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out, image=images[0], page_out=page_out, tree=trees[0])
    twin = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code2, data2, out, image=images[1], page_out=page_out, tree=trees[1])
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    assert np.array_equal(twin.seal, receipt.seal), f"{int((twin.seal != receipt.seal).sum())} of {receipt.seal.size} seal words differ"
    for r in (receipt, twin):
        r.verify(desc, root)
        assert oc.verify(r.seal, root) is None
    if page_out:                                                             # the page-out leaves the same memory and the same commitment
        after, after2 = images[0].to_vec(), images[1].to_vec()
        assert not np.array_equal(after, image) and np.array_equal(after2 % P, after % P)
        assert np.array_equal(hal.image_root(trees[0]), logup.reference_image_root(after))
        assert np.array_equal(hal.image_root(trees[1]), hal.image_root(trees[0]))


def test_the_seal_of_a_built_in_accum_circuit_is_a_function_of_the_residues(hal, oracle):
    po2 = 12
    n = 1 << po2
    desc = syn_air.syn_small()
    prover = SegmentProver(hal, desc)
    seg = Segment(index=0, po2=po2, seed=0x5EED0001, noise_seed=NOISE)
    dcode, ddata, out = prover.witgen(seg)
    code, data = dcode.to_vec(), ddata.to_vec()
    device = prover.seal(seg, dcode, ddata, out)
    rng = np.random.default_rng(po2)
    code2, data2 = _raised(rng, code, n), _raised(rng, data, n)
    rw.assert_raised(code2, code)
    rw.assert_raised(data2, data)
    receipt = _seal_host(hal, prover, seg, code, data, out)
    twin = _seal_host(hal, prover, seg, code2, data2, out)
    assert np.array_equal(receipt.seal, device.seal)
    assert np.array_equal(twin.seal, receipt.seal), f"{int((twin.seal != receipt.seal).sum())} of {receipt.seal.size} seal words differ"
    oc = zko.OracleCircuit(oracle, desc)
    root = prover.control_root(po2, seg.zk_cycles)
    assert np.array_equal(root, oc.control_root(po2, seg.zk_cycles))
    twin.verify(desc, root)
    assert oc.verify(twin.seal, root) is None


def test_reduce_elem_is_w_mod_p_on_any_view(hal):
    """zkh_reduce_elem takes 16 bytes a lane: views that start 0 .. 3 words past a 16-byte boundary and end anywhere (head and tail of up
    to three words, no body, one body lane, more than one workgroup), every 32-bit word, nothing outside the view touched"""
    rng = np.random.default_rng(11)
    words = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    words[rng.choice(words.size, 70, replace=False)] = np.repeat(np.array([0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 0xFFFFFFFF], dtype=np.uint32), 10)
    for off in (0, 1, 2, 3, 6):
        for count in (1, 2, 3, 4, 5, 7, 8, 11, 1021, 1024, 1027, 4099):
            buf = hal.copy_from("words", words)
            hal.reduce_elem(buf.slice(off, count))
            want = words.copy()
            want[off:off + count] %= np.uint32(P)
            assert np.array_equal(buf.to_vec(), want), (off, count)


# ---- 5. sessions ----
def test_a_session_seals_raised_host_traces_as_the_reduced_ones(hal, oracle):
    from zeth_amd.host import Session
    po2 = 12
    n = 1 << po2
    desc, blob = syn_lookup.syn_lookup_tiny_derived()
    segs = [Segment(index=i, po2=po2, noise_seed=NOISE + i) for i in range(2)]
    traces = [syn_lookup.witness(TINY, po2, s.zk_cycles, seed=40 + i, count=False) for i, s in enumerate(segs)]
    rng = np.random.default_rng(5)
    raised = [(_raised(rng, code, n), _raised(rng, data, n), out) for code, data, out in traces]
    for (code, data, _), (code2, data2, _) in zip(traces, raised):
        rw.assert_raised(code2, code)
        rw.assert_raised(data2, data)
    sess = Session(desc, lanes_per_device=1)
    sess.set_arguments(blob)
    comp, _, _ = sess.prove(segs, host_traces=traces, verify=True)
    comp2, _, _ = sess.prove(segs, host_traces=raised)
    sess.close()
    oc = zko.OracleCircuit(oracle, desc)
    for (code, _, _), r, r2 in zip(traces, comp.segments, comp2.segments):
        assert np.array_equal(r2.seal, r.seal), f"{int((r2.seal != r.seal).sum())} of {r.seal.size} seal words differ"
        assert oc.verify(r2.seal, oc.root_of_code(po2, code)) is None


# ---- 6. the built-in path gained nothing ----
# the profile scopes of one prove_segment of SYN-SMALL at po2 12 with device witgen, as the commit before the reduction ran them
BUILT_IN_SCOPES = ["batch_bit_reverse", "batch_evaluate_any", "batch_expand_into_evaluate_ntt:k_ntt_pass", "batch_interpolate_ntt:k_ntt_pass",
                   "batch_interpolate_ntt_from:k_ntt_low12", "combos_divide", "combos_prepare", "eltwise_copy_elem", "eltwise_sum_extelem", "eval_check",
                   "fri_fold", "hash_fold_tail", "hash_fold_wide", "hash_rows", "merkle_open", "mix_poly_coeffs", "prefix_products", "syn_accum_store",
                   "syn_accum_terms", "syn_code"]


def test_the_built_in_path_launches_what_it_launched(hal):
    prover = SegmentProver(hal, syn_air.syn_small())
    seg = Segment(index=0, po2=12, seed=0x5EED0000, noise_seed=NOISE)
    prover.prove_segment(seg)                                                # tables and code objects loaded
    prof = profiled(hal, lambda: prover.prove_segment(seg))
    assert sorted(prof) == BUILT_IN_SCOPES
    assert "reduce_elem" not in prof
