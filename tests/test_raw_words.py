"""The host references are functions of the residues (DESIGN.md §2 ARGUMENTS: a trace cell is read as raw % P, raw words >= P are legal):
on a trace raised by raw_words.raise_words -- words up to 0xFFFFFFFF, which the `+ P` cases of the other suites never reach -- every
reference gives what it gives on the reduced trace.  Word for word where it computes a word; residue for residue on the cells a stage
defines as copies of a raw word (the sorted copies, prev_j, p_addr, p_in, p_out, p_time); a refusal with the same message."""
import numpy as np
import pytest

import check_bus_cases as bus_cases
import check_rows_cases as rows_cases
import pages_cases as pc
import raw_words as rw
from test_logup_derive_gpu import _random_case
from test_logup_gpu import _random_arguments, _traces
from zeth_amd.circuits import check, logup, syn_lookup

P = rw.P
TINY = syn_lookup.TINY
SHARE = 0.3


def _raised(rng, a, n, rows=None):
    """a flat trace of n-row columns, raised -> flat"""
    return rw.raise_words(np.asarray(a).reshape(-1, n), rng, SHARE, rows=rows).reshape(-1)


def _same_refusal(call, reduced, raised):
    with pytest.raises(logup.ReferenceError) as want:
        call(*reduced)
    with pytest.raises(logup.ReferenceError) as got:
        call(*raised)
    assert str(got.value) == str(want.value)
    return str(want.value)


def test_raise_words_plants_the_edge_words():
    rng = np.random.default_rng(1)
    a = rw.plant(rng.integers(0, P, (3, 64), dtype=np.uint64).astype(np.uint32), rng)
    out = rw.raise_words(a, rng, SHARE)
    assert rw.planted(out) == set(rw.EDGE_WORDS) and out.dtype == np.uint32 and out.shape == a.shape
    part = rw.raise_words(a, rng, SHARE, rows=np.arange(10, 40))
    assert np.array_equal(part[:, :10], a[:, :10]) and np.array_equal(part[:, 40:], a[:, 40:])
    with pytest.raises(AssertionError):
        rw.assert_raised(a, a)                                               # a reduced trace does not pass for a raised one


@pytest.mark.parametrize("po2,zk,k", [(8, 37, 3), (9, 100, 5), (10, 11, 2)])
def test_reference_accumulate(po2, zk, k):
    n = 1 << po2
    desc, blob = _random_arguments(po2 * 100 + k, k)
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(po2 + 17 * k)
    code, data = _traces(rng, 6, 10, n)
    code, data = rw.plant(code.reshape(-1, n), rng).reshape(-1), rw.plant(data.reshape(-1, n), rng).reshape(-1)
    mix = rng.integers(0, P, 12, dtype=np.uint64).astype(np.uint32)
    want, total = logup.reference_accumulate(args, po2, zk, code, data, mix)
    assert total == [0, 0, 0, 0]
    code2, data2 = _raised(rng, code, n), _raised(rng, data, n)
    assert rw.planted(code2) == rw.planted(data2) == set(rw.EDGE_WORDS)
    got, total2 = logup.reference_accumulate(args, po2, zk, code2, data2, mix)
    assert total2 == total and np.array_equal(got, want)


def test_reference_accumulate_refusals():
    po2, zk = 10, 200
    n = 1 << po2
    desc, blob = syn_lookup.syn_lookup_tiny()
    args = logup.Arguments.parse(blob)
    code, data, _out = syn_lookup.witness(TINY, po2, zk, seed=7)
    rng = np.random.default_rng(3)
    mix = rng.integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    bad = syn_lookup.corrupt_limb(TINY, data, po2, row=123, word=1)
    call = lambda c, d, m: logup.reference_accumulate(args, po2, zk, c, d, m)
    msg = _same_refusal(call, (code, bad, mix), (_raised(rng, code, n), _raised(rng, bad, n), mix))
    assert msg.startswith("the bus does not balance: total [")
    mix[4:8] = [rw.R1, 0, 0, 0]                                              # beta = 1, alpha = limb 0 of word 0 on row 0
    mix[0:4] = [data.reshape(-1, n)[2, 0], 0, 0, 0]
    raised = _raised(rng, data, n).reshape(-1, n)
    raised[2, 0] = data.reshape(-1, n)[2, 0] + np.uint32(P)                  # the vanishing denominator through a raised tuple word
    msg = _same_refusal(call, (code, data, mix), (_raised(rng, code, n), raised.reshape(-1), mix))
    assert msg == "denominator vanishes at row 0, accum column 0, term 0"


@pytest.mark.parametrize("po2,zk,big", [(8, 37, False), (9, 100, True)])
def test_reference_multiplicities(po2, zk, big):
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data = _random_case(po2 * 7 + zk, po2, zk, big)
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(po2)
    want = logup.reference_multiplicities(args, po2, zk, code, data)
    code2, data2 = _raised(rng, code, n), _raised(rng, data, n)
    got = logup.reference_multiplicities(args, po2, zk, code2, data2)
    m = sorted(t.mult[1] for t in args.terms if t.derive)
    g, w, d2 = got.reshape(-1, n), want.reshape(-1, n), data2.reshape(-1, n).copy()
    assert np.array_equal(g[m, :A], w[m, :A]) and w[m, :A].any()             # the derived columns word for word ...
    d2[m, :A] = g[m, :A]
    assert np.array_equal(g, d2)                                             # ... and nothing else touched


def test_reference_multiplicities_refusals():
    po2, zk = 10, 200
    n = 1 << po2
    desc, blob = syn_lookup.syn_lookup_tiny_derived()
    args = logup.Arguments.parse(blob)
    code, data, _out = syn_lookup.witness(TINY, po2, zk, seed=7, count=False)
    rng = np.random.default_rng(4)
    bad = syn_lookup.corrupt_limb(TINY, data, po2, row=123, word=1)
    call = lambda c, d: logup.reference_multiplicities(args, po2, zk, c, d)
    msg = _same_refusal(call, (code, bad), (_raised(rng, code, n), _raised(rng, bad, n)))
    assert "at row 123 has no table entry" in msg
    c2 = code.reshape(-1, n).copy()
    c2[5, 3] = rows_cases.enc(2)                                             # table selector 2 on row 3
    r2 = _raised(rng, c2, n).reshape(-1, n)
    r2[5, 3] = c2[5, 3] + np.uint32(P)
    msg = _same_refusal(call, (c2.reshape(-1), data), (r2.reshape(-1), _raised(rng, data, n)))
    assert "has selector 2 at row 3" in msg


def _derive_chain(args, po2, zk, code, data, image=None):
    """the stages in their order, as zkh_derive_all runs them"""
    data = logup.reference_sorted(args, po2, zk, code, data)
    data = logup.reference_columns(args, po2, zk, code, data)
    data = logup.reference_links(args, po2, zk, code, data, image=image)
    return logup.reference_multiplicities(args, po2, zk, code, data) if any(t.derive for t in args.terms) else data


@pytest.mark.parametrize("variant", ["ordered", "linked", "reads", "multi_sorted"])
def test_reference_sorted_columns_links(variant):
    po2, zk = 9, 100
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, _po2, _zk, code, full, bare = bus_cases.honest(variant, po2, zk)
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(len(variant))
    want = _derive_chain(args, po2, zk, code, bare)
    assert np.array_equal(want, full)                                        # the chain makes the honest witness
    code2, bare2 = _raised(rng, code, n), _raised(rng, bare, n)
    got = _derive_chain(args, po2, zk, code2, bare2)
    assert np.array_equal(got % P, want)                                     # residue for residue
    # the copies are copies of the raw words: every derived cell that is >= P is a word of the raised input
    g, b2 = got.reshape(-1, n), bare2.reshape(-1, n)
    derived = sorted({c for r in args.records for c in r.dsts} | {c for t in args.terms if t.sorted_from is not None for _g, c in t.tuple_cols})
    big = g[derived, :A][g[derived, :A] >= P]
    assert big.size and np.isin(big, b2[:, :A]).all()
    # what a stage computes (limbs, flags, linked, last, multiplicities) is a reduced word
    computed = [c for r in args.records for c in (r.dsts if isinstance(r, logup.Record) else (r.linked, r.last) + tuple(r.limbs))]
    computed += [t.mult[1] for t in args.terms if t.derive]
    assert np.array_equal(g[computed, :A], want.reshape(-1, n)[computed, :A])
    rest = [c for c in range(g.shape[0]) if c not in derived and c not in computed]
    assert np.array_equal(g[rest], b2[rest]) and np.array_equal(g[:, A:], b2[:, A:])


@pytest.mark.parametrize("kind", ["range5", "sparse", "big", "two"])
def test_reference_links_with_an_image(kind):
    po2, zk = 8, 40
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data, image = pc.case(kind, 100 * po2 + 3, po2, zk)
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(8)
    t, t_image = data % P, image % P                                         # `big` holds raw words itself
    want = logup.reference_links(args, po2, zk, code.reshape(-1), t.reshape(-1), image=t_image)
    srcs = [pc.KEY, pc.CLOCK, pc.VALUE, pc.WRITE] + ([pc.SECOND, pc.SECOND + 1, pc.SECOND + 2] if kind == "two" else [])
    data2 = t.copy()
    data2[srcs] = rw.raise_words(t[srcs], rng, SHARE)
    code2, image2 = rw.raise_words(code, rng, SHARE), rw.raise_words(t_image, rng, SHARE)
    got = logup.reference_links(args, po2, zk, code2.reshape(-1), data2.reshape(-1), image=image2)
    assert np.array_equal(got % P, want % P)
    g, w = got.reshape(-1, n), want.reshape(-1, n)
    computed = [pc.LINKED, pc.LAST, pc.P_ON] + list(range(pc.LIMB0, pc.LIMB0 + 3)) + list(range(pc.ALIMB0, pc.ALIMB0 + 6))
    assert np.array_equal(g[computed, :A], w[computed, :A])
    copies = g[[pc.PCLOCK, pc.PVALUE, pc.P_ADDR, pc.P_IN, pc.P_OUT, pc.P_TIME], :A]
    assert (copies >= P).any() and np.isin(copies[copies >= P], np.concatenate([data2.reshape(-1), image2])).all()
    # the page-out writes the raw p_out words: the image after it is the same image, residue for residue
    out_w, out_g = logup.reference_page_out(args, po2, zk, want, t_image), logup.reference_page_out(args, po2, zk, got, image2)
    assert np.array_equal(out_g % P, out_w % P) and not np.array_equal(out_w, t_image)
    assert np.array_equal(logup.reference_image_root(out_g), logup.reference_image_root(out_w))


def test_reference_links_refusals():
    po2, zk = 10, 300
    n = 1 << po2
    variant, _accum, code, forged, _out, _mix, row, _cols = rows_cases.lookup_forgery("misread_row", po2, zk)
    desc, blob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True, reads=True)
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(6)
    call = lambda c, d: logup.reference_links(args, po2, zk, c, d)
    msg = _same_refusal(call, (code, forged), (_raised(rng, code, n), _raised(rng, forged, n)))
    assert f"at row {row}: a load of carried column " in msg
    # ... and with an image: a load that the image does not answer, the image's word raised
    desc, blob, code, data, image = pc.case("range5", 5, 8, 40)
    args = logup.Arguments.parse(blob)
    A = 256 - 40
    first = next(r for r in range(A) if data[pc.WRITE, r] == 0)              # the first access is a load of these kinds
    bad = data.copy()
    bad[pc.VALUE, first] = (int(bad[pc.VALUE, first]) + rw.R1) % P
    call = lambda c, d, im: logup.reference_links(args, 8, 40, c.reshape(-1), d.reshape(-1), image=im)
    msg = _same_refusal(call, (code, bad, image), (rw.raise_words(code, rng, SHARE), rw.raise_words(bad, rng, SHARE), rw.raise_words(image, rng, SHARE)))
    assert "the image holds" in msg


@pytest.mark.parametrize("name", list(bus_cases.HAND) + ["corrupt_limb", "wrong_pval"])
def test_reference_bus(name):
    case = bus_cases.hand(name) if name in bus_cases.HAND else bus_cases.forgery(name)
    desc, blob, po2, zk, code, data = case[:6]
    n = 1 << po2
    args = logup.Arguments.parse(blob)
    rng = np.random.default_rng(len(name))
    code, data = code % P, data % P                                          # `raw_words` holds raw words itself
    want = logup.reference_bus(args, po2, zk, code, data)
    got = logup.reference_bus(args, po2, zk, _raised(rng, code, n), _raised(rng, data, n))
    bus_cases.same(got, want)
    assert logup.describe_bus(got, args) == logup.describe_bus(want, args)
    if name in bus_cases.HAND:
        assert (want["term"], want["row"]) == bus_cases.HAND[name][:2]


@pytest.mark.parametrize("kind", rows_cases.FORGERIES + ("honest",))
def test_reference_check_rows(kind):
    po2, zk = 8, 40
    n = 1 << po2
    rng = np.random.default_rng(len(kind))
    if kind == "honest":
        variant = "reads"
        code, data, out, mix = rows_cases.lookup_witness(variant, po2, zk)
        accum, row = rows_cases.lookup_accum(variant, po2, zk, code, data, mix), -1
    else:
        variant, accum, code, data, out, mix, row, _cols = rows_cases.lookup_forgery(kind, po2, zk)
    desc, _blob = rows_cases.lookup_circuit(variant)
    want = check.reference_check_rows(desc, po2, accum, code, data, out, mix)
    assert check.first_failure(want)[0] == row
    globals_ = [(np.asarray(g, dtype=np.uint32) + np.where(rng.random(len(g)) < 0.5, np.uint32(P), np.uint32(0))) for g in (out, mix)]     # a handful of words: + P
    raised = [_raised(rng, a, n) for a in (accum, code, data)] + globals_
    got = check.reference_check_rows(desc, po2, *raised)
    assert np.array_equal(got, want)
    if row >= 0:
        step = int(want[row])
        assert check.reference_value(desc, po2, *raised, row, step) == check.reference_value(desc, po2, accum, code, data, out, mix, row, step)
