"""Derived sorted copies on the GPU (zkh_derive_sorted, csrc/sort.hip): word for word against the host reference over random argument
sets (tuple widths 1..4, 1..3 keys, selectors, code and data sources, several pairs, narrow and 93-bit keys), stability and determinism
on many equal keys, SYN-LOOKUP-sorted at po2 20 against the host sort and sealed byte-identically to the plain circuit, the native
session, the refusals (data unchanged), and one size above 2^20 rows."""
import numpy as np
import pytest

from args_gpu import circuit as _circuit, enc as _enc, seal_host as _seal_host
import zko
from conftest import rand_fp
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x50C7
ONE = (1 << 32) % P


def _key_values(rng, style, A):
    """canonical values of one key field"""
    if style == "few":                                                       # confined to a few bits: many equal keys
        return rng.integers(0, 1 << int(rng.integers(1, 7)), A, dtype=np.uint64)
    if style == "full":                                                      # all 31 bits
        v = rng.integers(0, P, A, dtype=np.uint64)
        v[:2] = (P - 1, 0)
        return v
    if style == "offset":                                                    # a few live bits under constant high bits
        return np.uint64(0x5A5A0000) + (rng.integers(0, 1 << 5, A, dtype=np.uint64) << np.uint64(3))
    return np.full(A, int(rng.integers(0, P)), dtype=np.uint64)               # "equal": no live bit at all


def _random_case(seed, po2, zk, style, selector=None):
    """1..3 pairs (source +1, sorted copy -1, one accum column each) of widths 1..4 with 1..3 keys at random tuple positions, sources
    in code and data, half of them under a 0/1 code selector, about one raw word in twenty of every source column >= P.  style: the
    key fields are "few", "full" (the first pair then has three 31-bit keys: a 93-bit packed key) or a mixture.
    -> (desc, blob, code, data)"""
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    wc, wd = 24, 40
    code, data = rand_fp(rng, wc, n), rand_fp(rng, wd, n)
    groups = {GROUP_CODE: code, GROUP_DATA: data}
    nc, nd = iter(range(3, wc)), iter(range(wd))
    n_pairs = int(rng.integers(1, 4))
    b = logup.LogupBuilder((4 * n_pairs, wc, wd), (4, 8))
    for p in range(n_pairs):
        w = int(rng.integers(1, 5))
        if style == "full" and p == 0:
            w = max(w, 3)
        nkeys = 3 if style == "full" and p == 0 else int(rng.integers(1, min(w, 3) + 1))
        keys = [int(x) for x in rng.permutation(w)[:nkeys]]
        src = [(GROUP_DATA, next(nd)) if rng.random() < 0.7 else (GROUP_CODE, next(nc)) for _ in range(w)]
        dst = [(GROUP_DATA, next(nd)) for _ in range(w)]
        for pos in keys:
            st = style if style in ("few", "full") else str(rng.choice(["few", "full", "offset", "equal"]))
            g, c = src[pos]
            groups[g][c, :A] = _enc(_key_values(rng, st, A))
        for g, c in src:                                                     # the same residues as raw words >= P (2 P < 2^32)
            big = rng.random(A) < 0.05
            groups[g][c, :A][big] += np.uint32(P)
        sel = None
        if selector if selector is not None else rng.random() < 0.5:
            sel = next(nc)
            code[sel, :A] = _enc(rng.random(A) < rng.choice([0.05, 0.5, 0.97]))
        b.term(p, src, tag=p + 1, sel=sel)
        b.term(p, dst, sign=-1, tag=p + 1, sel=sel, sorted_from=2 * p, sort_keys=keys)
    chain = b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2))
    desc, blob = b.finish_all(chain)
    return desc, blob, code.reshape(-1), data.reshape(-1)


def _derive(hal, c, po2, zk, code, data):
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", data.size)
    dcode.write(code)
    ddata.write(data)
    hal.derive_sorted(c, po2, zk, dcode, ddata)
    return ddata.to_vec()


GRID = [(8, 37, "few"), (9, 100, "mixed"), (10, 11, "full"), (11, 970, "mixed"), (12, 1994, "few"), (13, 1994, "full"), (14, 3, "mixed"),
        (15, 1994, "mixed"), (16, 1994, "full"), (16, 1994, "few")]


def test_random_arguments_match_the_reference(hal):
    widths, nkeys, selectors = set(), set(), set()
    for po2, zk, style in GRID:
        desc, blob, code, data = _random_case(po2 * 11 + zk, po2, zk, style)
        args = logup.Arguments.parse(blob)
        for t in args.terms:
            if t.sorted_from is not None:
                widths.add(len(t.tuple_cols)); nkeys.add(len(t.sort_keys)); selectors.add(t.sel is not None)
        c = _circuit(hal, desc, blob)
        assert c.derives_sorted() and not c.derives_multiplicities()
        want = logup.reference_sorted(args, po2, zk, code, data)
        hal.prof_enable(True)
        hal.prof_reset()
        got = _derive(hal, c, po2, zk, code, data)
        names = {r["name"] for r in hal.prof_get() if r["calls"]}
        hal.prof_enable(False)
        assert {"sort_keys", "sort_pack", "sort_gather"} <= names, names
        n, A = 1 << po2, (1 << po2) - zk
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"po2 {po2} {style}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
        assert not np.array_equal(got, data)                                 # the copies were written
        assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])    # the blinding rows were not
    assert widths == {1, 2, 3, 4} and nkeys == {1, 2, 3} and selectors == {True, False}, (widths, nkeys, selectors)


def test_equal_keys_are_stable_and_deterministic(hal):
    shape = syn_lookup.MULTI
    desc, blob = syn_lookup.build_syn_lookup(shape, sort=True, sort_keys=(0,))
    c = _circuit(hal, desc, blob)
    args = logup.Arguments.parse(blob)
    for po2, zk in ((10, 300), (13, 1994), (16, 1994)):
        code, want, _ = syn_lookup.witness_equal_keys(shape, po2, zk, seed=9)           # the host's stable sort by addr alone
        _, zero, _ = syn_lookup.witness_equal_keys(shape, po2, zk, seed=9, sort=False)
        assert np.array_equal(logup.reference_sorted(args, po2, zk, code, zero), want)
        first = _derive(hal, c, po2, zk, code, zero)
        assert np.array_equal(first, want)
        assert np.array_equal(_derive(hal, c, po2, zk, code, zero), first)
        assert np.array_equal(_derive(hal, c, po2, zk, code, first), first)              # whatever the copies held before
    desc, blob, code, data = _random_case(77, 14, 1994, "few")
    c = _circuit(hal, desc, blob)
    first = _derive(hal, c, 14, 1994, code, data)
    assert np.array_equal(_derive(hal, c, 14, 1994, code, data), first)


def _po2_20_case(derive):
    po2, zk = 20, zhal.ZK_CYCLES
    code, want, out = syn_lookup.witness(syn_lookup.FULL, po2, zk, seed=21)
    _, zero, _ = syn_lookup.witness(syn_lookup.FULL, po2, zk, seed=21, sort=False, count=not derive)
    return po2, zk, code, want, zero, out


@pytest.mark.parametrize("derive", [False, True])
def test_syn_lookup_sorted_at_po2_20(hal, oracle, derive):
    po2, zk, code, want, zero, out = _po2_20_case(derive)
    desc, blob = syn_lookup.build_syn_lookup(syn_lookup.FULL, derive=derive, sort=True)
    pdesc, pblob = syn_lookup.syn_lookup()
    assert np.array_equal(desc, pdesc)
    c = _circuit(hal, desc, blob)
    assert c.derives_sorted() and c.derives_multiplicities() == derive
    got = _derive(hal, c, po2, zk, code, zero)
    if not derive:
        assert np.array_equal(got, want)                                     # the host-sorted witness, every word
    else:
        n = 1 << po2
        perm = [x for cols in syn_lookup.layout(*syn_lookup.FULL[:2], syn_lookup.FULL.n_mem)[4] for x in cols]
        assert np.array_equal(got.reshape(-1, n)[perm], want.reshape(-1, n)[perm])
    # sealed through seal_host_witness from the unsorted (and uncounted) witness: the plain circuit's seal of the host-made witness,
    # byte for byte, and both verifiers accept it
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, zero, out)
    plain = _seal_host(hal, SegmentProver(hal, pdesc, arguments=pblob), seg, code, want, out)
    assert np.array_equal(receipt.seal, plain.seal)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


@pytest.mark.parametrize("derive", [False, True])
def test_native_session_derives_sorted(hal, oracle, derive):
    from zeth_amd.host import Session
    po2 = 12
    desc, blob = syn_lookup.build_syn_lookup(syn_lookup.TINY, derive=derive, sort=True)
    pblob = syn_lookup.syn_lookup_tiny()[1]
    segs = [Segment(index=i, po2=po2, noise_seed=NOISE + i) for i in range(2)]
    traces = [syn_lookup.witness(syn_lookup.TINY, po2, s.zk_cycles, seed=40 + i, sort=False, count=not derive) for i, s in enumerate(segs)]
    full = [syn_lookup.witness(syn_lookup.TINY, po2, s.zk_cycles, seed=40 + i) for i, s in enumerate(segs)]
    sess = Session(desc, lanes_per_device=1)
    sess.set_arguments(blob)
    comp, _, _ = sess.prove(segs, host_traces=traces, verify=True)
    sess.close()
    prover = SegmentProver(hal, desc, arguments=pblob)                       # the plain circuit on the host-made witness
    oc = zko.OracleCircuit(oracle, desc)
    for seg, (code, data, out), r in zip(segs, full, comp.segments):
        assert oc.verify(r.seal, oc.root_of_code(po2, code)) is None
        assert np.array_equal(r.seal, _seal_host(hal, prover, seg, code, data, out).seal)


def test_refusals_leave_data_unchanged(hal):
    po2, zk = 12, 200
    n = 1 << po2
    desc, blob, code, data = _random_case(5, po2, zk, "mixed", selector=True)
    args = logup.Arguments.parse(blob)
    copies = [i for i, t in enumerate(args.terms) if t.sorted_from is not None]
    c = _circuit(hal, desc, blob)
    bad = code.reshape(-1, n).copy()
    last = args.terms[copies[-1]]
    bad[last.sel, 1234] = _enc(2)                                            # the last copy's selector, twice; the lower row is named
    bad[last.sel, 77] = _enc(P - 1)
    msg = r"sorted-copy term %d \(tag %d\) has selector %d at row 77, not 0 or 1" % (copies[-1], last.tag, P - 1)
    with pytest.raises(logup.ReferenceError, match=msg):
        logup.reference_sorted(args, po2, zk, bad.reshape(-1), data)
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", data.size)
    dcode.write(bad.reshape(-1))
    ddata.write(data)
    with pytest.raises(HalError, match=msg):
        hal.derive_sorted(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), data)
    bad[args.terms[copies[0]].sel, 3000] = _enc(3)                           # the first copy is named before the last, whatever the row
    if len(copies) > 1:
        dcode.write(bad.reshape(-1))
        first = args.terms[copies[0]]
        with pytest.raises(HalError, match=r"sorted-copy term %d \(tag %d\) has selector 3 at row 3000" % (copies[0], first.tag)):
            hal.derive_sorted(c, po2, zk, dcode, ddata)
        assert np.array_equal(ddata.to_vec(), data)
    good = code.reshape(-1, n).copy()
    good[last.sel, n - zk:] = _enc(7)                                        # the blinding rows of a selector are not looked at
    dcode.write(good.reshape(-1))
    hal.derive_sorted(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), logup.reference_sorted(args, po2, zk, good.reshape(-1), data))
    # nothing is sealed from a refused witness, and a circuit without sorted copies is an error, not a no-op
    tdesc, tblob = syn_lookup.syn_lookup_tiny_sorted()
    for other in (syn_lookup.syn_lookup_tiny()[1], syn_lookup.syn_lookup_tiny_derived()[1]):
        with pytest.raises(HalError, match="derive no sorted copy"):
            tcode, tdata, _ = syn_lookup.witness(syn_lookup.TINY, 10, 200, seed=7)
            tc, td = hal.alloc_elem("code", tcode.size), hal.alloc_elem("data", tdata.size)
            tc.write(tcode)
            td.write(tdata)
            hal.derive_sorted(_circuit(hal, tdesc, other), 10, 200, tc, td)


def test_one_size_above_2_20_rows(hal):
    po2, zk = 22, zhal.ZK_CYCLES
    n, A = 1 << po2, (1 << po2) - zk
    rng = np.random.default_rng(22)
    b = logup.LogupBuilder((4, 3, 4), (4, 8))
    b.term(0, [(GROUP_DATA, 0), (GROUP_DATA, 1)], tag=1)
    b.term(0, [(GROUP_DATA, 2), (GROUP_DATA, 3)], sign=-1, tag=1, sorted_from=0, sort_keys=(0,))
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    code, data = rand_fp(rng, 3, n), rand_fp(rng, 4, n)
    data[0, :A] = _enc(rng.integers(0, 1 << 21, A, dtype=np.uint64))          # 2^21 addresses for 2^22 rows: equal keys among them
    code, data = code.reshape(-1), data.reshape(-1)
    want = logup.reference_sorted(logup.Arguments.parse(blob), po2, zk, code, data)
    got = _derive(hal, _circuit(hal, desc, blob), po2, zk, code, data)
    assert np.array_equal(got, want)
