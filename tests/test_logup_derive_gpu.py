"""Derived lookup multiplicities on the GPU (zkh_derive_multiplicities, csrc/multiplicities.hip): word for word against the host reference
over random argument sets on both sides of the LDS / global count, SYN-LOOKUP-derived at po2 20 against the host count and sealed
byte-identically to the plain circuit, the refusals (data unchanged, nothing sealed), the native session, WIDE (a 2^16-row table) and
determinism."""
import numpy as np
import pytest

from args_gpu import enc as _enc, seal_host as _seal_host
import zko
from conftest import rand_fp
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x10C1
ONE = (1 << 32) % P


def _random_case(seed, po2, zk, big):
    """two tags: tag 3 with two derived tables (the second repeating part of the first, selectors in code), tag 5 with one (values in
    code or data, small or -- big -- mostly distinct keys); lookups of tuple widths 1..4 with selectors and multiplicities (weights
    other than 1) whose weight-0 rows hold keys in no table.  -> (desc, blob, code, data)"""
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    wc, wd = 32, 40
    code, data = rand_fp(rng, wc, n), rand_fp(rng, wd, n)
    b = logup.LogupBuilder((4 * 4, wc, wd), (4, 8))
    terms = []
    nc, nd = iter(range(wc)), iter(range(wd))
    wa, wb = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    # tag 3: table D1 (width wa, values from a pool of 40, rows selected by a 0/1 code selector), D2 = D1's columns on other rows
    t1 = [(GROUP_DATA if rng.random() < 0.5 else GROUP_CODE, None) for _ in range(wa)]
    t1 = [(g, next(nd) if g == GROUP_DATA else next(nc)) for g, _ in t1]
    pool = rng.integers(0, P, size=(40, wa), dtype=np.uint64)
    pick = rng.integers(0, 40, A)
    for e, (g, c) in enumerate(t1):
        (data if g == GROUP_DATA else code)[c, :A] = _enc(pool[pick, e])
    s1, s2 = next(nc), next(nc)
    code[s1, :A] = _enc(rng.random(A) < 0.3)
    code[s2, :A] = _enc(rng.random(A) < 0.1)
    m1, m2, m3 = next(nd), next(nd), next(nd)
    terms.append(dict(tuple_cols=t1, sign=-1, sel=s1, mult=(GROUP_DATA, m1), tag=3, derive=True))
    terms.append(dict(tuple_cols=t1, sign=-1, sel=s2, mult=(GROUP_DATA, m2), tag=3, derive=True))
    tab1 = np.nonzero((_dec(code[s1, :A]) == 1) | (_dec(code[s2, :A]) == 1))[0]
    # tag 5: table D3 of width wb, no selector: every active row an entry
    g3 = GROUP_DATA if big else GROUP_CODE
    t3 = [(g3, next(nd) if g3 == GROUP_DATA else next(nc)) for _ in range(wb)]
    vals = rng.integers(0, P, size=(A if big else 300, wb), dtype=np.uint64)
    if not big:
        vals = vals[rng.integers(0, 300, A)]                                 # at most 300 distinct keys: the LDS count
    for e, (g, c) in enumerate(t3):
        (data if g == GROUP_DATA else code)[c, :A] = _enc(vals[:, e])
    terms.append(dict(tuple_cols=t3, sign=-1, mult=(GROUP_DATA, m3), tag=5, derive=True))
    groups = {GROUP_CODE: code, GROUP_DATA: data}

    def lookup(tag, table_cols, rows_of_table, width):
        cols = [(GROUP_DATA, next(nd)) if rng.random() < 0.7 else (GROUP_CODE, next(nc)) for _ in range(width)]
        src = rng.choice(rows_of_table, A)
        for (g, c), (tg, tc) in zip(cols, table_cols):
            groups[g][c, :A] = groups[tg][tc, src]
        spec = dict(tuple_cols=cols, tag=tag)
        weight = np.ones(A, bool)
        if rng.random() < 0.7:
            sc = next(nc)
            code[sc, :A] = rand_fp(rng, A)
            code[sc, :A][rng.random(A) < 0.2] = 0
            spec["sel"] = sc
            weight &= code[sc, :A] != 0
        if rng.random() < 0.7:
            g, c = (GROUP_DATA, next(nd)) if rng.random() < 0.7 else (GROUP_CODE, next(nc))
            groups[g][c, :A] = _enc(rng.integers(0, 5, A))
            spec["mult"] = (g, c)
            weight &= groups[g][c, :A] != 0
        g0, c0 = cols[0]
        groups[g0][c0, :A][~weight] = _enc(rng.integers(P - 10 ** 6, P, int((~weight).sum()), dtype=np.uint64))   # keys in no table
        return spec
    terms.append(lookup(3, t1, tab1, wa))
    terms.append(lookup(3, t1, tab1, wa))
    terms.append(lookup(5, t3, np.arange(A), wb))
    terms.append(dict(tuple_cols=[(GROUP_DATA, next(nd))], tag=9))            # another tag, no table: not a lookup of the derive
    order = rng.permutation(len(terms))
    for i, j in enumerate(order):
        b.term(i // 2, **terms[j])
    chain = b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2))
    desc, blob = b.finish_all(chain)
    return desc, blob, code.reshape(-1), data.reshape(-1)


def _dec(x):
    return (np.asarray(x, dtype=np.uint64) * np.uint64(pow(ONE, -1, P))) % np.uint64(P)


def _derive(hal, c, po2, zk, code, data):
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", data.size)
    dcode.write(code)
    ddata.write(data)
    hal.derive_multiplicities(c, po2, zk, dcode, ddata)
    return ddata.to_vec()


GRID = [(8, 37, False), (9, 100, False), (10, 11, False), (11, 970, False), (12, 1994, False), (13, 1994, True), (14, 1994, True),
        (14, 3, False)]


def test_random_arguments_match_the_reference_on_both_count_paths(hal):
    seen = set()
    for po2, zk, big in GRID:
        desc, blob, code, data = _random_case(po2 * 7 + zk, po2, zk, big)
        c = hal.load_circuit(desc, jit=False)
        c.set_arguments(blob)
        assert c.derives_multiplicities()
        want = logup.reference_multiplicities(logup.Arguments.parse(blob), po2, zk, code, data)
        hal.prof_enable(True)
        hal.prof_reset()
        got = _derive(hal, c, po2, zk, code, data)
        names = {r["name"] for r in hal.prof_get() if r["calls"]}
        hal.prof_enable(False)
        assert {"derive_build", "derive_write"} <= names
        path = "derive_count_global" if big else "derive_count_lds"
        assert path in names, (po2, names)
        seen.add(path)
        bad = np.nonzero(got != want)[0]
        n = 1 << po2
        assert bad.size == 0, f"po2 {po2}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
        assert not np.array_equal(got, data)                                 # the m columns were rewritten
    assert seen == {"derive_count_lds", "derive_count_global"}


def test_syn_lookup_derived_at_po2_20(hal, oracle):
    po2, zk = 20, zhal.ZK_CYCLES
    desc, blob = syn_lookup.syn_lookup_derived()
    pdesc, pblob = syn_lookup.syn_lookup()
    assert np.array_equal(desc, pdesc)
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    code, want, out = syn_lookup.witness(syn_lookup.FULL, po2, zk, seed=21)
    _, zero, _ = syn_lookup.witness(syn_lookup.FULL, po2, zk, seed=21, count=False)
    assert np.array_equal(_derive(hal, c, po2, zk, code, zero), want)
    m = syn_lookup.layout(syn_lookup.FULL.n_words, syn_lookup.FULL.n_limbs, syn_lookup.FULL.n_mem)[2]
    garbage = zero.reshape(-1, 1 << po2).copy()
    garbage[m, :(1 << po2) - zk] = rand_fp(np.random.default_rng(5), (1 << po2) - zk)
    assert np.array_equal(_derive(hal, c, po2, zk, code, garbage.reshape(-1)), want)
    # sealed through seal_host_witness from the uncounted witness: both verifiers accept, and the seal is the plain circuit's of the
    # host-counted witness, byte for byte
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, garbage.reshape(-1), out)
    plain = _seal_host(hal, SegmentProver(hal, pdesc, arguments=pblob), seg, code, want, out)
    assert np.array_equal(receipt.seal, plain.seal)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


def test_refusals_leave_data_unchanged(hal):
    po2, zk = 10, 200
    desc, blob = syn_lookup.syn_lookup_tiny_derived()
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    code, data, out = syn_lookup.witness(syn_lookup.TINY, po2, zk, seed=7, count=False)
    bad = syn_lookup.corrupt_limb(syn_lookup.TINY, data, po2, row=123, word=1)
    dcode, ddata = hal.alloc_elem("code", code.size), hal.alloc_elem("data", bad.size)
    dcode.write(code)
    ddata.write(bad)
    limb = int(logup._dec(bad.reshape(-1, 1 << po2)[6, 123]))
    with pytest.raises(HalError, match=r"lookup term 4 \(tag 0\) at row 123 has no table entry: key \(%d, 0, 0, 0\)" % limb):
        hal.derive_multiplicities(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), bad)
    prover = SegmentProver(hal, desc, arguments=blob)
    seg = Segment(index=0, po2=12, noise_seed=NOISE)
    code12, data12, out12 = syn_lookup.witness(syn_lookup.TINY, 12, seg.zk_cycles, seed=7, count=False)
    with pytest.raises(HalError, match="at row 123 has no table entry"):                   # nothing is sealed
        _seal_host(hal, prover, seg, code12, syn_lookup.corrupt_limb(syn_lookup.TINY, data12, 12, row=123, word=1), out12)
    c2 = code.reshape(-1, 1 << po2).copy()
    c2[5, 3] = _enc(2)                                                       # table selector 2 on row 3
    dcode.write(c2.reshape(-1))
    ddata.write(data)
    with pytest.raises(HalError, match=r"table term 8 \(tag 0\) has selector 2 at row 3"):
        hal.derive_multiplicities(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), data)
    with pytest.raises(HalError, match="derive no multiplicity"):
        plain = hal.load_circuit(desc, jit=False)
        plain.set_arguments(syn_lookup.syn_lookup_tiny()[1])
        hal.derive_multiplicities(plain, po2, zk, dcode, ddata)


def test_native_session_derives(hal, oracle):
    from zeth_amd.host import Session
    po2 = 12
    desc, blob = syn_lookup.syn_lookup_tiny_derived()
    segs = [Segment(index=i, po2=po2, noise_seed=NOISE + i) for i in range(2)]
    traces = [syn_lookup.witness(syn_lookup.TINY, po2, s.zk_cycles, seed=40 + i, count=False) for i, s in enumerate(segs)]
    sess = Session(desc, lanes_per_device=1)
    sess.set_arguments(blob)
    comp, _, _ = sess.prove(segs, host_traces=traces, verify=True)
    sess.close()
    prover = SegmentProver(hal, desc, arguments=blob)
    oc = zko.OracleCircuit(oracle, desc)
    for seg, (code, data, out), r in zip(segs, traces, comp.segments):
        assert oc.verify(r.seal, oc.root_of_code(po2, code)) is None
        assert np.array_equal(r.seal, _seal_host(hal, prover, seg, code, data, out).seal)


def test_wide_table_at_po2_17(hal, oracle):
    po2, zk = 17, zhal.ZK_CYCLES
    desc, blob = syn_lookup.build_syn_lookup(syn_lookup.WIDE, derive=True)
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    code, want, out = syn_lookup.witness(syn_lookup.WIDE, po2, zk, seed=17)
    _, zero, _ = syn_lookup.witness(syn_lookup.WIDE, po2, zk, seed=17, count=False)
    assert np.array_equal(logup.reference_multiplicities(logup.Arguments.parse(blob), po2, zk, code, zero), want)
    hal.prof_enable(True)
    hal.prof_reset()
    got = _derive(hal, c, po2, zk, code, zero)
    names = {r["name"] for r in hal.prof_get() if r["calls"]}
    hal.prof_enable(False)
    assert "derive_count_global" in names
    assert np.array_equal(got, want)
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, zero, out)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


def test_fills_are_deterministic(hal):
    po2, zk = 13, 1994
    desc, blob, code, data = _random_case(99, po2, zk, True)
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    first = _derive(hal, c, po2, zk, code, data)
    assert np.array_equal(_derive(hal, c, po2, zk, code, data), first)
    desc, blob = syn_lookup.syn_lookup_tiny_derived()
    c = hal.load_circuit(desc, jit=False)
    c.set_arguments(blob)
    code, data, _ = syn_lookup.witness(syn_lookup.TINY, 12, 1994, seed=3, count=False)
    assert np.array_equal(_derive(hal, c, 12, 1994, code, data), _derive(hal, c, 12, 1994, code, data))
