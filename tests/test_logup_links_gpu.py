"""LINK records on the GPU (zkh_derive_links, csrc/links.hip): word for word against the host reference at three sizes (A = 216: no
multiple of a wave; 2102; 6198: past one 4096-item sort tile) over the key patterns that can break a link — one chain through every
wave and tile boundary, nothing linked, a handful of addresses, a sparse selector, one access, none, raw words >= P next to their
residues, keys that differ in bit 0 or bit 30 only, two records in one blob, no limbs —, the chain columns -> links -> multiplicities
on SYN-LOOKUP-linked against the host-made witness and sealed byte-identically to the flag-free blob, the native session,
SYN-LOOKUP-linked FULL at po2 20, the refusals (data unchanged, nothing sealed), a forged forward link that yields no accepted seal, and
the sparse upload.

Mutants these cases catch (never committed): taking prev from sorted position j + 1 instead of j - 1 fails every case with a linked
access (`equal`, `range5`, ...); treating the first item of a 4096-item sort tile as unlinked fails `equal` at po2 13, where sorted
position 4096 continues the one chain."""
import numpy as np
import pytest

from args_gpu import circuit as _circuit, enc as _enc, links_refused, profiled, seal_host as _seal_host, upload as _upload
import zko
from conftest import rand_fp
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x0C05
ONE = (1 << 32) % P
TINY, FULL = syn_lookup.TINY, syn_lookup.FULL
SIZES = [(8, 40), (12, 1994), (13, 1994)]
WC, PER_REC = 8, 12                             # code columns; data columns per record: key, clock, carried, 9 destinations


def _keys(kind, rng, A):
    if kind in ("equal", "nl0"):
        return np.full(A, 77777, dtype=np.int64)
    if kind == "distinct":
        return rng.permutation(A).astype(np.int64) * 3 + 1
    if kind == "spread31":                      # keys over 31 bits, many of them one bit apart: bit 0, bit 30, and a byte boundary
        pool = rng.integers(0, 1 << 30, 12)
        pool = np.concatenate([pool, pool ^ 1, pool ^ (1 << 30), pool ^ (1 << 8), [0, P - 1, P - 2]]) % P
        return pool[rng.integers(0, pool.size, A)].astype(np.int64)
    return rng.integers(0, 5 if kind in ("range5", "sparse", "big", "two") else 1 << 12, A).astype(np.int64)


def _case(kind, seed, po2, zk):
    """-> (desc, blob, code, data): random traces (destinations and blinding rows poisoned) under one LINK record, or two for `two`.
    The clock of an access is the number of earlier accesses to its key times a step, so every difference fits the limbs."""
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    n_rec = 2 if kind == "two" else 1
    wd = PER_REC * n_rec + 1
    code, data = rand_fp(rng, WC, n), rand_fp(rng, wd, n)
    b = logup.LogupBuilder((4, WC, wd), (4, 8))
    b.term(0, [(GROUP_DATA, wd - 1)], tag=1)
    for i in range(n_rec):
        base = PER_REC * i
        L, nl, nc = (8, 0, 1) if kind == "nl0" else (5, 4, 3) if i else (8, 3, 2)
        sel = 3 + i if kind in ("sparse", "one", "none", "two") else None
        keys = _keys(kind, rng, A)
        if sel is not None:
            on = rng.random(A) < (0.3 if kind in ("sparse", "two") else 0)
            if kind == "one":
                on[A // 2] = True
            code[sel, :A] = _enc(on.astype(np.uint64))
        else:
            on = np.ones(A, dtype=bool)
        step = 1 if kind == "nl0" else int(rng.integers(1, 40))
        seen, clock = {}, np.zeros(A, dtype=np.int64)
        for r in np.nonzero(on)[0]:
            k = int(keys[r])
            clock[r] = seen.get(k, int(rng.integers(0, 1000))) + (step if k in seen else 0)
            seen[k] = int(clock[r])
        clock[~on] = rng.integers(0, P, int((~on).sum()))
        kcol = (GROUP_CODE, 5 + i) if kind == "two" and i else (GROUP_DATA, base)
        groups = {GROUP_CODE: code, GROUP_DATA: data}
        groups[kcol[0]][kcol[1], :A] = _enc(keys)
        data[base + 1, :A] = _enc(clock)
        if kind in ("big", "spread31", "two"):                               # about a third of the keys and clocks as raw words >= P
            for col in (groups[kcol[0]][kcol[1]], data[base + 1]):
                col[:A][rng.random(A) < 0.3] += np.uint32(P)
        carried = [(GROUP_DATA, base + 1), (GROUP_DATA, base + 2), (GROUP_CODE, 7)][:nc]
        b.derive_links(sel, kcol, carried, list(range(base + 3, base + 3 + 2 + nc + nl)), L)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code.reshape(-1), data.reshape(-1)


KINDS = ["equal", "distinct", "range5", "sparse", "one", "none", "big", "spread31", "two", "nl0"]


@pytest.mark.parametrize("po2,zk", SIZES)
def test_links_match_the_reference(hal, po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(KINDS):
        desc, blob, code, data = _case(kind, 100 * po2 + i, po2, zk)
        args = logup.Arguments.parse(blob)
        assert args.version == 5 and len(args.records) == (2 if kind == "two" else 1)
        c = _circuit(hal, desc, blob)
        assert c.derives_links() and not c.derives_columns() and not c.derives_sorted() and not c.derives_multiplicities()
        assert c.derived_data_columns() == sorted(x for r in args.records for x in r.dsts)
        want = logup.reference_links(args, po2, zk, code, data)
        w = want.reshape(-1, n)
        r0 = args.records[0]
        linked, last = int((w[r0.linked, :A] == ONE).sum()), int((w[r0.last, :A] == ONE).sum())
        if kind in ("equal", "nl0"):
            assert (linked, last) == (A - 1, 1)
        elif kind == "distinct":
            assert (linked, last) == (0, A)
        elif kind in ("one", "none"):
            assert (linked, last) == (0, int(kind == "one"))
        else:
            assert linked > A // 8 and last >= 3
        dcode, ddata = _upload(hal, code, data)
        prof = profiled(hal, lambda: hal.derive_links(c, po2, zk, dcode, ddata))
        assert {"sort_keys", "sort_pack", "links_check", "links_write"} <= set(prof), set(prof)
        if kind == "spread31":                                               # bits 0 and 30 are live, 25 or more in all: four digit passes
            k = logup._dec(data.reshape(-1, n)[0, :A]).astype(np.int64)
            live = int(np.bitwise_or.reduce(k) & ~np.bitwise_and.reduce(k))
            assert live & 1 and live >> 30 & 1 and bin(live).count("1") > 24 and "sort_passes" in prof
        got = ddata.to_vec()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{kind} po2 {po2}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
        assert not np.array_equal(got, data)                                 # the (poisoned) destinations were written
        assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])    # the blinding rows were not
        assert np.array_equal(dcode.to_vec(), code)
        hal.derive_links(c, po2, zk, dcode, ddata)                           # a function of the sources: again the same
        assert np.array_equal(ddata.to_vec(), want)


# ---- the chain on SYN-LOOKUP-linked ----
def _linked(shape):
    """-> (description, the blob with everything derived, the flag-free blob of the same arguments)"""
    desc, blob = syn_lookup.build_syn_lookup(shape, derive=True, limbs=True, link=True)
    return desc, blob, logup.Arguments.parse(blob).plain().blob()


def _witnesses(shape, po2, zk, seed, addr_range):
    code, full, out = syn_lookup.witness(shape, po2, zk, seed=seed, addr_range=addr_range, link=True)
    _, bare, _ = syn_lookup.witness(shape, po2, zk, seed=seed, addr_range=addr_range, count=False, limbs=False, link=False)
    return code, full, bare, out


@pytest.mark.parametrize("po2,zk,addr_range", [(8, 40, 16), (12, 1994, 5), (13, 1994, 64)])
def test_the_chain_equals_the_host_made_witness_and_seals_alike(hal, oracle, po2, zk, addr_range):
    desc, blob, plain = _linked(TINY)
    assert logup.Arguments.parse(plain).version == 1 and logup.Arguments.parse(blob).version == 5
    code, full, bare, out = _witnesses(TINY, po2, zk, po2, addr_range)
    assert not np.array_equal(bare, full)
    c = _circuit(hal, desc, blob)
    assert c.derives_links() and c.derives_columns() and c.derives_multiplicities() and not c.derives_sorted()
    dcode, ddata = _upload(hal, code, bare)
    hal.derive_columns(c, po2, zk, dcode, ddata)
    hal.derive_links(c, po2, zk, dcode, ddata)
    hal.derive_multiplicities(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), full)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out)
    again = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out)
    host = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    assert np.array_equal(receipt.seal, host.seal) and np.array_equal(receipt.seal, again.seal)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


def test_native_session_derives_links(hal, oracle):
    from zeth_amd.host import Session
    po2 = 12
    desc, blob, plain = _linked(TINY)
    segs = [Segment(index=i, po2=po2, noise_seed=NOISE + i) for i in range(2)]
    wit = [_witnesses(TINY, po2, s.zk_cycles, 70 + i, 64) for i, s in enumerate(segs)]
    sess = Session(desc, lanes_per_device=1)
    sess.set_arguments(blob)
    comp, _, _ = sess.prove(segs, host_traces=[(code, bare, out) for code, _full, bare, out in wit], verify=True)
    sess.close()
    prover = SegmentProver(hal, desc, arguments=plain)                       # the flag-free blob on the host-made witness
    oc = zko.OracleCircuit(oracle, desc)
    for seg, (code, full, _bare, out), r in zip(segs, wit, comp.segments):
        assert oc.verify(r.seal, oc.root_of_code(po2, code)) is None
        assert np.array_equal(r.seal, _seal_host(hal, prover, seg, code, full, out).seal)


def _strip(c, data, po2, zk, fill=0):
    """a copy of the host-made `data` with the active rows of every column the library derives set to `fill`"""
    n = 1 << po2
    d = data.reshape(-1, n).copy()
    d[c.derived_data_columns(), :n - zk] = fill
    return d.reshape(-1)


def test_syn_lookup_linked_full_at_po2_20(hal, oracle):
    po2, zk = 20, zhal.ZK_CYCLES
    desc, blob, plain = _linked(FULL)
    c = _circuit(hal, desc, blob)
    assert int(desc[5]) == 16 + 64 + 1 + 10 and len(c.derived_data_columns()) == 64 + 1 + 7
    code, want, out = syn_lookup.witness(FULL, po2, zk, seed=22, link=True)
    bare = _strip(c, want, po2, zk)
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out)
    host = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, want, out)
    assert np.array_equal(receipt.seal, host.seal)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


# ---- refusals ----
def _refused(hal, desc, blob, po2, zk, code, data, want_msg):
    links_refused(hal, desc, blob, po2, zk, code, data, want_msg, seal=True)


def test_refusals_name_the_lowest_record_and_row_and_leave_data_unchanged(hal):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data = _case("two", 9, po2, zk)                        # record 0: selector code 3, clock data 1, L nl = 24 bits
    args = logup.Arguments.parse(blob)
    c2, d2 = code.reshape(-1, n).copy(), data.reshape(-1, n).copy()
    # selectors come first, over all records: record 1's bad selector is named although record 0 has a bad clock at a lower row
    c2[4, 700], c2[4, 650] = _enc(2), _enc(P - 1)
    on0 = np.nonzero(c2[3, :A] == ONE)[0]
    k0 = logup._dec(d2[0, :A])
    chain = [r for r in on0 if k0[r] == k0[on0[5]]]                          # the accesses of record 0 to one address, in row order
    assert len(chain) >= 4
    d2[1, chain[2]] = d2[1, chain[0]]                                        # the clock of the third = the clock of the first
    _refused(hal, desc, blob, po2, zk, c2, d2, f"record 1 at row 650: selector {P - 1}, not 0 or 1")
    c2[4, 650] = c2[4, 700] = 0
    t0, t1 = int(logup._dec(d2[1, chain[0]])), int(logup._dec(d2[1, chain[1]]))
    msg = f"record 0 at row {chain[2]}: clock not increasing ({t0} after {t1} at row {chain[1]})"
    d2[PER_REC + 1, :A] = d2[PER_REC + 1, ::-1][n - A:]                      # record 1's clocks reversed: bad too, but record 0 is named
    _refused(hal, desc, blob, po2, zk, c2, d2, msg)
    # of two bad rows of one record the lower; a clock equal to the previous one is d = -1
    d2[1, chain[3]] = d2[1, chain[2]]
    _refused(hal, desc, blob, po2, zk, c2, d2, msg)
    # in order, but too wide: 2^24 + 1 after the previous clock
    d3 = data.reshape(-1, n).copy()
    d3[1, chain[1]] = _enc(t0 + (1 << 24) + 1)
    _refused(hal, desc, blob, po2, zk, code, d3,
             f"record 0 at row {chain[1]}: the clock difference {1 << 24} (after row {chain[0]}) does not fit 3 limbs of 8 bits")
    d3[1, chain[1]] = _enc(t0 + (1 << 24))                                   # the widest that fits: its successor is then behind it
    with pytest.raises(HalError, match=f"record 0 at row {chain[2]}: clock not increasing"):
        hal.derive_links(_circuit(hal, desc, blob), po2, zk, *_upload(hal, code, d3.reshape(-1)))
    # a circuit without LINK records is an error, not a no-op
    pdesc, pblob = syn_lookup.build_syn_lookup(TINY, limbs=True)
    pcode, pdata, _ = syn_lookup.witness(TINY, po2, zk, seed=2)
    dcode, ddata = _upload(hal, pcode, pdata)
    with pytest.raises(HalError, match="hold no LINK record"):
        hal.derive_links(_circuit(hal, pdesc, pblob), po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), pdata)


# ---- a forged link ----
def test_a_forged_forward_link_yields_no_accepted_seal(hal, oracle):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, plain = _linked(TINY)
    code, full, _bare, out = _witnesses(TINY, po2, zk, 12, 16)
    d = syn_lookup.relink_row(TINY, full, po2, A // 2).reshape(-1, n)
    m = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[2]
    d[m, :A] = 0
    counted = logup.Arguments.parse(syn_lookup.build_syn_lookup(TINY, derive=True, link=True)[1])
    assert counted.version == 5 and all(r.kind == logup.KIND_LINK for r in counted.records)
    forged = logup.reference_multiplicities(counted, po2, zk, code, d.reshape(-1))          # the limbs of the forged rows counted
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    _, total = logup.reference_accumulate(logup.Arguments.parse(plain), po2, zk, code, forged, mix)
    assert total == [0, 0, 0, 0]                                             # every lookup is answered and the bus balances
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    honest = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    honest.verify(desc, root)                                                # the honest witness under the same blob is accepted
    try:
        receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, forged, out)
    except HalError:
        return                                                               # no seal at all
    with pytest.raises(HalError):
        receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is not None


# ---- the sparse upload ----
def test_link_destinations_cross_on_blinding_rows_only(hal):
    po2, zk = 14, zhal.ZK_CYCLES
    n = 1 << po2
    desc, blob = syn_lookup.build_syn_lookup(TINY, link=True)                # only the LINK record derives: 7 of the 21 data columns
    c = _circuit(hal, desc, blob)
    lcols = syn_lookup.link_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0]
    assert c.derived_data_columns() == lcols[3:] and int(desc[5]) == 21
    code, want, out = syn_lookup.witness(TINY, po2, zk, seed=14, addr_range=64, link=True)
    bare = _strip(c, want, po2, zk, fill=0x12345678)                         # garbage in what the library derives never crosses
    ddata = hal.alloc("data", want.size, zero=True)
    dcode = hal.alloc_elem("code", code.size)
    dcode.write(code)
    before = hal.h2d_bytes()
    hal.upload_data_trace(c, po2, zk, ddata, bare, pinned_async=False)
    assert hal.h2d_bytes() - before == 4 * ((21 - 7) * n + 7 * zk)
    hal.derive_links(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), want)
