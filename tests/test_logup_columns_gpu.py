"""Derived-column records on the GPU (zkh_derive_columns, csrc/columns.hip): word for word against the host reference over random records
(every limb width and count, code and data sources, raw words >= P, one and two sorted keys with many equal values, odd row counts),
the chain sorted -> columns -> multiplicities on SYN-LOOKUP-ordered against the host-made witness and sealed byte-identically to the
flag-free blob, the native session, SYN-LOOKUP FULL at po2 20 with every derivable column derived, the refusals (data unchanged,
nothing sealed), a forged order witness that yields no accepted seal, and the sparse upload of a caller's data trace."""
import re

import numpy as np
import pytest

from args_gpu import circuit as _circuit, enc as _enc, seal_host as _seal_host, upload as _upload
import zko
from conftest import rand_fp
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x0C01
ONE = (1 << 32) % P
TINY, MULTI, FULL = syn_lookup.TINY, syn_lookup.MULTI, syn_lookup.FULL


# every (limb bits, limb count) the format allows
SHAPES = [(L, nl) for L in range(1, 17) for nl in range(1, 9) if L * nl <= 32]
# A = n - zk odd (3, 37) and even but no multiple of 64 (970, 1994); the last two: fewer rows than a lane takes, and n no multiple of 4
GRID = [(8, 3), (8, 37), (9, 37), (10, 3), (10, 970), (11, 970), (11, 1994), (12, 1994), (12, 37), (13, 3), (14, 970), (15, 37), (16, 1994),
        (16, 3), (2, 1), (1, 0)]
WC, WD, PER_CASE = 16, 56, 5


def _sorted_keys(rng, A, bits, two):
    """canonical key columns in order whose ordered differences fit `bits` bits, with many equal values, and their sum below P"""
    top = max(1, min(1 << bits, P // (2 * A + 2)))
    if not two:
        return [np.cumsum(np.where(rng.random(A) < 0.6, 0, rng.integers(0, top, A)))]
    k0 = np.cumsum(np.where(rng.random(A) < 0.6, 0, 1 + rng.integers(0, top, A)))       # a step s > 0 of the first key gives d = s - 1
    k1 = np.zeros(A, dtype=np.int64)
    new = np.concatenate([[True], k0[1:] != k0[:-1]])
    inc = rng.integers(0, top, A)
    start = rng.integers(0, P // 2, A)
    cur = 0
    for r in range(A):                                                       # inside a run the second key never falls
        cur = int(start[r]) if new[r] else cur + int(inc[r])
        k1[r] = cur
    assert k1.max() < P and k0.max() < P
    return [k0, k1]


def _random_case(seed, po2, zk, shapes):
    """one record per (L, nl) of `shapes`, the kinds in turn (LIMBS, ORDER by one key, ORDER by two), sources in code and data, about one
    raw source word in twenty >= P, everything else — the destinations and the blinding rows included — random words
    -> (desc, blob, code, data)"""
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    code, data = rand_fp(rng, WC, n), rand_fp(rng, WD, n)
    groups = {GROUP_CODE: code, GROUP_DATA: data}
    nc, nd = iter(range(3, WC)), iter(range(WD - 1))
    b = logup.LogupBuilder((4, WC, WD), (4, 8))
    b.term(0, [(GROUP_DATA, WD - 1)], tag=1)
    for i, (L, nl) in enumerate(shapes):
        bits = L * nl
        kind = (seed + i) % 3
        if kind == 2 and nl > 7:
            kind = 0
        pick = lambda: (GROUP_DATA, next(nd)) if rng.random() < 0.6 else (GROUP_CODE, next(nc))
        if kind == 0:
            srcs = [pick()]
            vals = [rng.integers(0, min(P, 1 << bits), A)]
            vals[0][rng.integers(0, A)] = min(P, 1 << bits) - 1              # the largest value that fits
        else:
            srcs = [pick() for _ in range(kind)]
            vals = _sorted_keys(rng, A, bits, kind == 2)
        for (g, c), v in zip(srcs, vals):
            groups[g][c, :A] = _enc(v)
            big = (rng.random(A) < 0.05) & (groups[g][c, :A].astype(np.uint64) + P < 1 << 32)
            groups[g][c, :A][big] += np.uint32(P)                            # the same residue as a raw word >= P
        dsts = [next(nd) for _ in range(nl + (kind == 2))]
        if kind == 0:
            b.derive_limbs(srcs[0], dsts, L)
        else:
            b.derive_order(srcs, dsts, L)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code.reshape(-1), data.reshape(-1)


def test_random_records_match_the_reference(hal):
    seen, kinds, big_words = set(), set(), 0
    for i, (po2, zk) in enumerate(GRID):
        shapes = [SHAPES[(PER_CASE * i + j) % len(SHAPES)] for j in range(PER_CASE)]
        desc, blob, code, data = _random_case(7 * i + 1, po2, zk, shapes)
        args = logup.Arguments.parse(blob)
        assert len(args.records) == PER_CASE
        for r in args.records:
            seen.add((r.limb_bits, r.nl)); kinds.add((r.kind, r.n_src, r.srcs[0][0]))
        n, A = 1 << po2, (1 << po2) - zk
        big_words += int((code.reshape(-1, n)[:, :A] >= P).sum() + (data.reshape(-1, n)[:, :A] >= P).sum())
        c = _circuit(hal, desc, blob)
        assert c.derives_columns() and not c.derives_sorted() and not c.derives_multiplicities()
        assert c.derived_data_columns() == sorted(x for r in args.records for x in r.dsts)
        want = logup.reference_columns(args, po2, zk, code, data)
        dcode, ddata = _upload(hal, code, data)
        hal.prof_enable(True)
        hal.prof_reset()
        hal.derive_columns(c, po2, zk, dcode, ddata)
        names = {r["name"] for r in hal.prof_get() if r["calls"]}
        hal.prof_enable(False)
        assert {"columns_check", "columns_write"} <= names, names
        got = ddata.to_vec()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"po2 {po2} zk {zk}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
        assert not np.array_equal(got, data)                                 # the (poisoned) destinations were written
        assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])    # the blinding rows were not
        assert np.array_equal(dcode.to_vec(), code)
    assert seen == set(SHAPES) and {L for L, _ in seen} == set(range(1, 17)) and {nl for _, nl in seen} == set(range(1, 9))
    assert kinds == {(k, s, g) for k, s in ((1, 1), (2, 1), (2, 2)) for g in (GROUP_CODE, GROUP_DATA)}, kinds
    assert big_words > 1000


# ---- the chain on SYN-LOOKUP-ordered ----
def _ordered(shape):
    """-> (description, the blob with everything derived, the flag-free blob of the same arguments)"""
    desc, blob = syn_lookup.build_syn_lookup(shape, derive=True, sort=True, limbs=True, order=True)
    return desc, blob, logup.Arguments.parse(blob).plain().blob()


def _witnesses(shape, po2, zk, seed, addr_range):
    code, full, out = syn_lookup.witness(shape, po2, zk, seed=seed, addr_range=addr_range, order=True)
    _, bare, _ = syn_lookup.witness(shape, po2, zk, seed=seed, addr_range=addr_range, sort=False, count=False, limbs=False, order=False)
    return code, full, bare, out


@pytest.mark.parametrize("shape,po2,zk,addr_range", [(TINY, 8, 40, 16), (TINY, 10, 300, 1 << 12), (TINY, 12, 1994, 5), (MULTI, 12, 1994, 1 << 12)])
def test_the_chain_equals_the_host_made_witness_and_seals_alike(hal, oracle, shape, po2, zk, addr_range):
    desc, blob, plain = _ordered(shape)
    assert logup.Arguments.parse(plain).version == 1
    code, full, bare, out = _witnesses(shape, po2, zk, po2, addr_range)
    assert not np.array_equal(bare, full)
    c = _circuit(hal, desc, blob)
    assert c.derives_sorted() and c.derives_columns() and c.derives_multiplicities()
    dcode, ddata = _upload(hal, code, bare)
    hal.derive_sorted(c, po2, zk, dcode, ddata)
    hal.derive_columns(c, po2, zk, dcode, ddata)
    hal.derive_multiplicities(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), full)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out)
    host = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    assert np.array_equal(receipt.seal, host.seal)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


def test_native_session_derives_columns(hal, oracle):
    from zeth_amd.host import Session
    po2 = 12
    desc, blob, plain = _ordered(TINY)
    segs = [Segment(index=i, po2=po2, noise_seed=NOISE + i) for i in range(2)]
    wit = [_witnesses(TINY, po2, s.zk_cycles, 60 + i, 1 << 12) for i, s in enumerate(segs)]
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


def test_syn_lookup_full_at_po2_20_with_every_derivable_column_derived(hal, oracle):
    po2, zk = 20, zhal.ZK_CYCLES
    desc, blob = syn_lookup.build_syn_lookup(FULL, limbs=True, sort=True, derive=True)
    pdesc, pblob = syn_lookup.syn_lookup()
    assert np.array_equal(desc, pdesc)
    c = _circuit(hal, desc, blob)
    assert len(c.derived_data_columns()) == 87 - 19
    code, want, out = syn_lookup.witness(FULL, po2, zk, seed=21)
    bare = _strip(c, want, po2, zk)
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, bare, out)
    plain = _seal_host(hal, SegmentProver(hal, pdesc, arguments=pblob), seg, code, want, out)
    assert np.array_equal(receipt.seal, plain.seal)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is None


# ---- refusals ----
def _refused(hal, c, prover, po2, zk, code, data, out, want_msg):
    """derive_columns refuses with the reference's words and leaves the data as it was; nothing is sealed from that witness"""
    dcode, ddata = _upload(hal, code, data)
    if c.derives_sorted():
        hal.derive_sorted(c, po2, zk, dcode, ddata)
    before = ddata.to_vec()
    with pytest.raises(HalError, match=re.escape(want_msg)):
        hal.derive_columns(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), before)
    with pytest.raises(HalError, match=re.escape(want_msg)):
        _seal_host(hal, prover, Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE), code, data, out)


def test_refusals_leave_data_unchanged_and_seal_nothing(hal):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, plain = _ordered(TINY)
    args = logup.Arguments.parse(blob)
    c, prover = _circuit(hal, desc, blob), SegmentProver(hal, desc, arguments=blob)
    code, full, bare, out = _witnesses(TINY, po2, zk, 3, 1 << 12)
    # a word of 2^16 or more does not fit TINY's 4 limbs of 4 bits; of two such rows the lower is named
    bad = bare.reshape(-1, n).copy()
    bad[1, 700] = _enc(1 << 16)
    bad[1, 123] = _enc((1 << 16) + 5)
    bad[0, 500] = _enc(P - 1)                                                # record 0 comes before record 1, whatever the row
    msg = "record 0 at row 500: the value 2013265920 does not fit 4 limbs of 4 bits"
    with pytest.raises(logup.ReferenceError, match=re.escape(msg)):
        logup.reference_columns(args, po2, zk, code, logup.reference_sorted(args, po2, zk, code, bad.reshape(-1)))
    _refused(hal, c, prover, po2, zk, code, bad.reshape(-1), out, msg)
    bad[0, 500] = bare.reshape(-1, n)[0, 500]
    _refused(hal, c, prover, po2, zk, code, bad.reshape(-1), out, "record 1 at row 123: the value 65541 does not fit 4 limbs of 4 bits")
    # a host-filled copy that is a permutation but not sorted (the memory tuple as it is), under the ORDER record
    hdesc, hblob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, order=True)
    hargs = logup.Arguments.parse(hblob)
    assert np.array_equal(hdesc, desc) and len(hargs.records) == 3 and not any(t.sorted_from is not None for t in hargs.terms)
    _w, _l, _m, mem, perm = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)
    unsorted = bare.reshape(-1, n).copy()
    unsorted[perm[0], :A] = unsorted[mem[0], :A]
    with pytest.raises(logup.ReferenceError) as e:
        logup.reference_columns(hargs, po2, zk, code, unsorted.reshape(-1))
    assert re.fullmatch(r"record 2 at row \d+: not ordered \(difference -\d+\)", str(e.value))
    _refused(hal, _circuit(hal, hdesc, hblob), SegmentProver(hal, hdesc, arguments=hblob), po2, zk, code, unsorted.reshape(-1), out, str(e.value))
    # a difference that is in order but too wide for the limbs: addresses up to 2^20 against 12 bits
    wcode, wide, wout = _witnesses_wide(po2, zk)
    with pytest.raises(logup.ReferenceError) as e:
        logup.reference_columns(args, po2, zk, wcode, logup.reference_sorted(args, po2, zk, wcode, wide))
    assert re.fullmatch(r"record 2 at row \d+: the difference \d+ does not fit 3 limbs of 4 bits", str(e.value))
    _refused(hal, c, prover, po2, zk, wcode, wide, wout, str(e.value))
    # a circuit without records is an error, not a no-op
    dcode, ddata = _upload(hal, code, full)
    with pytest.raises(HalError, match="hold no derived-column record"):
        hal.derive_columns(_circuit(hal, desc, plain), po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), full)


def _witnesses_wide(po2, zk):
    """SYN-LOOKUP-ordered TINY with addresses far beyond its 12 order bits: the plain witness generator, widened by zero order columns"""
    n = 1 << po2
    code, data, out = syn_lookup.witness(TINY, po2, zk, seed=8, sort=False, count=False, limbs=False, addr_range=1 << 20)
    wide = np.concatenate([data.reshape(-1, n), rand_fp(np.random.default_rng(8), 4, n)])
    return code, wide.reshape(-1), out


# ---- a forged order witness ----
def test_a_forged_order_witness_yields_no_accepted_seal(hal, oracle):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, plain = _ordered(TINY)
    code, full, _bare, out = _witnesses(TINY, po2, zk, 11, 16)
    row = A // 2
    d = syn_lookup.swap_sorted_rows(TINY, full, po2, row).reshape(-1, n)
    perm = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[4][0]
    flag, *limbs = syn_lookup.order_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0]
    k0, k1 = logup._dec(d[perm[0], :A]).astype(np.int64), logup._dec(d[perm[2], :A]).astype(np.int64)
    same = np.concatenate([[0], (k0[1:] == k0[:-1]).astype(np.int64)])
    diff = np.concatenate([[0], np.where(same[1:] == 1, k1[1:] - k1[:-1], k0[1:] - k0[:-1] - 1)])
    assert (diff < 0).sum() == 1 and (np.abs(diff) < 1 << 12).all()          # the swap made exactly one step go back
    d[flag, :A] = _enc(same)
    for j, col in enumerate(limbs):                                          # in-range limbs of the absolute difference
        d[col, :A] = _enc((np.abs(diff) >> (4 * j)) & 15)
    m = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[2]
    d[m, :A] = 0
    counted = logup.Arguments.parse(syn_lookup.build_syn_lookup(TINY, derive=True, order=True)[1])
    forged = logup.reference_multiplicities(counted, po2, zk, code, d.reshape(-1))          # ... and counted multiplicities
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    _, total = logup.reference_accumulate(logup.Arguments.parse(plain), po2, zk, code, forged, mix)
    assert total == [0, 0, 0, 0]                                             # every lookup is answered and the bus balances
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    try:
        receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, forged, out)
    except HalError:
        return                                                               # no seal at all
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    with pytest.raises(HalError):
        receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is not None
    # the honest witness under the same blob is accepted: the rejection is the order constraints'
    honest = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    honest.verify(desc, root)


# ---- the sparse upload ----
def test_only_what_the_library_cannot_derive_is_uploaded(hal):
    po2, zk = 16, zhal.ZK_CYCLES
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob = syn_lookup.build_syn_lookup(FULL, limbs=True, sort=True, derive=True)
    c = _circuit(hal, desc, blob)
    derived = c.derived_data_columns()
    assert len(derived) == 68 and int(desc[5]) == 87
    code, want, out = syn_lookup.witness(FULL, po2, zk, seed=16)
    bare = _strip(c, want, po2, zk)
    seg = Segment(index=0, po2=po2, noise_seed=NOISE)
    prover = SegmentProver(hal, desc, arguments=blob)
    hcode, hdata = hal.host_alloc(code.size), hal.host_alloc(bare.size)
    hcode[:] = code
    hdata[:] = bare
    try:
        before = hal.h2d_bytes()
        first = prover.seal_host_witness(seg, hcode, hdata, out)
        hal.sync()
        crossed = hal.h2d_bytes() - before
        # the garbage a host may leave in what the library derives never crosses, so it changes no seal byte
        hdata[:] = _strip(c, want, po2, zk, fill=0x12345678)
        second = prover.seal_host_witness(seg, hcode, hdata, out)
        hal.sync()
    finally:
        hal.host_free(hcode)
        hal.host_free(hdata)
    trace = 4 * ((87 - 68) * n + 68 * zk) + 4 * code.size
    # what a seal uploads besides its traces — challenges, globals and the prover's own small tables — is what the plain circuit's seal
    # of the whole host-made witness uploads besides its traces, counted here in the same way ...
    before = hal.h2d_bytes()
    pdesc, pblob = syn_lookup.syn_lookup()
    plain = _seal_host(hal, SegmentProver(hal, pdesc, arguments=pblob), seg, code, want, out)
    other = hal.h2d_bytes() - before - 4 * (want.size + code.size)
    # ... plus the records and terms as the three derives' kernels read them: 16 records of 18 words, one entry of 13 words and one list
    # word per term (67) for the multiplicities, one pair of 22 words and 10 status words for the sort
    tables = 4 * (16 * 18 + 67 * 14 + 32)
    print(f"h2d bytes across one seal: {crossed} = traces {trace} + {crossed - trace}; the plain seal: traces {4 * (want.size + code.size)} + {other}; "
          f"room for the derives' tables: {tables}")
    assert 0 <= other < 1 << 16                                              # words, not columns of rows
    assert trace <= crossed <= trace + other + tables
    assert np.array_equal(first.seal, second.seal)
    assert np.array_equal(first.seal, plain.seal)
    # the helper by itself, from memory that is not pinned: the same columns, then the derives complete the trace
    ddata = hal.alloc("data", want.size, zero=True)
    before = hal.h2d_bytes()
    hal.upload_data_trace(c, po2, zk, ddata, bare, pinned_async=False)
    assert hal.h2d_bytes() - before == 4 * ((87 - 68) * n + 68 * zk)
    assert np.array_equal(ddata.to_vec(), bare)
    with pytest.raises(HalError, match="not inside a zkh_host_alloc block"):
        hal.upload_data_trace(c, po2, zk, ddata, bare, pinned_async=True)
