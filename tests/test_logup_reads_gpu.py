"""The read rule on the GPU (zkh_derive_links under a ZKA1 version-6 blob, csrc/links.hip): a load returns the last store.  Random
load / store traces at three sizes (A = 216: no multiple of a wave; 2102; 6198: past one 4096-item sort tile) over the key patterns that
can break the rule — one address for every access (one chain through every wave and tile boundary: at po2 13 the load at sorted
position 4096 is compared with position 4095), five addresses, a sparse selector, distinct addresses (every load is unlinked, so every
load is 0, a third of the zeros written as the raw word P), raw words >= P next to their residues in the value columns, and two records
of which one has READS (nc = 3) and one has not (nc = 2): the destinations equal the host reference word for word and what the
version-5 blob derives from the same trace (the rule adds no output).  The refusals — a planted bad load at a wave boundary, at sorted
position 4096, an unlinked one, in the second value column at nc = 3; a flag of 2; two bad rows in two records; a row bad in clock and
value — carry the reference's message, leave `data` unchanged and seal nothing.  The chain columns -> links -> multiplicities on
SYN-LOOKUP-reads seals byte-identically to the host-made witness under the plain blob, and a forged load (syn_lookup.misread_row),
host-made and uploaded under the plain blob, yields no accepted seal on SYN-LOOKUP-reads while the same values seal and verify on
SYN-LOOKUP-linked.

Mutants these cases catch (never committed):
  * the previous value taken from sorted position j + 1: every honest trace with a linked load is refused (`equal`, `range5`, ... of
    test_reads_match_the_reference);
  * the rule skipped at the first item of a 4096-item sort tile: `tile` of test_a_bad_load_is_refused, the load at sorted position 4096;
  * raw words compared instead of residues: `big` and `distinct` of test_reads_match_the_reference are refused (a load P + v of a store
    v; a zero written as P);
  * unlinked loads not checked: `unlinked` of test_a_bad_load_is_refused is accepted;
  * only the first value column checked: `second` of test_a_bad_load_is_refused is accepted."""
import re
from dataclasses import replace

import numpy as np
import pytest

from args_gpu import circuit as _circuit, enc as _enc, links_refused, profiled, seal_host as _seal_host, upload as _upload
import zko
from conftest import rand_fp
from zeth_amd.circuits import logup, syn_lookup
from zeth_amd.circuits.desc import GROUP_CODE, GROUP_DATA
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver

pytestmark = pytest.mark.gpu
P = 2013265921
NOISE = 0x0C06
ONE = (1 << 32) % P
TINY = syn_lookup.TINY
SIZES = [(8, 40), (12, 1994), (13, 1994)]
WC, PER_REC = 8, 13                             # code columns; data columns per record: key, clock, value, 9 destinations, the write flag


def _without_reads(blob):
    """the version-5 blob of the same arguments: every LINK record without READS"""
    a = logup.Arguments.parse(blob)
    recs = [replace(r, write=None) if isinstance(r, logup.Link) else r for r in a.records]
    return logup.Arguments(a.k, a.alpha, a.beta, a.terms, recs).blob()


def _case(kind, seed, po2, zk):
    """-> (desc, blob, code, data) as (columns, n) arrays: a random load / store trace (destinations and blinding rows poisoned) under
    one LINK record with READS (nc = 2: the clock and one value; 3 limbs of 8 bits), or for `two` under record 0 with READS (nc = 3: the
    second value the code column 7; 4 limbs of 5 bits) and record 1 without (nc = 2, its values random).  The clock of an access is that
    of the previous access to its key plus a step, so every difference fits the limbs.  Every access draws a write flag; a load takes
    the values the previous access to its key left, or zeros"""
    rng = np.random.default_rng(seed)
    n, A = 1 << po2, (1 << po2) - zk
    n_rec = 2 if kind == "two" else 1
    wd = PER_REC * n_rec + 1
    code, data = rand_fp(rng, WC, n), rand_fp(rng, wd, n)
    b = logup.LogupBuilder((4, WC, wd), (4, 8))
    b.term(0, [(GROUP_DATA, wd - 1)], tag=1)
    for i in range(n_rec):
        base = PER_REC * i
        reads = i == 0
        L, nl, nc = ((5, 4, 3) if reads else (8, 3, 2)) if kind == "two" else (8, 3, 2)
        sel = 3 + i if kind in ("sparse", "two") else None
        if kind == "equal":
            keys = np.full(A, 77777, dtype=np.int64)
        elif kind == "distinct":
            keys = rng.permutation(A).astype(np.int64) * 3 + 1
        else:
            keys = rng.integers(0, 5, A).astype(np.int64)
        on = rng.random(A) < 0.3 if sel is not None else np.ones(A, dtype=bool)
        if sel is not None:
            code[sel, :A] = _enc(on.astype(np.uint64))
        step = int(rng.integers(1, 40))
        store = rng.random(A) < 0.5
        vals = [data[base + 2], code[7]][:nc - 1]
        seen, held, clock = {}, {}, np.zeros(A, dtype=np.int64)
        for r in np.nonzero(on)[0]:
            k = int(keys[r])
            clock[r] = seen.get(k, int(rng.integers(0, 1000))) + (step if k in seen else 0)
            seen[k] = int(clock[r])
            if reads:
                if not store[r]:
                    for v, h in zip(vals, held.get(k, [0] * len(vals))):
                        v[r] = h
                held[k] = [int(v[r]) for v in vals]
        clock[~on] = rng.integers(0, P, int((~on).sum()))
        data[base, :A] = _enc(keys)
        data[base + 1, :A] = _enc(clock)
        data[base + 12, :A] = _enc(store.astype(np.uint64))
        if kind == "distinct":                                               # every load is a zero: a third of them as the raw word P
            zero = on & ~store & (rng.random(A) < 0.33)
            data[base + 2, :A][zero] = np.uint32(P)
        if kind in ("big", "two"):                                           # about a third of the cells as raw words >= P
            for col in [data[base], data[base + 1], data[base + 12]] + (vals if reads else []):
                col[:A][rng.random(A) < 0.3] += np.uint32(P)
        carried = [(GROUP_DATA, base + 1), (GROUP_DATA, base + 2), (GROUP_CODE, 7)][:nc]
        b.derive_links(sel, (GROUP_DATA, base), carried, list(range(base + 3, base + 3 + 2 + nc + nl)), L,
                       write=(GROUP_DATA, base + 12) if reads else None)
    desc, blob = b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2)))
    return desc, blob, code, data


KINDS = ["equal", "range5", "sparse", "distinct", "big", "two"]


@pytest.mark.parametrize("po2,zk", SIZES)
def test_reads_match_the_reference(hal, po2, zk):
    n, A = 1 << po2, (1 << po2) - zk
    for i, kind in enumerate(KINDS):
        desc, blob, code, data = _case(kind, 100 * po2 + i, po2, zk)
        code, data = code.reshape(-1), data.reshape(-1)
        args = logup.Arguments.parse(blob)
        blob5 = _without_reads(blob)
        assert args.version == 6 and int(blob[7]) == 1 and int(blob5[1]) == 5 and len(args.records) == (2 if kind == "two" else 1)
        c = _circuit(hal, desc, blob)
        assert c.derives_links() and c.links_check_reads() == 1
        assert c.derived_data_columns() == sorted(x for r in args.records for x in r.dsts)       # the write flag is the host's
        want = logup.reference_links(args, po2, zk, code, data)
        w = want.reshape(-1, n)
        r0 = args.records[0]
        sel = np.ones(A, dtype=bool) if r0.sel is None else code.reshape(-1, n)[r0.sel, :A] == ONE
        load = sel & (data.reshape(-1, n)[r0.write[1], :A] % P == 0)
        linked = w[r0.linked, :A] == ONE
        assert load.sum() > sel.sum() // 4
        if kind == "distinct":
            assert not linked.any() and (data.reshape(-1, n)[2, :A][load] == P).sum() > load.sum() // 6
        else:
            assert (load & linked).sum() > sel.sum() // 4
        dcode, ddata = _upload(hal, code, data)
        prof = profiled(hal, lambda: hal.derive_links(c, po2, zk, dcode, ddata))
        assert {"sort_keys", "sort_pack", "links_check", "links_write"} <= set(prof), set(prof)
        got = ddata.to_vec()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{kind} po2 {po2}: {bad.size} words differ, first at column {bad[0] // n}, row {bad[0] % n}"
        assert not np.array_equal(got, data)                                 # the (poisoned) destinations were written
        assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])    # the blinding rows were not
        assert np.array_equal(dcode.to_vec(), code)
        c5 = _circuit(hal, desc, blob5)                                      # the rule adds no output: the version-5 blob derives the same
        assert c5.links_check_reads() == 0
        ddata.write(data)
        hal.derive_links(c5, po2, zk, dcode, ddata)
        assert np.array_equal(ddata.to_vec(), want)


# ---- refusals ----
def _refused(hal, desc, blob, po2, zk, code, data, want_msg, seal=True):
    links_refused(hal, desc, blob, po2, zk, code, data, want_msg, seal=seal)


def _store_then_bad_load(data, row, value=4242):
    """`equal` (every row an access to the one address, sorted position = row): row - 1 stores `value`, `row` loads value + 1, and row + 1
    stores, so that no other row objects -> the message's tail"""
    data[12, row - 1], data[12, row], data[12, row + 1] = ONE, 0, ONE
    data[2, row - 1], data[2, row] = _enc(value), _enc(value + 1)
    return f"a load of carried column 1 returns {value + 1}, but {value} was last stored (row {row - 1})"


@pytest.mark.parametrize("where", ["wave", "tile", "unlinked", "second"])
def test_a_bad_load_is_refused(hal, where):
    if where in ("wave", "tile"):                                            # one chain: the load at sorted position 64 / 4096 against 63 / 4095
        po2, zk = (8, 40) if where == "wave" else (13, 1994)
        row = 64 if where == "wave" else 4096
        desc, blob, code, data = _case("equal", 5, po2, zk)
        msg = f"record 0 at row {row}: " + _store_then_bad_load(data, row)
    elif where == "unlinked":                                                # a load of an address never accessed that returns 5
        po2, zk = 8, 40
        desc, blob, code, data = _case("distinct", 6, po2, zk)
        row = 131
        data[12, row], data[2, row] = 0, _enc(5)
        msg = f"record 0 at row {row}: a load of carried column 1 returns 5, but its address was never accessed: the value must be 0"
    else:                                                                    # nc = 3: the first value column holds, the second does not
        po2, zk = 12, 1994
        desc, blob, code, data = _case("two", 7, po2, zk)
        n, A = 1 << po2, (1 << po2) - zk
        w = logup.reference_links(logup.Arguments.parse(blob), po2, zk, code.reshape(-1), data.reshape(-1)).reshape(-1, n)
        row = next(r for r in range(A // 2, A) if code[3, r] == ONE and data[12, r] % P == 0 and w[3, r] == ONE)      # a linked load
        prow = max(r for r in range(row) if code[3, r] == ONE and data[0, r] % P == data[0, row] % P)
        before = int(logup._dec(code[7, prow]))
        code[7, row] = _enc(before + 1)
        msg = f"record 0 at row {row}: a load of carried column 2 returns {(before + 1) % P}, but {before} was last stored (row {prow})"
    _refused(hal, desc, blob, po2, zk, code, data, msg)
    # the same trace under the version-5 blob has no read rule: it derives
    c5 = _circuit(hal, desc, _without_reads(blob))
    dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
    hal.derive_links(c5, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), logup.reference_links(logup.Arguments.parse(_without_reads(blob)), po2, zk, code.reshape(-1), data.reshape(-1)))


def test_refusals_name_the_lowest_record_and_row_and_the_first_rule(hal):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, code, data = _case("two", 9, po2, zk)                        # record 0: READS, selector code 3, nc = 3; record 1: selector code 4
    on0 = np.nonzero(code[3, :A] == ONE)[0]
    k0 = logup._dec(data[0, :A])
    chain = [int(r) for r in on0 if k0[r] == k0[on0[5]] and r > 300]         # accesses of record 0 to one address, in row order, one after another
    assert len(chain) >= 6
    dec = lambda v: int(logup._dec(np.uint32(v)))
    # a flag of 2 (as a raw word >= P)
    d = data.copy()
    d[12, chain[2]] = _enc(2) + np.uint32(P)
    _refused(hal, desc, blob, po2, zk, code, d, f"record 0 at row {chain[2]}: write flag 2, not 0 or 1")
    # a bad load: chain[1] stores, chain[2] loads another value, chain[3] stores
    d = data.copy()
    d[12, chain[1]], d[12, chain[2]], d[12, chain[3]] = ONE, 0, ONE
    c = code.copy()
    c[7, chain[2]] = c[7, chain[1]]
    d[2, chain[2]] = (int(d[2, chain[1]]) % P + ONE) % P
    v = dec(d[2, chain[1]])
    msg = f"record 0 at row {chain[2]}: a load of carried column 1 returns {(v + 1) % P}, but {v} was last stored (row {chain[1]})"
    _refused(hal, desc, blob, po2, zk, c, d, msg, seal=False)
    # two bad rows in two records: record 1 (no READS) has a clock that does not increase at a lower row, record 0 is named
    on1 = np.nonzero(code[4, :A] == ONE)[0]
    k1 = logup._dec(d[PER_REC, :A])
    chain1 = [int(r) for r in on1 if k1[r] == k1[on1[0]]]                    # ... and of record 1, from its first access on
    assert chain1[1] < chain[2]
    d[PER_REC + 1, chain1[1]] = d[PER_REC + 1, chain1[0]]
    _refused(hal, desc, blob, po2, zk, c, d, msg, seal=False)
    # ... and alone record 1's clock is what is named: clock and read-rule refusals are reduced together
    t = dec(d[PER_REC + 1, chain1[0]])
    d1 = data.copy()
    d1[PER_REC + 1, chain1[1]] = d1[PER_REC + 1, chain1[0]]
    _refused(hal, desc, blob, po2, zk, code, d1, f"record 1 at row {chain1[1]}: clock not increasing ({t} after {t} at row {chain1[0]})", seal=False)
    # of two bad rows of one record the lower
    d[12, chain[4]], d[12, chain[5]] = ONE, 0
    d[2, chain[5]] = (int(d[2, chain[4]]) % P + ONE) % P
    _refused(hal, desc, blob, po2, zk, c, d, msg, seal=False)
    # a row bad in both clock and value: the clock message; with a flag that is no flag on top: the flag's
    d[1, chain[2]] = d[1, chain[1]]
    t = dec(d[1, chain[1]])
    _refused(hal, desc, blob, po2, zk, c, d, f"record 0 at row {chain[2]}: clock not increasing ({t} after {t} at row {chain[1]})")
    d[12, chain[2]] = _enc(P - 1)
    _refused(hal, desc, blob, po2, zk, c, d, f"record 0 at row {chain[2]}: write flag {P - 1}, not 0 or 1", seal=False)
    # selectors still come first, over all records
    c[4, 650] = _enc(2)
    _refused(hal, desc, blob, po2, zk, c, d, "record 1 at row 650: selector 2, not 0 or 1", seal=False)


# ---- the chain on SYN-LOOKUP-reads ----
def _reads(shape):
    """-> (description, the blob with everything derived, the flag-free blob of the same arguments)"""
    desc, blob = syn_lookup.build_syn_lookup(shape, derive=True, limbs=True, link=True, reads=True)
    return desc, blob, logup.Arguments.parse(blob).plain().blob()


@pytest.mark.parametrize("po2,zk,addr_range", [(8, 40, 16), (12, 1994, 5), (13, 1994, 64)])
def test_the_chain_equals_the_host_made_witness_and_seals_alike(hal, oracle, po2, zk, addr_range):
    desc, blob, plain = _reads(TINY)
    assert logup.Arguments.parse(plain).version == 1 and logup.Arguments.parse(blob).version == 6
    code, full, out = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=addr_range, link=True, reads=True)
    _, bare, _ = syn_lookup.witness(TINY, po2, zk, seed=po2, addr_range=addr_range, count=False, limbs=False, link=False, reads=True)
    assert not np.array_equal(bare, full)
    c = _circuit(hal, desc, blob)
    assert c.derives_links() and c.links_check_reads() == 1 and c.derives_columns() and c.derives_multiplicities() and not c.derives_sorted()
    assert syn_lookup.reads_layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[0] not in c.derived_data_columns()
    dcode, ddata = _upload(hal, code, bare)
    hal.derive_columns(c, po2, zk, dcode, ddata)
    hal.derive_links(c, po2, zk, dcode, ddata)
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


# ---- a forged load ----
def test_a_forged_load_yields_no_accepted_seal(hal, oracle):
    po2, zk = 10, 300
    n, A = 1 << po2, (1 << po2) - zk
    desc, blob, plain = _reads(TINY)
    code, full, out = syn_lookup.witness(TINY, po2, zk, seed=12, addr_range=16, link=True, reads=True)
    forged, row = syn_lookup.misread_row(TINY, full, po2, zk)
    assert not np.array_equal(forged, full)
    m = syn_lookup.layout(TINY.n_words, TINY.n_limbs, TINY.n_mem)[2]
    d = forged.reshape(-1, n).copy()
    d[m, :A] = 0
    forged = logup.reference_multiplicities(logup.Arguments.parse(blob), po2, zk, code, d.reshape(-1))      # the multiplicities counted again
    mix = np.random.default_rng(2).integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    _, total = logup.reference_accumulate(logup.Arguments.parse(plain), po2, zk, code, forged, mix)
    assert total == [0, 0, 0, 0]                                             # every lookup is answered and the bus balances
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    # the same forged values on SYN-LOOKUP-linked, which has no read rule, seal and verify
    ldesc, lblob = syn_lookup.build_syn_lookup(TINY, derive=True, limbs=True, link=True)
    lplain = logup.Arguments.parse(lblob).plain().blob()
    same = np.ascontiguousarray(forged.reshape(-1, n)[:21]).reshape(-1)
    lc = zko.OracleCircuit(oracle, ldesc)
    lroot = lc.root_of_code(po2, code)
    accepted = _seal_host(hal, SegmentProver(hal, ldesc, arguments=lplain), seg, code, same, out)
    accepted.verify(ldesc, lroot)
    assert lc.verify(accepted.seal, lroot) is None
    # on SYN-LOOKUP-reads the honest witness under the plain blob is accepted, the forged one is not
    honest = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, full, out)
    oc = zko.OracleCircuit(oracle, desc)
    root = oc.root_of_code(po2, code)
    honest.verify(desc, root)
    with pytest.raises(HalError, match=re.escape(f"at row {row}: a load of carried column 1 returns")):     # with the derive, the library refuses it
        _seal_host(hal, SegmentProver(hal, desc, arguments=blob), seg, code, forged, out)
    try:
        receipt = _seal_host(hal, SegmentProver(hal, desc, arguments=plain), seg, code, forged, out)
    except HalError:
        return                                                               # no seal at all
    with pytest.raises(HalError):
        receipt.verify(desc, root)
    assert oc.verify(receipt.seal, root) is not None
