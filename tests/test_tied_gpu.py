"""THE TIE on the GPU (csrc/accumulate.hip zkh_accumulate_open, csrc/tie.hip zkh_table_fingerprint, zkh_data_root,
zkh_seal_data_root; prover.seal_tied / verify_tied).  The open accumulate word for word against the reference on the tiny tied segment
and on a P2-PAGE-tied part, with its total, and the closed and the open call refusing each other's blobs; the table's fingerprint against
the plain-Python sum at every row count at which the kernel takes another path, on residues 0 and P - 1, inside a real ZKU1 proof, and
its refusal of vanishing denominators; the data root of a trace against the root read out of its seal; and one tied group end to end
with its forgeries.

Shapes.  The segment: SYN-LOOKUP-tied's tiny shape at (po2 8, zk 40) over 40 addresses (few addresses, many accesses each) and at (po2
12, zk 1994) over a whole image of 1000 words (two workgroups of every row kernel).  The part: page_ordered_cases' h = 5 shape.  The
fingerprint: a lane's run is 4 rows, a workgroup's 1024; 3 workgroups and 5 rows is the ragged tail.  End to end: the segment at po2 8
over an image of 64 words, its page-out in three parts of 22 slots at po2 12, the last with dead slots."""
import re

import numpy as np
import pytest

import page_circuit_cases as cases
import page_ordered_cases as oc
import tied_cases as host
from args_gpu import circuit, image_buf, upload
from zeth_amd import hal as zhal
from zeth_amd.circuits import logup, p2_page_tied as T, syn_lookup as sl
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, seal_tied, verify_tied

pytestmark = pytest.mark.gpu
P = host.P
ONE = host.ONE
NOISE = 0x71ED
CHALLENGE = host.CHALLENGE
H5 = cases.SHAPES[1]
LANE_RUN, GROUP_RUN = 4, 1024


def _noise(seed, po2, zk):
    """the accum group's blinding rows as the library draws them: noise(column) -> rows [A, n)"""
    key, lib = zhal.noise_key(seed), zhal.load_library()
    n, A = 1 << po2, (1 << po2) - zk
    return lambda col: np.array([lib.zkh_noise_cell_host(zhal._ptr(key), 0, col, r) for r in range(A, n)], dtype=np.uint32)


def _open_against_the_reference(hal, desc, blob, po2, zk, code, data):
    c = circuit(hal, desc, blob)
    args = logup.Arguments.parse(blob)
    dcode, ddata = upload(hal, np.ascontiguousarray(code).reshape(-1), np.ascontiguousarray(data).reshape(-1))
    accum = hal.alloc_elem("accum", 4 * args.k << po2)
    total = hal.accumulate_open(c, po2, zk, NOISE, dcode, ddata, CHALLENGE, accum)
    want, want_total = logup.reference_accumulate(args, po2, zk, code, data, CHALLENGE, noise=_noise(NOISE, po2, zk))
    got = accum.to_vec()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} accum words differ, the first at (column, row) {divmod(int(bad[0]), 1 << po2)}"
    assert np.array_equal(total, host.enc(want_total)) and total.any()
    return c, dcode, ddata, accum, total


@pytest.mark.parametrize("po2,zk,addr_range", [(8, 40, 40), (12, 1994, 1000)], ids=["8-40-sparse", "12-1994-wide"])
def test_accumulate_open_is_the_reference_on_the_tiny_tied_segment(hal, po2, zk, addr_range):
    desc, blob = sl.syn_lookup_tiny_tied()
    image = np.random.default_rng(po2).integers(1, P, 1000, dtype=np.uint64).astype(np.uint32)
    code, data, _ = sl.witness(sl.TINY, po2, zk, seed=po2, link=True, reads=True, pages=True, image=image, addr_range=addr_range)
    c, dcode, ddata, accum, total = _open_against_the_reference(hal, desc, blob, po2, zk, code, data)
    # the witness with `out` = 0 ‖ challenge ‖ total satisfies the circuit's own constraints on the device, and with the total off by one
    # only the `last` row objects
    out = np.concatenate([np.zeros(4, dtype=np.uint32), CHALLENGE, total])
    mix = np.zeros(8, dtype=np.uint32)
    assert hal.check_rows(c, po2, accum, dcode, ddata, out, mix)["row"] == -1
    out[sl.OUT_TOTAL + 3] = (int(out[sl.OUT_TOTAL + 3]) + 1) % P
    found = hal.check_rows(c, po2, accum, dcode, ddata, out, mix)
    assert (found["row"], found["failing_rows"]) == ((1 << po2) - zk - 1, 1)
    # the bus check skips the open tag's keys: every other key balances
    assert hal.check_bus(c, po2, zk, dcode, ddata)["row"] == -1


def test_accumulate_open_is_the_reference_on_a_tied_part(hal):
    po2, zk, W = H5
    t = oc.table(po2, zk, W, "2N+3")
    for first in (0, 26):                                                         # a full part, and the last with its dead slots
        data, _, code = oc.part(po2, zk, W, "2N+3", first)
        _, _, _, _, total = _open_against_the_reference(hal, T.p2_page_tied_circuit(), T.arguments(), po2, zk, code, data)
        rows = t["table"][first:first + t["N"]]
        assert not host.f4_add(total, logup.table_fingerprint(rows, CHALLENGE[:4], CHALLENGE[4:])).any()


def test_the_closed_and_the_open_call_refuse_each_others_blobs(hal):
    po2, zk = 8, 40
    image = np.random.default_rng(1).integers(1, P, 100, dtype=np.uint64).astype(np.uint32)
    code, data, _ = sl.witness(sl.TINY, po2, zk, seed=1, link=True, reads=True, pages=True, image=image)
    dcode, ddata = upload(hal, code, data)
    tied, paged = circuit(hal, *sl.syn_lookup_tiny_tied()), circuit(hal, *sl.syn_lookup_tiny_paged())
    assert tied.open_bus() == (logup.TIE_TAG, 4, 8, 12) and paged.open_bus() is None
    accum = hal.alloc_elem("accum", 32 << po2)
    with pytest.raises(HalError, match=r"^accumulate: the arguments are an open bus \(ZKA1 version 8\).*\(zkh_accumulate_open\)$"):
        hal.accumulate(tied, po2, zk, NOISE, dcode, ddata, np.zeros(8, dtype=np.uint32), accum)
    with pytest.raises(HalError, match=r"^accumulate_open: the arguments are a closed bus \(no OPEN record\).*\(zkh_accumulate\)$"):
        hal.accumulate_open(paged, po2, zk, NOISE, dcode, ddata, CHALLENGE, accum)
    bad = CHALLENGE.copy()
    bad[5] = P
    with pytest.raises(HalError, match="^accumulate_open: challenge word 5 is not a reduced element$"):
        hal.accumulate_open(tied, po2, zk, NOISE, dcode, ddata, bad, accum)
    assert hal.accumulate_open(tied, po2, zk, NOISE, dcode, ddata, CHALLENGE, accum).any()      # the good call right after them


# ------------------------------------------------------------------------------------------------ the fingerprint
def _table(rng, D):
    rows = np.empty((D, 3), dtype=np.uint32)
    rows[:, 0] = np.sort(rng.choice(1 << 29, D, replace=False)) if D else 0
    rows[:, 1:] = rng.integers(0, P, (D, 2), dtype=np.uint64)
    return rows


ROW_COUNTS = [0, 1, LANE_RUN - 1, LANE_RUN, LANE_RUN + 1, GROUP_RUN + 1, 3 * GROUP_RUN + 5]


@pytest.mark.parametrize("D", ROW_COUNTS)
def test_the_fingerprint_is_the_plain_sum_at_every_row_count(hal, D):
    rows = _table(np.random.default_rng(D), D)
    if D > 2:
        top = int(host.enc(P - 1))
        rows[1, 1:], rows[2, 1:] = (top, 0), (0, top)                             # residues P - 1 and 0, as Montgomery words
    at = 7                                                                        # not at the start of its buffer
    buf = hal.copy_from("table", np.concatenate([np.full(at, 0xdeadbeef, dtype=np.uint32), rows.reshape(-1), np.full(5, 0xdeadbeef, dtype=np.uint32)]))
    got = hal.table_fingerprint(buf, at, D, CHALLENGE)
    assert np.array_equal(got, logup.table_fingerprint(rows, CHALLENGE[:4], CHALLENGE[4:])) and got.any() == bool(D)


def test_the_fingerprint_reads_the_table_inside_a_real_proof_and_refuses_one_outside_its_buffer(hal):
    po2, zk, W = H5
    t = oc.table(po2, zk, W, "2N+3")
    before = hal.image_commit(image_buf(hal, t["image"]))
    proof = cases.host_proof(t["image"], t["addrs"], t["outs"], before.to_vec())
    D, h = int(proof[2]), int(proof[4])
    assert D == len(t["table"]) and h == 5
    buf = hal.copy_from("proof", proof)
    got = hal.table_fingerprint(buf, 5 + h, D, CHALLENGE)
    assert np.array_equal(got, logup.table_fingerprint(t["table"], CHALLENGE[:4], CHALLENGE[4:]))
    with pytest.raises(HalError, match=rf"^table_fingerprint: a table of {proof.size} rows at word 10 does not lie in a buffer of {proof.size} words$"):
        hal.table_fingerprint(buf, 5 + h, proof.size, CHALLENGE)
    with pytest.raises(HalError, match=rf"^table_fingerprint: a table of 1 rows at word {proof.size - 2} does not lie in a buffer of {proof.size} words$"):
        hal.table_fingerprint(buf, proof.size - 2, 1, CHALLENGE)


def test_the_fingerprint_refuses_the_lower_of_two_vanishing_denominators(hal):
    D = 2 * GROUP_RUN + 9
    rows = _table(np.random.default_rng(99), D)
    lo, hi = GROUP_RUN + 3, 2 * GROUP_RUN + 1                                     # in two workgroups
    rows[hi] = rows[lo]                                                           # the same row twice: one alpha makes both vanish
    dec = lambda w: [int(x) % P * pow(ONE, -1, P) % P for x in w]
    beta = dec(CHALLENGE[4:])
    b2 = logup._f4_mul(beta, beta)
    b3 = logup._f4_mul(b2, beta)
    a, vi, vo = int(rows[lo, 0]) % P, *dec(rows[lo, 1:])
    alpha = [(beta[e] * a + b2[e] * vi + b3[e] * vo + (logup.TIE_TAG if e == 0 else 0)) % P for e in range(4)]     # solved for that row
    challenge = np.concatenate([host.enc(alpha), CHALLENGE[4:]])
    buf = hal.copy_from("table", rows.reshape(-1))
    with pytest.raises(HalError, match=rf"^table_fingerprint: the denominator of row {lo} vanishes under this challenge: the table is refused$"):
        hal.table_fingerprint(buf, 0, D, challenge)
    with pytest.raises(logup.ReferenceError, match=f"the denominator of row {lo} vanishes"):
        logup.table_fingerprint(rows, challenge[:4], challenge[4:])
    assert hal.table_fingerprint(buf, 0, lo, challenge).any()                     # the rows below it are fine under the same challenge


# ------------------------------------------------------------------------------------------------ end to end
SEG_PO2, SEG_ZK, W = host.SEG_PO2, host.SEG_ZK, host.W
PAGE_PO2, PAGE_ZK = host.PAGE_PO2, host.PAGE_ZK


class Group:
    """one tied group on the device: the segment's traces derived from the image, the page-out's proof and trees, the provers"""

    def __init__(self, hal):
        s = host.segment()
        self.hal, self.desc, self.table = hal, s["desc"], s["table"]
        self.seg_prover = SegmentProver(hal, s["desc"], arguments=s["blob"])
        self.page_prover = SegmentProver(hal, T.p2_page_tied_circuit(), arguments=T.arguments())
        self.seg = Segment(index=0, po2=SEG_PO2, zk_cycles=SEG_ZK, noise_seed=NOISE)
        self.page_segs = [Segment(index=1 + p, po2=PAGE_PO2, zk_cycles=PAGE_ZK, noise_seed=NOISE + 1 + p) for p in range(3)]
        # the library derives the link columns and the page table from the image; the host left them zero
        code, bare, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=3, link=False, reads=True, pages=False, image=s["image"])
        self.host_code, self.host_data, self.host_image = code, bare, s["image"]
        self.code, self.data = self.traces(bare)
        self.image = image_buf(hal, s["image"])                                   # the page-out turns it, and its tree, into the image after
        self.after = hal.image_commit(self.image)
        self.proof, self.before = self.seg_prover.page_out(self.seg, self.data, self.image, tree=self.after, proof=True, keep_before=True)
        h = int(self.proof[4])
        assert [tuple(int(x) for x in row) for row in self.proof[5 + h:5 + h + 3 * int(self.proof[2])].reshape(-1, 3)] == self.table     # the host-made witness's
        self.root_before, self.root_after = hal.image_root(self.before), hal.image_root(self.after)

    def traces(self, host_data):
        c = self.seg_prover.circuit
        code, data = upload(self.hal, self.host_code, host_data)
        self.hal.derive_all_paged(c, SEG_PO2, SEG_ZK, code, data, image_buf(self.hal, self.host_image))
        self.hal.reduce_elem(code)
        self.hal.reduce_elem(data)
        return code, data

    def seal(self, data=None, proof=None, after=None, **kw):
        proof = self.proof if proof is None else proof
        return seal_tied(self.seg_prover, self.seg, self.code, self.data if data is None else data, np.zeros(4, dtype=np.uint32), self.page_prover,
                         self.page_segs, proof, proof.size, self.before, self.after if after is None else after, **kw)

    def verify(self, seg_receipt, parts, **kw):
        return verify_tied(seg_receipt, self.desc, seg_receipt.control_root, parts, parts[0].control_root, **kw)


@pytest.fixture(scope="module")
def group(hal):
    g = Group(hal)
    g.receipts = g.seal(check=True)
    return g


def test_a_tied_group_seals_and_verifies_from_root_to_root(hal, group):
    seg_receipt, parts = group.receipts
    assert len(parts) == 3 and len(group.table) == int(group.proof[2]) and any(i == o for _, i, o in group.table)
    root_before, root_after, hi = group.verify(seg_receipt, parts, root_before=group.root_before)
    assert np.array_equal(root_before, group.root_before) and np.array_equal(root_after, group.root_after) and hi == group.table[-1][0] + 1
    assert not np.array_equal(root_before, root_after)
    # every seal also verifies alone, and states one challenge: the one its data roots give
    seg_receipt.verify(group.desc, seg_receipt.control_root)
    page_hc = zhal.HostCircuit(T.p2_page_tied_circuit())
    for r in parts:
        r.verify(T.p2_page_tied_circuit(), r.control_root)
        assert np.array_equal(r.seal[T.OUT_ALPHA:T.OUT_TOTAL], seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL])
    roots = [zhal.HostCircuit(group.desc).seal_data_root(seg_receipt.seal)] + [page_hc.seal_data_root(r.seal) for r in parts]
    assert np.array_equal(zhal.tie_challenge(np.concatenate(roots)), seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL])
    # the last part has dead slots: its hi is the table's, and it adds only its live rows
    assert T.decode(parts[2].seal[17]) == hi and T.decode(parts[2].seal[16]) == group.table[43][0] + 1


def test_the_roots_of_the_traces_are_the_roots_the_seals_carry(hal, group):
    seg_receipt, _ = group.receipts
    hc = zhal.HostCircuit(group.desc)
    assert np.array_equal(group.seg_prover.data_root(group.data, SEG_PO2), hc.seal_data_root(seg_receipt.seal))
    assert np.array_equal(group.seg_prover.code_root(group.code, SEG_PO2), seg_receipt.control_root)
    hdr, _ = hc.receipt_decode(seg_receipt.to_words(group.desc, seg_receipt.control_root))
    assert np.array_equal(hdr["control_root"], group.seg_prover.code_root(group.code, SEG_PO2))
    with pytest.raises(HalError, match="^seal_data_root: "):
        hc.seal_data_root(seg_receipt.seal[:20])


def _forged_page_out(hal, group):
    """a consistent page-out of ANOTHER table: one `out` word of row 1 altered in the proof's table, and the tree after it committed over
    the image with that word"""
    proof = group.proof.copy()
    h = int(proof[4])
    at = 5 + h + 3 * 1 + 2
    proof[at] = (int(proof[at]) + ONE) % P
    image = group.image.to_vec()
    image[int(proof[5 + h + 3])] = proof[at]
    return proof, hal.image_commit(image_buf(hal, image))


def test_a_proof_of_another_table_is_refused_before_a_part_is_sealed_and_by_the_verifier_without_the_check(hal, group):
    proof, after = _forged_page_out(hal, group)
    with pytest.raises(HalError, match=r"^seal_tied: the proof's table is not the segment's page table: the segment's open total is [0-9a-f ]+, the fingerprint of "
                                       rf"the proof's {len(group.table)} rows is [0-9a-f ]+$"):
        group.seal(proof=proof, after=after)
    seg_receipt, parts = group.seal(proof=proof, after=after, check_table=False)       # all seals are made: the forged page-out is consistent
    with pytest.raises(HalError, match=r"^verify_tied: the totals do not cancel: the segment's F plus the parts' is [0-9a-f ]+, not zero"):
        group.verify(seg_receipt, parts)


def test_the_verifier_refuses_a_part_of_another_challenge_swapped_parts_and_another_segment(hal, group):
    seg_receipt, parts = group.receipts
    # the same group with one blinding word of the segment's data changed: another data root, so another challenge; the parts' traces,
    # and so their data roots, are the same
    other = group.host_data.copy().reshape(-1, 1 << SEG_PO2)
    other[0, -1] = (int(other[0, -1]) + 1) % P
    _, data2 = group.traces(other.reshape(-1))
    seg2, parts2 = group.seal(data=data2)
    assert not np.array_equal(seg2.seal[sl.OUT_ALPHA:sl.OUT_TOTAL], seg_receipt.seal[sl.OUT_ALPHA:sl.OUT_TOTAL])
    group.verify(seg2, parts2)
    with pytest.raises(HalError, match=r"^verify_tied: part 1: its challenge [0-9a-f ]+ is not the one the data roots give, [0-9a-f ]+$"):
        group.verify(seg_receipt, [parts[0], parts2[1], parts[2]])
    with pytest.raises(HalError, match=r"^verify_tied: part 1 opens root [0-9a-f ]+, but part 0 left root [0-9a-f ]+$"):
        group.verify(seg_receipt, [parts[0], parts[2], parts[1]])
    with pytest.raises(HalError, match=r"^verify_tied: part 0: its challenge [0-9a-f ]+ is not the one the data roots give, [0-9a-f ]+$"):
        group.verify(seg2, parts)                                                 # the receipt of another trace over the same image
    with pytest.raises(HalError, match=r"^verify_tied: part 0 opens root [0-9a-f ]+, not root_before [0-9a-f ]+$"):
        group.verify(seg_receipt, parts, root_before=group.root_after)
    with pytest.raises(HalError, match="^verify_segment: "):
        verify_tied(seg_receipt, group.desc, parts[0].control_root, parts, parts[0].control_root)
