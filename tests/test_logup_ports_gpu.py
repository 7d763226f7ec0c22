"""PORTS on the GPU (ZKA1 version 9; csrc/links.hip k_links<.., kPorts>, csrc/sort.hip's runs of several ports): the device against the numpy
twin cell for cell on small circuits whose ports have selectors (ports_cases.DIRECT: 2, 3 and 8 ports, an idle port, an idle head, one access,
equal addresses, ports with disjoint live key bits, raw words >= P, several memories after LIMBS records), the paged ported witness in
image and table mode with its page-out, the refusals with the twin's words and the data unchanged, SYN-LOOKUP-reads-ported sealed from
the library-derived witness byte for byte as from the host-made one, one 2-port tied run end to end, and two blobs WITHOUT ports, which
must launch what they launched before LINK records learnt to join.

Mutants these cases catch (never committed): masks per record instead of per memory fail `disjoint` (packed keys of the two ports are no
longer comparable: equal addresses stop linking); ranking the items by (port, row) instead of (row, port) fails every case with two
accesses to one address in a row (`equal`, `k2`); reading the previous access's cells through the lane's own record fails `k2` .. `mixed`."""
import re

import numpy as np
import pytest

import ports_cases as pc
import zko
from args_gpu import circuit as _circuit, image_buf, links_refused, profiled, seal_host as _seal_host, upload as _upload
from zeth_amd.circuits import logup, p2_tree_tied as TT, syn_lookup as sl
from zeth_amd.hal import HalError
from zeth_amd.prover import Segment, SegmentProver, preflight_paged_run, seal_paged_step, verify_paged_run

pytestmark = pytest.mark.gpu
P, ONE = pc.P, pc.ONE
NOISE = 0x9047


# ------------------------------------------------------------------------------------------------ device == twin
@pytest.mark.parametrize("kind", list(pc.DIRECT))
def test_the_device_is_the_twin_cell_for_cell(hal, kind):
    desc, blob, code, data, po2, zk = pc.direct(kind)
    n, A = 1 << po2, (1 << po2) - zk
    args = logup.Arguments.parse(blob)
    assert args.version == 9
    c = _circuit(hal, desc, blob)
    assert c.derives_links() and c.links_check_reads() == sum(pc.DIRECT[kind][2])
    assert c.derived_data_columns() == sorted(x for r in args.records for x in r.dsts)
    want = logup.reference_links(args, po2, zk, code, data)
    dcode, ddata = _upload(hal, code, data)
    prof = profiled(hal, lambda: hal.derive_links(c, po2, zk, dcode, ddata))
    assert {"sort_keys", "sort_pack", "links_check", "links_write"} <= set(prof), set(prof)
    assert ("sort_passes" in prof) == (kind not in ("equal", "one")), set(prof)     # no live key bit: zero radix passes
    got = ddata.to_vec()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{kind}: {bad.size} cells differ, the first in column {bad[0] // n} at row {bad[0] % n}: {got[bad[0]]} for {want[bad[0]]}"
    assert np.array_equal(got.reshape(-1, n)[:, A:], data.reshape(-1, n)[:, A:])                 # rows [A, n) bit for bit
    assert np.array_equal(dcode.to_vec(), code)
    hal.derive_links(c, po2, zk, dcode, ddata)                                # again, over its own output: the same
    assert np.array_equal(ddata.to_vec(), want)


def test_the_live_bits_are_the_memorys(hal):
    """`disjoint`: port 0's keys have live bits 0..3 only, port 1's among bits 0..3 and 4..6 and all of them bit 16: per record bit 16 is dead,
    per memory it tells the ports apart, and the rows where both ports touch one address link across them"""
    desc, blob, code, data, po2, zk = pc.direct("disjoint")
    n, A = 1 << po2, (1 << po2) - zk
    d = data.reshape(-1, n)
    k0, k1 = logup._dec(d[pc.KEY, :A]).astype(np.int64), logup._dec(d[pc.PER + pc.KEY, :A]).astype(np.int64)
    live = lambda k: int(np.bitwise_or.reduce(k) & ~np.bitwise_and.reduce(k))
    sel = lambda q: code.reshape(-1, n)[pc.WC0 + q, :A] == ONE
    assert live(k0[sel(0)]) < 16 and live(np.concatenate([k0[sel(0)], k1[sel(1)]])) >> 16 == 1


# ------------------------------------------------------------------------------------------------ paged
def test_the_paged_memory_in_image_and_table_mode_and_its_page_out(hal):
    s = pc.paged()
    po2, zk = 8, 40
    c = _circuit(hal, s["desc"], s["blob"])
    assert c.pages() and c.derives_links() and c.derives_columns() and c.derives_multiplicities()
    dcode, by_image = _upload(hal, s["code"], s["bare"])
    dimage = image_buf(hal, s["image"])
    hal.derive_all_paged(c, po2, zk, dcode, by_image, dimage)
    _, by_table = _upload(hal, s["code"], s["bare"])
    hal.derive_all_paged_table(c, po2, zk, dcode, by_table, s["table"], pc.W)
    assert np.array_equal(by_image.to_vec(), s["full"]) and np.array_equal(by_table.to_vec(), s["full"])
    assert np.array_equal(dimage.to_vec(), s["image"])
    hal.page_out(c, po2, zk, by_image, dimage)
    assert np.array_equal(dimage.to_vec(), s["after"]) and not np.array_equal(s["after"], s["image"])
    short = s["table"][:-1]                                                  # a table that lacks the trace's last page
    D = len(s["table"])
    _, ddata = _upload(hal, s["code"], s["bare"])
    with pytest.raises(HalError, match=r"but the page table has %d rows: the witness is refused" % (D - 1)):
        hal.derive_links_paged_table(c, po2, zk, dcode, ddata, short, pc.W)
    assert np.array_equal(ddata.to_vec(), s["bare"])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("what", ["clock", "load", "range"])
def test_a_refusal_across_ports_has_the_twins_words(hal, what):
    po2, zk = 8, 40
    s = pc.syn(po2, zk, 8)
    forged, want = pc.forge(what, s, po2, zk)
    links_refused(hal, s["desc"], s["blob"], po2, zk, s["code"], forged, want, seal=what == "load")


@pytest.mark.parametrize("what", ["clock0", "outside"])
def test_a_paged_refusal_on_a_joiner_has_the_twins_words(hal, what):
    po2, zk = 8, 40
    s = pc.paged()
    forged, want = pc.forge(what, s, po2, zk)
    links_refused(hal, s["desc"], s["blob"], po2, zk, s["code"], forged, want, image=s["image"])


def test_more_pages_than_the_table_has_rows_is_refused_before_anything_is_written(hal):
    """the one guard of the page table's rows: 2 ports over 6 active rows of an 8-row trace touch 12 addresses; the same trace with 6 is derived"""
    desc, blob, code, data, image, po2, zk = pc.overfull()
    links_refused(hal, desc, blob, po2, zk, code, data, pc.OVERFULL, image=image)
    _, _, code, data, image, _, _ = pc.overfull(spread=False)
    dcode, ddata = _upload(hal, code, data)
    hal.derive_links_paged(_circuit(hal, desc, blob), po2, zk, dcode, ddata, image_buf(hal, image))
    assert np.array_equal(ddata.to_vec(), logup.reference_links(logup.Arguments.parse(blob), po2, zk, code, data, image=image))


def test_selectors_are_refused_first_over_all_records_joiners_included(hal):
    desc, blob, code, data, po2, zk = pc.direct("k8")
    n = 1 << po2
    args = logup.Arguments.parse(blob)
    code, data = code.reshape(-1, n).copy(), data.reshape(-1, n).copy()
    code[pc.WC0 + 5, 7] = pc.enc(3)                                          # port 5 at row 7 ...
    code[pc.WC0 + 2, 9] = pc.enc(4)                                          # ... and port 2 at row 9: the lower record is named
    data[pc.WRITE, 1] = pc.enc(2)                                            # a write flag of the head at row 1 is not looked at before
    links_refused(hal, desc, blob, po2, zk, code, data, f"record {pc._record(args, 2)} at row 9: selector 4, not 0 or 1")
    code[pc.WC0 + 2, 9] = ONE
    links_refused(hal, desc, blob, po2, zk, code, data, f"record {pc._record(args, 5)} at row 7: selector 3, not 0 or 1")


def test_the_lowest_record_then_row_is_the_one_named(hal):
    po2, zk = 8, 40
    s = pc.syn(po2, zk, 8)
    n = 1 << po2
    _, wcols = pc.columns()
    d = np.array(s["full"], dtype=np.uint32).reshape(-1, n)
    d[wcols[2], 3], d[wcols[1], 100] = pc.enc(2), pc.enc(5)
    links_refused(hal, s["desc"], s["blob"], po2, zk, s["code"], d, f"record {pc._record(s['args'], 1)} at row 100: write flag 5, not 0 or 1")


# ------------------------------------------------------------------------------------------------ seals
@pytest.mark.parametrize("po2,zk", [(8, 40), (10, 200)])
def test_the_chain_equals_the_host_made_witness_and_seals_alike(hal, oracle, po2, zk):
    s = pc.syn(po2, zk, 8)
    assert logup.Arguments.parse(s["plain"]).version == 1 and s["args"].version == 9 and not np.array_equal(s["bare"], s["full"])
    c = _circuit(hal, s["desc"], s["blob"])
    assert c.derives_links() and c.links_check_reads() == 3 and c.derives_columns() and c.derives_multiplicities() and not c.derives_sorted()
    dcode, ddata = _upload(hal, s["code"], s["bare"])
    hal.derive_all(c, po2, zk, dcode, ddata)
    assert np.array_equal(ddata.to_vec(), s["full"])
    bus = hal.check_bus(c, po2, zk, dcode, ddata)                            # the bus of a ported circuit, checked by the code that knows no ports
    assert bus["unbalanced_keys"] == 0 and (bus["term"], bus["row"]) == (-1, -1)
    seg = Segment(index=0, po2=po2, zk_cycles=zk, noise_seed=NOISE)
    receipt = _seal_host(hal, SegmentProver(hal, s["desc"], arguments=s["blob"]), seg, s["code"], s["bare"], s["out"], check=True)
    host = _seal_host(hal, SegmentProver(hal, s["desc"], arguments=s["plain"]), seg, s["code"], s["full"], s["out"])
    assert np.array_equal(receipt.seal, host.seal)
    oc = zko.OracleCircuit(oracle, s["desc"])
    root = oc.root_of_code(po2, s["code"])
    receipt.verify(s["desc"], root)
    assert oc.verify(receipt.seal, root) is None
    # under the blob of three separate memories the same traces are no witness: a load reads what another port stored
    with pytest.raises(HalError, match=r"derive_links: record \d at row \d+: a load of carried column 1 returns \d+, but "):
        hal.derive_links(_circuit(hal, s["desc"], s["apart"]), po2, zk, *_upload(hal, s["code"], s["bare"]))


# ------------------------------------------------------------------------------------------------ one run end to end
def test_a_two_port_tied_run_of_two_segments(hal):
    po2, zk, h = 8, 40, 3
    shape = sl.Shape(2, 4, 4, 2)
    first = pc.paged(po2, zk, seed=3, tied=True, shape=shape)
    desc, blob, args = first["desc"], first["blob"], first["args"]
    assert args.version == 9 and args.open is not None and args.pages is not None
    images, witnesses = [first["image"]], []
    for seed in (3, 4):
        code, bare, _ = sl.witness(shape, po2, zk, seed=seed, link=False, reads=True, ports=True, pages=False, image=images[-1])
        _, full, _ = sl.witness(shape, po2, zk, seed=seed, link=True, reads=True, ports=True, pages=True, image=images[-1])
        witnesses.append((code, bare))
        images.append(logup.reference_page_out(args, po2, zk, full, images[-1]))
    roots = [logup.reference_image_root(i) for i in images]
    assert not np.array_equal(roots[0], roots[1]) and not np.array_equal(roots[1], roots[2])
    segs = [Segment(index=10 * k, po2=po2, zk_cycles=zk, noise_seed=NOISE + 100 * k) for k in range(2)]
    seg_prover = SegmentProver(hal, desc, arguments=blob)
    page_prover = SegmentProver(hal, TT.p2_tree_tied_circuit(), arguments=TT.arguments())
    image = image_buf(hal, images[0])
    tree = hal.image_commit(image)
    steps = preflight_paged_run(seg_prover, segs, witnesses, image, tree)
    assert np.array_equal(image.to_vec() % P, images[2] % P)
    for k, s in enumerate(steps):
        assert np.array_equal(s.root_before, roots[k]) and np.array_equal(s.root_after, roots[k + 1])
    del image, tree
    prefix = np.zeros(4, dtype=np.uint32)
    groups = [seal_paged_step(steps[k], seg_prover, prefix, page_prover, lambda p, k=k: Segment(index=10 * k + 1 + p, po2=8, zk_cycles=40, noise_seed=NOISE + 100 * k + 1 + p))
              for k in range(2)]
    got = verify_paged_run(groups, desc, groups[0][0].control_root, groups[0][1][0].control_root, h, root_before=roots[0])
    assert np.array_equal(got[0], roots[0]) and np.array_equal(got[1], roots[2])
    with pytest.raises(HalError, match=r"^verify_paged_run: group 1 opens root [0-9a-f ]+, but group 0 left root [0-9a-f ]+$"):
        verify_paged_run(groups[::-1], desc, groups[0][0].control_root, groups[0][1][0].control_root, h)


# ------------------------------------------------------------------------------------------------ blobs without ports
# {scope: (calls, algorithmic bytes)} of one derive, read off the commit before this one with the two calls below (its
# tests/test_logup_links_gpu.py::_case("two", 1208, 12, 1994) and tests/pages_cases.py case("two", 7, 10, 200)); a blob without a joiner
# must go through the launches it went through then
LINKED_BEFORE = {'links_check': (1, 84080.0), 'links_write': (1, 260648.0), 'sort_keys': (1, 33632.0), 'sort_pack': (1, 84080.0), 'sort_passes': (1, 159536.0)}
PAGED_BEFORE = {'links_check': (1, 49440.0), 'links_write': (1, 138432.0), 'pages_scan': (1, 9920.0), 'sort_keys': (1, 6592.0), 'sort_pack': (1, 26368.0),
                'sort_passes': (1, 67520.0)}


def _scopes(prof):
    return {name: (r["calls"], r["alg_bytes"]) for name, r in sorted(prof.items())}


def test_blobs_without_ports_launch_what_they_launched(hal):
    import pages_cases
    from test_logup_links_gpu import _case
    desc, blob, code, data = _case("two", 1208, 12, 1994)
    assert logup.Arguments.parse(blob).version == 5
    c = _circuit(hal, desc, blob)
    dcode, ddata = _upload(hal, code, data)
    linked = _scopes(profiled(hal, lambda: hal.derive_links(c, 12, 1994, dcode, ddata)))
    desc, blob, code, data, image = pages_cases.case("two", 7, 10, 200)
    assert logup.Arguments.parse(blob).version == 7
    c = _circuit(hal, desc, blob)
    dcode, ddata = _upload(hal, code.reshape(-1), data.reshape(-1))
    dimage = image_buf(hal, image)
    paged = _scopes(profiled(hal, lambda: hal.derive_links_paged(c, 10, 200, dcode, ddata, dimage)))
    assert linked == LINKED_BEFORE and paged == PAGED_BEFORE
