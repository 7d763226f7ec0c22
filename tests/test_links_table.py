"""Paging in from a page table, without a device: the numpy twin `logup.reference_links(..., table=, image_words=)` against the image
variant on every kind of pages_cases at (8, 40), the three refusals that are the table's own, the image variant's read-rule text for a first
load the table contradicts, and the links of a paged run (`link_paged_run`) over made-up roots."""
import re

import numpy as np
import pytest

import links_table_cases as lt
import pages_cases as pc
from zeth_amd.circuits import logup
from zeth_amd.hal import HalError
from zeth_amd.prover import link_paged_run

P = pc.P
PO2, ZK = 8, 40
N, A = 1 << PO2, (1 << PO2) - ZK


def _case(kind, seed=7):
    desc, blob, code, data, image = pc.case(kind, seed, PO2, ZK)
    return logup.Arguments.parse(blob), code, data, image


@pytest.mark.parametrize("kind", pc.KINDS)
def test_the_table_stands_for_the_image(kind):
    args, code, data, image = _case(kind)
    want = logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), image=image)
    table = lt.table_of(want, PO2, ZK)
    assert np.array_equal(table[:, :2], lt.table_for(code, data, image, A, kind)[:, :2]), "the two ways to make the table differ"
    got = logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), table=table, image_words=len(image))
    assert np.array_equal(got % P, want % P)
    if kind == "big":                                                        # the image's raw words >= P reach the table as residues: the case exercises the path
        assert (got != want).any() and (image[table[:, 0]] >= P).any()
    else:
        assert np.array_equal(got, want)
    with pytest.raises(ValueError, match="exactly one of image / table"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), image=image, table=table, image_words=len(image))


@pytest.mark.parametrize("what", ["changed", "cut", "added"])
def test_a_table_of_other_pages_is_refused(what):
    args, code, data, image = _case("two")
    table = lt.table_for(code, data, image, A, "two")
    bad, msg = lt.own_refusals(table, data, A, 2, 17)[what]
    assert len(table) > 18 and args.records.index(args.pages) == 2
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), table=bad, image_words=len(image))


def test_on_one_row_the_address_goes_first_and_the_clock_after():
    """the first access of the highest address, with clock 0 and another address in its row of the table: the table's refusal is named; in
    an image that ends at that address, the address's"""
    args, code, data, image = _case("two")
    table = lt.table_for(code, data, image, A, "two")
    bad, msg = lt.own_refusals(table, data, A, 2, len(table) - 1)["changed"]
    a = int(table[-1, 0])
    r = lt.first_access(data, A, a)
    d = data.copy()
    d[pc.CLOCK, r] = np.uint32(P)
    with pytest.raises(logup.ReferenceError, match=f"^record 0 at row {r}: clock 0 is the image's$"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), d.reshape(-1), table=table, image_words=len(image))
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), d.reshape(-1), table=bad, image_words=len(image))
    with pytest.raises(logup.ReferenceError, match=f"^record 0 at row {r}: address {a} outside the image of {a} words$"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), d.reshape(-1), table=bad, image_words=a)


def test_a_first_load_that_the_table_contradicts_gets_the_read_rule_text():
    args, code, data, image = _case("two")
    table = lt.table_for(code, data, image, A, "two")
    x = lambda v: int(pc.dec(v))
    page = next(i for i in range(len(table)) if data[pc.WRITE, lt.first_access(data, A, int(table[i, 0]))] % P == 0)
    a = int(table[page, 0])
    r = lt.first_access(data, A, a)
    table[page, 1] = pc.enc(x(image[a]) + 1)
    msg = f"record 0 at row {r}: a load of carried column 1 returns {x(image[a])}, but the image holds {(x(image[a]) + 1) % P} at its address {a}"
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), table=table, image_words=len(image))
    # and it is the image variant's text: an image with that word says the same
    other = image.copy()
    other[a] = table[page, 1]
    with pytest.raises(logup.ReferenceError, match="^" + re.escape(msg) + "$"):
        logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), image=other)


def test_the_image_words_are_bounded():
    args, code, data, image = _case("range5")
    table = lt.table_for(code, data, image, A, "range5")
    for W in (0, 1 << 32, None):
        with pytest.raises(logup.ReferenceError, match=re.escape(f"an image of {W} words (1 .. 2^32 - 1)")):
            logup.reference_links(args, PO2, ZK, code.reshape(-1), data.reshape(-1), table=table, image_words=W)


def test_the_groups_of_a_run_must_link():
    r = [np.random.default_rng(k).integers(0, P, 8, dtype=np.uint64).astype(np.uint32) for k in range(5)]
    fmt = lambda w: " ".join(f"{int(x):08x}" for x in w)
    run = [(r[0], r[1]), (r[1], r[2]), (r[2], r[3])]
    for given in (None, r[0]):
        first, last = link_paged_run(run, given)
        assert np.array_equal(first, r[0]) and np.array_equal(last, r[3])
    assert np.array_equal(link_paged_run(iter(run[:1]))[1], r[1])
    with pytest.raises(HalError, match=f"^verify_paged_run: group 1 opens root {fmt(r[0])}, but group 0 left root {fmt(r[2])}$"):
        link_paged_run([run[1], run[0], run[2]])                              # a swapped pair
    with pytest.raises(HalError, match=f"^verify_paged_run: group 1 opens root {fmt(r[2])}, but group 0 left root {fmt(r[1])}$"):
        link_paged_run([run[0], run[2]])                                      # the middle group dropped
    with pytest.raises(HalError, match=f"^verify_paged_run: group 0 opens root {fmt(r[0])}, not root_before {fmt(r[4])}$"):
        link_paged_run(run, r[4])
    with pytest.raises(HalError, match="^verify_paged_run: no group$"):
        link_paged_run([])
