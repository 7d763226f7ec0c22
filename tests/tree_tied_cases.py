"""What the tests of P2-TREE-tied share (tests/test_tree_tied.py, tests/test_tree_tied_gpu.py; imported the way page_tree_cases is): the
reference's tied parts (p2_tree_tied.reference_tree_tied_part) of page_tree_cases' tables under tied_cases' fixed challenge, and the
two-block case of the split closure.  Every part is built once per process and handed out read-only."""
import functools

import numpy as np

import page_tree_cases as tc
import tied_cases
from zeth_amd.circuits import logup, p2_tree, p2_tree_tied as TT

P = tc.P
ONE = tc.ONE
CHALLENGE = tied_cases.CHALLENGE
H3, H5, H6, H8 = tc.H3, tc.H5, tc.H6, tc.H8
# (shape, address set): what the CPU tests check the constraints and the totals on; the GPU parity test adds H8 x random
TABLES = [(H3, 0), (H3, "one_pair"), (H3, "adjacent"), (H3, "all"), (H5, "first_last"), (H6, "all")]


def grid(tables=TABLES):
    """(shape, what, p) over `tables` and every part of each plan"""
    return [(s, what, p) for s, what in tables for p in range(len(tc.table(*s, what)["plan"]))]


grid_id = tc.grid_id


def altered_table(table):
    """the table with one `out` word of one row (the second, or the only one) another residue"""
    table = list(table)
    i = min(1, len(table) - 1)
    a, w_in, w_out = table[i]
    table[i] = (a, w_in, (w_out + ONE) % P)
    return table


@functools.lru_cache(maxsize=None)
def part(po2, zk, W, what, p=0, altered=False):
    """-> (data, accum, out, code) of part p of page_tree_cases.table(...)'s plan under CHALLENGE: the reference's data group as (138, n)
    with the blinding rows zero, its accum group (48, n), its 31 `out` words and the code group (41, n).  altered: `altered_table`, on the
    page-out side only (the image the parts open is the table's)"""
    t = tc.table(po2, zk, W, what)
    first, count = t["plan"][p]
    active, accum, out = TT.reference_tree_tied_part(po2, zk, W, altered_table(t["table"]) if altered else t["table"], t["image"], first, count, CHALLENGE)
    n = 1 << po2
    data = np.zeros((TT.WD, n), dtype=np.uint32)
    data[:, :n - zk] = active
    for a in (data, accum, out):
        a.setflags(write=False)
    return data, accum, out, tc.code_of(po2, zk)


def reaccumulate(po2, zk, data, out, args=None):
    """(accum, out) of a tampered data group: the reference accumulate again under CHALLENGE, and the sum of ALL columns in out's F"""
    args = logup.Arguments.parse(TT.arguments()) if args is None else args
    accum, total = logup.reference_accumulate(args, po2, zk, tc.code_of(po2, zk), data, CHALLENGE)
    out = np.array(out, dtype=np.uint32)
    out[TT.OUT_TOTAL:] = tied_cases.enc(total)
    return accum.reshape(TT.WA, 1 << po2), out


# the two-block case of the split closure: an image of 32 words is a tree of height 2, a root block over one pair block; the one row of
# the table has in = out, so the pair block is touched and produces its digests, but old = new everywhere
TWO_BLOCKS = (7, 40, 32)


# ... and the same image with a dead slot between the pair block and the root slot: room for a block that is cut off from the tree
THREE_BLOCKS = (7, 30, 32)


@functools.lru_cache(maxsize=None)
def two_blocks(shape=TWO_BLOCKS, changed=False):
    """-> (data, accum, out, code) of the one part of `shape` (TWO_BLOCKS or THREE_BLOCKS); changed: the row's out is another word than
    its in, so the two roots differ"""
    po2, zk, W = shape
    image = np.random.default_rng(32).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    table = [(5, int(image[5]), (int(image[5]) + ONE * changed) % P)]
    assert p2_tree.block_slots(po2, zk) == (2 if shape == TWO_BLOCKS else 3) and p2_tree.parts(po2, zk, W, [5]) == [(0, 1)]
    active, accum, out = TT.reference_tree_tied_part(po2, zk, W, table, image, 0, 1, CHALLENGE)
    n = 1 << po2
    data = np.zeros((TT.WD, n), dtype=np.uint32)
    data[:, :n - zk] = active
    return data, accum, out, tc.code_of(po2, zk)
