"""What the tests of THE TIE share (tests/test_tied.py, tests/test_tied_gpu.py; imported the way page_ordered_cases is): the tiny tied
segment's host-made witness over an image of 64 words, its page table, its open total under one fixed challenge, and the reference's
P2-PAGE-tied parts of that table.  Everything is built once per process."""
import functools

import numpy as np

import page_ordered_cases as oc
from zeth_amd.circuits import logup, p2_page, p2_page_tied as T, syn_lookup as sl

P = logup.P
ONE = (1 << 32) % P
SEG_PO2, SEG_ZK, W = 8, 40, 64
PAGE_PO2, PAGE_ZK, _W = oc.SHAPES[2]
assert _W == W
# the challenge of the totals tests, fixed: alpha ‖ beta as Montgomery words (test_the_fixed_challenge_separates_the_altered_table
# shows on the CPU that it tells the altered table from the honest one)
CHALLENGE = np.array([0x1234567, 0x89abcd, 0x2468ace, 0x13579bd, 0x0fedcba, 0x7654321, 0x3c3c3c3, 0x5a5a5a5], dtype=np.uint32)


def enc(x):
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P) * np.uint64(ONE) % np.uint64(P)).astype(np.uint32)


def f4_add(*xs):
    """the sum of Fp4 values given as 4 Montgomery words each"""
    return (np.sum([np.asarray(x, dtype=np.uint64) for x in xs], axis=0) % np.uint64(P)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def segment(seed=3):
    """the tiny tied segment's host-made witness over a random image of W words -> a dict: desc, blob, args, code, data, image, and its
    page table as ZKU1 rows (address, in, out)"""
    desc, blob = sl.syn_lookup_tiny_tied()
    args = logup.Arguments.parse(blob)
    image = np.random.default_rng(seed).integers(1, P, W, dtype=np.uint64).astype(np.uint32)
    code, data, _ = sl.witness(sl.TINY, SEG_PO2, SEG_ZK, seed=seed, link=True, reads=True, pages=True, image=image)
    n, A = 1 << SEG_PO2, (1 << SEG_PO2) - SEG_ZK
    d, pg = data.reshape(-1, n), args.pages
    on = d[pg.p_on, :A] == ONE
    table = [(int(a), int(i), int(o)) for a, i, o in zip(logup._dec(d[pg.p_addr, :A][on]), d[pg.p_in, :A][on], d[pg.p_out, :A][on])]
    return {"desc": desc, "blob": blob, "args": args, "code": code, "data": data, "image": image, "table": table}


@functools.lru_cache(maxsize=None)
def segment_total(seed=3):
    """(accum, the open total as 4 Montgomery words) of the segment under CHALLENGE, by the reference accumulate"""
    s = segment(seed)
    accum, total = logup.reference_accumulate(s["args"], SEG_PO2, SEG_ZK, s["code"], s["data"], CHALLENGE)
    return accum, enc(total)


@functools.lru_cache(maxsize=None)
def parts(altered=False):
    """the reference's P2-PAGE-tied parts of the segment's page table under CHALLENGE: [(data, accum, out)].  altered: one `out` word of
    row 1 of the table is another residue, on the page-out side only (the image the parts open is the segment's)"""
    s = segment()
    table = list(s["table"])
    if altered:
        a, w_in, w_out = table[1]
        table[1] = (a, w_in, (w_out + ONE) % P)
    plan = p2_page.parts(PAGE_PO2, PAGE_ZK, W, len(table))
    return [T.reference_tied_part(PAGE_PO2, PAGE_ZK, W, table, s["image"], first, CHALLENGE) for first, _ in plan]
