"""What the tests of the FLAT-ADDRESS columns share (tests/test_logup_flat.py, tests/test_logup_flat_gpu.py, tests/test_tied_wide.py,
tests/test_tied_wide_gpu.py; imported the way wide_cases is): wide_cases' hand-built traces with two more data columns, p_flat_0 and
p_flat_1, the flats of the PAGES record (ZKA1 version 11), poisoned like every destination; the independent answer, which is the address
column of the FLAT table that wide_cases.walk returns; and the tiny tied-wide segment over a flat image of 64 words with its flat table,
its open total under tied_cases' challenge and the reference's page-out parts of that table.  Everything heavy is built once per process."""
import functools

import numpy as np

import page_ordered_cases as oc
import tied_cases
import wide_cases as wc
from conftest import rand_fp
from zeth_amd.circuits import logup, p2_page, p2_page_tied, p2_tree, p2_tree_tied, syn_lookup as sl
from zeth_amd.circuits.desc import GROUP_CODE

P, ONE = wc.P, wc.ONE
KINDS = ["equal", "distinct", "edges", "sparse", "big"]       # D = 1; D = A, no row below the table; flat 0, 1, 2 W - 2, 2 W - 1; a selector; raw words >= P
PORTED_KINDS = ["equal", "edges", "sparse", "big"]           # k = 3: k A distinct addresses do not fit the table
SIZES = wc.SIZES
CHALLENGE = tied_cases.CHALLENGE


def flat_columns(data_columns):
    """(p_flat_0, p_flat_1) of a case whose data group has `data_columns` columns: the last two"""
    return data_columns - 2, data_columns - 1


@functools.lru_cache(maxsize=None)
def case(kind, seed, po2, zk, k=1):
    """wide_cases.case with the two flat columns -> (desc, blob, blob10, code, data, image).  blob is the version-11 blob whose PAGES
    record has the flats (the last two data columns, poisoned), blob10 the version-10 blob of the SAME circuit and columns without them;
    code, data, image as wide_cases' (read-only here: the cases are shared)"""
    _, old, code, data, image = wc.case(kind, seed, po2, zk, k=k)
    wd = data.shape[0] + 2
    data = np.vstack([data, rand_fp(np.random.default_rng(seed + 1000), 2, 1 << po2)])
    a = logup.Arguments.parse(old)
    out = []
    for flats in (flat_columns(wd), None):
        b = logup.LogupBuilder((4, wc.WC, wd), (4, 8))
        for t in a.terms:
            b.term(t.col, list(t.tuple_cols), tag=t.tag)
        built = []
        for r in a.records:                                                  # the blob's order: the LINK records, then the PAGES record
            if isinstance(r, logup.Link):
                built.append(b.derive_links(r.sel, r.key, r.carried, r.dsts, r.limb_bits, write=r.write, joins=None if r.joins is None else built[r.joins]))
            else:
                b.derive_pages(built[r.link], r.dsts, r.limb_bits, flats=flats)
        out.append(b.finish_all(b.arguments(b.true(), b.get(GROUP_CODE, 0), b.get(GROUP_CODE, 1), b.get(GROUP_CODE, 2))))
    (desc, blob), (desc10, blob10) = out
    assert np.array_equal(desc, desc10) and np.array_equal(logup.Arguments.parse(blob10).blob()[8:-32], old[8:-32])
    for x in (code, data, image):
        x.setflags(write=False)
    return desc, blob, blob10, code, data, image


def want(code, data, image, A, kind, k=1, flats=True):
    """-> (the data group the links stage must leave, D, the flat table): wide_cases.walk's columns over `data`, and the two flat columns
    from the walk's FLAT TABLE, whose address column 2 a + j is the independent answer: encoded on the table's rows, 0 below them"""
    out, mem, flat = wc.walk(code, data, image, A, kind, k=k)
    full = np.array(data, dtype=np.uint32)
    for c, v in out.items():
        full[c, :A] = v
    D = len(mem)
    assert flat.shape == (2 * D, 3)
    if flats:
        for j, c in enumerate(flat_columns(data.shape[0])):
            full[c, :A] = 0
            full[c, :D] = wc.enc(flat[j::2, 0])
    return full, D, flat


# ------------------------------------------------------------------------------------------------ the tiny tied-wide segment
SEG_PO2, SEG_ZK, WORDS = tied_cases.SEG_PO2, tied_cases.SEG_ZK, 64       # the flat image: 64 words, 32 addresses, a tree of height 3
H = 3
PAGE_PO2, PAGE_ZK = tied_cases.PAGE_PO2, tied_cases.PAGE_ZK              # P2-PAGE-tied's page shape: (12, 1994)
TWO_PARTS, ONE_PART = (8, 40), (10, 500)                                  # P2-TREE-tied's page shapes


def flat_image(seed=3):
    return np.random.default_rng(seed).integers(1, P, WORDS, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def segment(seed=3, ports=False):
    """the tiny tied-wide segment's host-made witness over the flat image -> a dict: desc, blob, args, shape, code, data, image and its FLAT
    page table as ZKU1 rows (2 a + j, in_j, out_j), read off the page table's own columns (p_addr, p_in_j, p_out_j), not off p_flat_j"""
    shape = sl.MULTI if ports else sl.TINY
    desc, blob = sl.build_syn_lookup(shape, link=True, reads=True, pages=True, tied=True, wide=True, flat=True, ports=ports)
    args = logup.Arguments.parse(blob)
    image = flat_image(seed)
    code, data, _ = sl.witness(shape, SEG_PO2, SEG_ZK, seed=seed, link=True, reads=True, pages=True, image=image, wide=True, flat=True, ports=ports)
    n, A = 1 << SEG_PO2, (1 << SEG_PO2) - SEG_ZK
    d, pg = data.reshape(-1, n), args.pages
    on = d[pg.p_on, :A] == ONE
    table = []
    for i in np.nonzero(on)[0]:
        a = int(logup._dec(d[pg.p_addr, i]))
        table += [(2 * a + j, int(d[pg.p_ins[j], i]), int(d[pg.p_outs[j], i])) for j in range(2)]
    return {"desc": desc, "blob": blob, "args": args, "shape": shape, "code": code, "data": data, "image": image, "table": table}


@functools.lru_cache(maxsize=None)
def segment_total(seed=3, ports=False):
    """(accum, the open total as 4 Montgomery words) of the segment under CHALLENGE, by the reference accumulate"""
    s = segment(seed, ports)
    accum, total = logup.reference_accumulate(s["args"], SEG_PO2, SEG_ZK, s["code"], s["data"], CHALLENGE)
    return accum, tied_cases.enc(total)


def altered(table):
    """the flat table with one `out` word of one flat row (row 1: the second word of the first page) another residue"""
    table = list(table)
    a, w_in, w_out = table[1]
    table[1] = (a, w_in, (w_out + ONE) % P)
    return table


@functools.lru_cache(maxsize=None)
def tree_parts(alter=False):
    """the reference's P2-TREE-tied parts of the segment's FLAT table at (8, 40) under CHALLENGE: [(active data, accum, out)]; the
    page-out side knows nothing of V.  alter: `altered`, on the page-out side only"""
    s = segment()
    table = altered(s["table"]) if alter else s["table"]
    plan = p2_tree.parts(*TWO_PARTS, WORDS, [a for a, _, _ in s["table"]])
    return [p2_tree_tied.reference_tree_tied_part(*TWO_PARTS, WORDS, table, s["image"], first, count, CHALLENGE) for first, count in plan]


@functools.lru_cache(maxsize=None)
def page_parts(alter=False):
    """... and its P2-PAGE-tied parts at tied_cases' page shape: [(data, accum, out)]"""
    s = segment()
    table = altered(s["table"]) if alter else s["table"]
    plan = p2_page.parts(PAGE_PO2, PAGE_ZK, WORDS, len(table))
    return [p2_page_tied.reference_tied_part(PAGE_PO2, PAGE_ZK, WORDS, table, s["image"], first, CHALLENGE) for first, _ in plan]


assert oc.SHAPES[2][2] == WORDS
