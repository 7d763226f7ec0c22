"""What the tests of paging in from a page table share (tests/test_links_table.py, tests/test_links_table_gpu.py; imported the way
pages_cases is): the ZKU1 rows (address, in, out) that stand for an image, read off a derived trace or made from the trace's own
addresses, and the tables of the three refusals that are the table's own."""
import numpy as np

import pages_cases as pc

P, ONE = pc.P, pc.ONE
SIZES = [(8, 40), (12, 1994), (13, 1994)]


def table_of(full, po2, zk):
    """the page table a derived data trace holds, as the proof of its page-out ships it: (a_i, p_in % P, p_out % P) of the rows with p_on = 1"""
    n, A = 1 << po2, (1 << po2) - zk
    d = np.asarray(full, dtype=np.uint32).reshape(-1, n)
    on = d[pc.P_ON, :A] == ONE
    return np.stack([pc.dec(d[pc.P_ADDR, :A][on]).astype(np.uint32), d[pc.P_IN, :A][on] % P, d[pc.P_OUT, :A][on] % P], axis=1).astype(np.uint32)


def table_for(code, data, image, A, kind):
    """the table of the trace's own pages without deriving anything: the distinct addresses of the paged record's accesses in order, in =
    image[a] % P (0 for an address outside the image), out = 0 (the derive never reads it)"""
    a = np.unique(pc.dec(data[pc.KEY, pc.accesses(code, data, A, kind)])).astype(np.int64)
    word = np.where(a < len(image), np.asarray(image, dtype=np.uint32)[np.minimum(a, len(image) - 1)] % P, 0)
    return np.stack([a, word, np.zeros_like(a)], axis=1).astype(np.uint32)


def first_access(data, A, address):
    """the row of the first access to `address` in a case without a selector"""
    return int(np.nonzero(pc.dec(data[pc.KEY, :A]) == address)[0][0])


def own_refusals(table, data, A, R, page):
    """-> {name: (table, message)} of the three refusals that are the table's own, for a trace whose pages are `table`'s rows (no selector):
    row `page` with another address, the last row cut, a row added.  R: the PAGES record's index"""
    D = len(table)
    changed = table.copy()
    a = int(table[page, 0])
    changed[page, 0] = b = a + 1 if page + 1 == D or int(table[page + 1, 0]) != a + 1 else a - 1
    top = int(table[D - 1, 0])
    added = np.concatenate([table, [[top + 1, 5, 6]]]).astype(np.uint32)
    return {"changed": (changed, f"record {R} at row {first_access(data, A, a)}: address {a} is page {page} of the trace, but row {page} of the page table holds address {b}"),
            "cut": (table[:-1].copy(), f"record {R} at row {first_access(data, A, top)}: address {top} is page {D - 1} of the trace, but the page table has {D - 1} rows"),
            "added": (added, f"record {R}: the trace pages {D} addresses, but the page table has {D + 1} rows")}
