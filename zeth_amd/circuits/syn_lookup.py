"""SYN-LOOKUP: the declared-synthetic circuit whose accum group is a SOUND argument — range lookups and a multiset equality as
log-derivative sums (logup.py), sealed through the library's built-in accumulate (zkh_accumulate).

The shape of what a real zkVM circuit keeps in its accum group: byte / range tables and the memory argument (DESIGN.md §2
ARGUMENTS).  Columns (n rows, A = n - zk_cycles active rows, L = limb_bits):
  code : c0 active, c1 first, c2 body (active & !first), c3 row index, c4 last (row A-1), c5 table selector (rows < 2^L),
         c6 table value (= row on table rows, else 0)
  data : words w_k (n_words), then limbs b_{k,j} (n_words x n_limbs), the table multiplicity m, then n_mem (addr, val, time)
         tuples and their permuted copies
  accum: the argument's running sums, three terms per Fp4 column
Constraints: w_k = sum_j b_{k,j} 2^{j L} on active rows; the argument (logup.py); SYN-AIR's selector sanity.
Argument terms (one bus):
  tag 0 — every limb +1 (tuple (b)); the table -m on table rows (tuple (c6), selector c5)
  tag 1 — every memory tuple +1 (addr, val, time), its permuted copy -1
Globals: out = 4 zero words; mix = alpha (words 0..3), beta (4..7).
The witness comes from the host (`witness`, numpy): the upstream flow of a CPU preflight + witgen uploaded as caller traces.
SYN-LOOKUP-derived (`syn_lookup_derived`, `build_syn_lookup(shape, derive=True)`): the same description word for word (the same
control root), the table term marked derived in a ZKA1 version-2 blob, so the library counts m (zkh_derive_multiplicities) and
the witness may leave it zero (`witness(count=False)`).
SYN-LOOKUP-sorted (`syn_lookup_sorted`, `build_syn_lookup(shape, sort=True)`): again the same description; every permuted copy is
marked as the sorted copy of its memory tuple by (addr, time) in a ZKA1 version-3 blob, so the library sorts (zkh_derive_sorted) and
the witness may leave the permuted columns zero (`witness(sort=False)`).  `derive` and `sort` combine.
`build_syn_lookup(shape, limbs=True)`: the same description once more; every word's decomposition is a LIMBS record of a ZKA1
version-4 blob, so the library splits the words (zkh_derive_columns) and the witness may leave the limbs zero (`witness(limbs=False)`).
SYN-LOOKUP-ordered (`build_syn_lookup(shape, order=True)`): ANOTHER description, the one a memory argument needs.  The multiset
equality alone lets any permutation pass for the sorted copy; here every memory pair gets, after the columns above, a flag column
e = "same address as the previous row" and `order_limbs` limb columns of the ordered difference of the copy's (addr, time), the
constraints that tie them to consecutive rows (logup.order_constraints) on the body rows, and the limbs as further lookups of tag 0.
They are an ORDER record, so the library fills them (`witness(order=False)` leaves them zero).  Addresses and times stay below
2^(order_limbs L).
SYN-LOOKUP-linked (`syn_lookup_linked`, `build_syn_lookup(shape, link=True)`): ANOTHER description again, the memory argument without
a sorted copy.  Every active row is an access; per memory pair the data columns are addr, val, time, linked, last, pval, ptime and
`order_limbs` limb columns.  On the bus (tag 1) every access adds (addr, val, time), removes -linked (addr, pval, ptime) — the
previous access to its address — and -last (addr, val, time) pages the final access of an address out; an unlinked access is the
page-in.  The limbs of time - ptime - 1 are lookups of tag 0 and logup.link_constraints ties them to the row, so a link cannot point
forward in time.  linked, last, pval, ptime and the limbs are a LINK record (ZKA1 version 5): the library fills them
(zkh_derive_links; `witness(link=False)` leaves them zero).  Times are the row numbers, so differences stay below 2^(order_limbs L).
What it leaves out: the read rule (a load returns pval), and an initial-memory table behind linked = 0.
SYN-LOOKUP-reads (`syn_lookup_reads`, `build_syn_lookup(shape, link=True, reads=True)`): SYN-LOOKUP-linked with the read rule.  Per
memory pair one more data column, the write flag w (after every pair's link columns: `reads_layout`), the host's; the LINK record has
READS (ZKA1 version 6), so zkh_derive_links refuses a load (w = 0) that does not return pval, or 0 where it is not linked, and
logup.link_constraints adds w (1 - w) = 0 and (1 - w) (val - linked pval) = 0.  `witness(link=..., reads=True)` is a real load / store
trace; `misread_row` forges one load so that the bus still balances.
SYN-LOOKUP-paged (`syn_lookup_paged`, `build_syn_lookup(shape, link=True, reads=True, pages=True)`; one memory pair): SYN-LOOKUP-reads
whose memory is paged in from an image and out again.  After the write flag come the page table's columns (`pages_layout`): p_on, p_addr,
p_in, p_out, p_time and `order_limbs` limbs each of the page address and of the gap to the page before.  On the bus (tag 1): every access
adds (addr, val, time) and removes (addr, pval, ptime), UNGATED: the first access to an address removes (addr, image word, 0), which the
page table put there with +p_on (p_addr, p_in) — a width-2 tuple, the key (addr, val, 0) — and -p_on (p_addr, p_out, p_time) pages the
final tuple of every address out.  Nothing uses linked or last as a multiplicity.  The link limbs, the address limbs and the gap limbs are
lookups of tag 0; logup.link_constraints (paged) and logup.page_constraints tie them to the rows, so the page addresses strictly increase
and no address is paged in twice.  The link columns are the LINK record's, the table a PAGES record's (ZKA1 version 7): the library fills
both from the image (zkh_derive_links_paged; `witness(link=False, pages=False)` leaves them zero).  Times are row + 1 (clock 0 is the
image's), so the limbs must cover A: 2^(order_limbs L) > A.  `fork_page` forges a table that pages one address in twice.
SYN-LOOKUP-tied (`syn_lookup_tied`, `build_syn_lookup(shape, link=True, reads=True, pages=True, tied=True)`): SYN-LOOKUP-paged on the
OPEN bus (logup.py, "THE OPEN BUS"; ZKA1 version 8), ANOTHER description with its own control root.  One more term, the last one:
+p_on (p_addr, p_in, p_out) of tag 2 (logup.TIE_TAG), the page table's rows put on the bus that the seals of its page-out chain
(p2_page_tied.py) take them off.  out = SYN-LOOKUP-paged's 4 words ‖ alpha ‖ beta ‖ F (16 words): every term reads the two challenges
from `out`, and the `last` constraint closes on F = logup.table_fingerprint of the page table.  The witness is SYN-LOOKUP-paged's.
Not a shipped circuit: its control root is zkh_code_root of its code trace.
SYN-LOOKUP-reads-ported (`build_syn_lookup(shape, link=True, reads=True, ports=True)`): SYN-LOOKUP-reads' description BYTE FOR BYTE, and
another blob (ZKA1 version 9): the n_mem memory pairs are the PORTS of one memory, pair 0 the head and the others LINK records that join it
(logup.py, PORTS).  The terms of all pairs carry tag 1, so they were one bus all along; what changes is the witness: a row makes n_mem
accesses to ONE memory, in port order.  `witness(..., ports=True)` orders the accesses by (row, port), gives access (r, q) the time
n_mem r + q (+ 1 when paged) and shares one memory across the ports, and the host-made link columns come from one walk over that order.
`pages=True` with `ports=True` lifts n_mem = 1: the PAGES record names the head, every port's link constraints are the paged ones, and
the page table's four bus terms stand once for the whole memory.  n_mem A must stay below 2^(order_limbs L).
SYN-LOOKUP-paged-wide (`build_syn_lookup(shape, link=True, reads=True, pages=True, wide=True)`; `ports=True` is accepted as well): ANOTHER
description, SYN-LOOKUP-paged over a memory of TWO value words per address, the two halves of a 32-bit machine word (ZKA1 version 10).
Every memory pair gains a second value column and its previous value, after the pair's link limbs (`link_layout(wide=True)`: val1, pval1),
and the page table its 2 V value columns (`pages_layout(wide=True)`: p_on, p_addr, p_in_0, p_in_1, p_out_0, p_out_1, p_time, the limbs).  On
the bus (tag 1): the access +(addr, v0, v1, time), the previous access -(addr, pv0, pv1, ptime), the page-in +p_on (p_addr, p_in_0, p_in_1),
the key (addr, v0, v1, 0), and the page-out -p_on (p_addr, p_out_0, p_out_1, p_time).  The LINK carries (time, val, val1), the PAGES record
has V = 2, and logup.link_constraints states (1 - w)(c_j - prev_j) = 0 for both values.  The image is 2 W words, word j of address a at
2 a + j (`witness(..., wide=True)`).  It does not combine with `tied` as it is: its table's rows on the open bus need flat-address columns.
`flat=True` (with `wide`; ZKA1 version 11) gives them: the page table gains p_flat_0, p_flat_1 after its gap limbs (`pages_layout(flat=True)`),
the PAGES record has them as its flats, so the library fills them with 2 a_i + j, and logup.page_constraints adds p_on (p_flat_j - 2 p_addr
- j) = 0.  Without `tied` it is a closed-bus circuit of its own, whose two columns no term reads.
SYN-LOOKUP-tied-wide (`syn_lookup_tied_wide`, `build_syn_lookup(shape, link=True, reads=True, pages=True, wide=True, flat=True, tied=True)`;
`ports=True` is accepted): that circuit on the OPEN bus, out = 16 words as SYN-LOOKUP-tied's, ANOTHER description with its own control root.
Two more terms, the last ones: +p_on (p_flat_j, p_in_j, p_out_j) of tag 2 (logup.TIE_TAG), j = 0, 1: the rows of the FLAT table
(2 a_i + j, in_j, out_j), which is the table the page-out's proof holds and its chain takes off the bus.  `last` closes on
F = logup.table_fingerprint of that flat table.  `witness(..., wide=True, flat=True)` is the wide witness with the two columns.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np

from .desc import GROUP_CODE, GROUP_DATA, P
from .logup import TIE_TAG, LogupBuilder

N_CODE = 7
MEM_W = 3


def layout(n_words: int, n_limbs: int, n_mem: int):
    """data column indices: (words, limbs[k][j], m, mem tuples, permuted tuples)"""
    words = list(range(n_words))
    limbs = [[n_words + k * n_limbs + j for j in range(n_limbs)] for k in range(n_words)]
    m = n_words + n_words * n_limbs
    mem = [[m + 1 + MEM_W * i + e for e in range(MEM_W)] for i in range(n_mem)]
    perm = [[m + 1 + MEM_W * (n_mem + i) + e for e in range(MEM_W)] for i in range(n_mem)]
    return words, limbs, m, mem, perm


class Shape(NamedTuple):
    n_words: int
    n_limbs: int
    limb_bits: int
    n_mem: int = 1


TINY = Shape(2, 4, 4, 1)            # 11 terms in 4 accum columns (po2 8..12)
FULL = Shape(16, 4, 8, 1)           # 67 terms in 23 accum columns, 87 data columns (sealed at po2 20)
WIDE = Shape(2, 2, 16, 1)           # a 2^16-row table (po2 >= 17): 7 terms in 3 accum columns
MULTI = Shape(2, 4, 4, 3)           # three memory pairs: 15 terms in 5 accum columns (the batched sort)
SORT_KEYS = (0, 2)                  # (addr, time) of a memory tuple


ORDER_LIMBS = 3


def order_layout(n_words: int, n_limbs: int, n_mem: int, order_limbs: int = ORDER_LIMBS):
    """data column indices of SYN-LOOKUP-ordered's additions, after `layout`'s: per memory pair [flag, limb_0 .. limb_{order_limbs-1}]"""
    base = n_words + n_words * n_limbs + 1 + 2 * MEM_W * n_mem
    return [[base + (1 + order_limbs) * i + e for e in range(1 + order_limbs)] for i in range(n_mem)]


LINK_W = 7                          # addr, val, time, linked, last, pval, ptime


def link_layout(n_words: int, n_limbs: int, n_mem: int, order_limbs: int = ORDER_LIMBS, wide: bool = False):
    """data column indices of SYN-LOOKUP-linked's memory pairs, after `layout`'s m: per pair [addr, val, time, linked, last, pval, ptime,
    limb_0 .. limb_{order_limbs-1}]; wide: then [val1, pval1], the second value word and its previous one"""
    base = n_words + n_words * n_limbs + 1
    w = LINK_W + order_limbs + 2 * bool(wide)
    return [[base + w * i + e for e in range(w)] for i in range(n_mem)]


def reads_layout(n_words: int, n_limbs: int, n_mem: int, order_limbs: int = ORDER_LIMBS, wide: bool = False):
    """data column indices of SYN-LOOKUP-reads' write flags, one per memory pair, after `link_layout`'s columns"""
    base = n_words + n_words * n_limbs + 1 + (LINK_W + order_limbs + 2 * bool(wide)) * n_mem
    return [base + i for i in range(n_mem)]


PAGE_W = 5                          # p_on, p_addr, p_in, p_out, p_time
TIED_OUT, OUT_ALPHA, OUT_BETA, OUT_TOTAL = 16, 4, 8, 12      # SYN-LOOKUP-tied's out: 4 zero words ‖ alpha ‖ beta ‖ F


def pages_layout(n_words: int, n_limbs: int, n_mem: int = 1, order_limbs: int = ORDER_LIMBS, wide: bool = False, flat: bool = False):
    """data column indices of SYN-LOOKUP-paged's page table, after `reads_layout`'s write flag: [p_on, p_addr, p_in, p_out, p_time,
    alimb_0 .. alimb_{order_limbs-1}, gap_0 .. gap_{order_limbs-1}]; wide: [p_on, p_addr, p_in_0, p_in_1, p_out_0, p_out_1, p_time, the limbs]; flat (with wide):
    then [p_flat_0, p_flat_1], the flat addresses of the page's two words"""
    base = n_words + n_words * n_limbs + 1 + (LINK_W + order_limbs + 2 * bool(wide)) * n_mem + n_mem
    return [base + e for e in range(PAGE_W + 2 * bool(wide) + 2 * order_limbs + 2 * bool(flat))]


def build_syn_lookup(shape: Shape = FULL, derive: bool = False, sort: bool = False,
                     sort_keys: Tuple[int, ...] = SORT_KEYS, limbs: bool = False, order: bool = False,
                     order_limbs: int = ORDER_LIMBS, link: bool = False, reads: bool = False, pages: bool = False,
                     tied: bool = False, ports: bool = False, wide: bool = False, flat: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ZKC1 description, ZKA1 argument blob); derive: the table term's multiplicity is derived by the library (version-2 blob,
    the description unchanged); sort: every permuted copy is the library's sorted copy of its memory tuple by the tuple positions
    `sort_keys` (version-3 blob, the description unchanged); limbs: every word's limbs are a LIMBS record (version-4 blob, the
    description unchanged); order: SYN-LOOKUP-ordered, another description (module docstring), its order columns an ORDER record over
    the copy's (addr, time); link: SYN-LOOKUP-linked, another description (module docstring), its link columns a LINK record (version-5
    blob); it has no sorted copy, so it refuses `sort` and `order`; reads: SYN-LOOKUP-reads, SYN-LOOKUP-linked with a write flag per
    memory pair and the read rule (version-6 blob, another description); it needs `link`; pages: SYN-LOOKUP-paged, SYN-LOOKUP-reads
    with its one memory paged in from an image and out again (version-7 blob, another description); it needs `link`, `reads` and n_mem = 1; tied: SYN-LOOKUP-tied, SYN-LOOKUP-paged on the open bus with
    the page table's rows as one more term (version-8 blob, another description, 16 `out` words); it needs `pages`; ports: the n_mem memory
    pairs are the ports of ONE memory (version-9 blob; without `pages` SYN-LOOKUP-reads' description unchanged); it needs `link` and `reads`,
    and with it `pages` takes any n_mem; wide: SYN-LOOKUP-paged-wide, the paged memory holds two value words per address (version-10 blob,
    another description); it needs `pages`, takes `ports`, and refuses `tied` without `flat`; flat: the wide page table has the two
    flat-address columns p_flat_j = 2 p_addr + j (version-11 blob, another description); it needs `wide`, and with `tied` it is
    SYN-LOOKUP-tied-wide, whose tie terms are the flat table's rows"""
    n_words, n_limbs, limb_bits, n_mem = shape
    if flat and not wide:
        raise ValueError("build_syn_lookup: flat=True adds the flat-address columns of a memory of two value words per address: it needs wide=True")
    if wide and tied and not flat:
        raise ValueError("build_syn_lookup: tied=True with wide=True: the tie of a memory of two value words per address is not built (its table's rows on the "
                         "open bus need flat-address columns in the trace): flat=True adds them")
    if wide and not pages:
        raise ValueError("build_syn_lookup: wide=True gives the paged memory two value words per address: it needs pages=True")
    if tied and not pages:
        raise ValueError("build_syn_lookup: tied=True ties the page table of a paged memory to its page-out: it needs pages=True")
    if pages and not (link and reads):
        raise ValueError("build_syn_lookup: pages=True pages the memory of a LINK record with the read rule: it needs link=True, reads=True")
    if ports and not (link and reads):
        raise ValueError("build_syn_lookup: ports=True makes the memory pairs the ports of one memory with the read rule: it needs link=True, reads=True")
    if pages and n_mem != 1 and not ports:
        raise ValueError(f"build_syn_lookup: pages=True pages one memory: n_mem is {n_mem}")
    if reads and not link:
        raise ValueError("build_syn_lookup: reads=True is the read rule of the LINK records: it needs link=True")
    if link and (sort or order):
        raise ValueError("build_syn_lookup: link=True has no sorted copy: it does not combine with sort= / order=")
    words, limb_cols, m, mem, perm = layout(n_words, n_limbs, n_mem)
    ocols = order_layout(n_words, n_limbs, n_mem, order_limbs) if order else []
    lcols = link_layout(n_words, n_limbs, n_mem, order_limbs, wide) if link else []
    wd = m + 1 + 2 * MEM_W * n_mem + sum(len(c) for c in ocols)
    n_terms = n_words * n_limbs + 1 + 2 * n_mem + n_mem * order_limbs * bool(order)
    if link:
        wd = m + 1 + sum(len(c) for c in lcols) + n_mem * bool(reads)
        n_terms = n_words * n_limbs + 1 + 3 * n_mem + n_mem * order_limbs
    wcols = reads_layout(n_words, n_limbs, n_mem, order_limbs, wide) if reads else [None] * n_mem
    pcols = pages_layout(n_words, n_limbs, n_mem, order_limbs, wide, flat) if pages else []
    pw = PAGE_W + 2 * bool(wide)                                             # the table's columns before its limbs
    fcols = pcols[pw + 2 * order_limbs:]                                     # flat: p_flat_0, p_flat_1, after the limbs
    if pages:
        wd += len(pcols)
        n_terms += 2 - n_mem + 2 * order_limbs + (2 if flat else 1) * bool(tied)                     # a port: its access and its previous one; the table's two terms once
    k = (n_terms + 2) // 3
    if tied:
        b = LogupBuilder((4 * k, N_CODE, wd), (TIED_OUT, 8), alpha=OUT_ALPHA, beta=OUT_BETA, open_bus=(TIE_TAG, OUT_TOTAL))
    else:
        b = LogupBuilder((4 * k, N_CODE, wd), (4, 8), alpha=0, beta=4)
    code = lambda c: b.get(GROUP_CODE, c)
    data = lambda c: b.get(GROUP_DATA, c)
    one = b.const(1)
    active, first, body, _rowidx, last = (code(i) for i in range(5))
    limbs_flag, limbs = limbs, limb_cols
    # the terms, three per column in this order: limbs, the table, the memory pair (, the order limbs)
    specs = [dict(tuple_cols=[(GROUP_DATA, c)], tag=0) for row in limbs for c in row]
    specs.append(dict(tuple_cols=[(GROUP_CODE, 6)], sign=-1, sel=5, mult=(GROUP_DATA, m), tag=0, derive=derive))
    for i in range(n_mem if not link else 0):
        specs.append(dict(tuple_cols=[(GROUP_DATA, c) for c in mem[i]], sign=1, tag=1))
        copy = dict(sorted_from=len(specs) - 1, sort_keys=sort_keys) if sort else {}
        specs.append(dict(tuple_cols=[(GROUP_DATA, c) for c in perm[i]], sign=-1, tag=1, **copy))
    for c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *rest in lcols if pages else []:
        val1, pval1 = ([(GROUP_DATA, rest[-2])], [(GROUP_DATA, rest[-1])]) if wide else ([], [])
        specs.append(dict(tuple_cols=[(GROUP_DATA, c_addr), (GROUP_DATA, c_val)] + val1 + [(GROUP_DATA, c_time)], sign=1, tag=1))
        specs.append(dict(tuple_cols=[(GROUP_DATA, c_addr), (GROUP_DATA, c_pval)] + pval1 + [(GROUP_DATA, c_ptime)], sign=-1, tag=1))
    if wide:                                                                 # +p_on (p_addr, p_in_0, p_in_1), the key (addr, v0, v1, 0); -p_on (p_addr, p_out_0, p_out_1, p_time)
        specs.append(dict(tuple_cols=[(GROUP_DATA, pcols[e]) for e in (1, 2, 3)], sign=1, mult=(GROUP_DATA, pcols[0]), tag=1))
        specs.append(dict(tuple_cols=[(GROUP_DATA, pcols[e]) for e in (1, 4, 5, 6)], sign=-1, mult=(GROUP_DATA, pcols[0]), tag=1))
    elif pages:
        specs.append(dict(tuple_cols=[(GROUP_DATA, pcols[1]), (GROUP_DATA, pcols[2])], sign=1, mult=(GROUP_DATA, pcols[0]), tag=1))
        specs.append(dict(tuple_cols=[(GROUP_DATA, pcols[1]), (GROUP_DATA, pcols[3]), (GROUP_DATA, pcols[4])], sign=-1, mult=(GROUP_DATA, pcols[0]), tag=1))
    for c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *_ in [] if pages else lcols:
        specs.append(dict(tuple_cols=[(GROUP_DATA, c_addr), (GROUP_DATA, c_val), (GROUP_DATA, c_time)], sign=1, tag=1))
        specs.append(dict(tuple_cols=[(GROUP_DATA, c_addr), (GROUP_DATA, c_pval), (GROUP_DATA, c_ptime)], sign=-1, mult=(GROUP_DATA, c_linked), tag=1))
        specs.append(dict(tuple_cols=[(GROUP_DATA, c_addr), (GROUP_DATA, c_val), (GROUP_DATA, c_time)], sign=-1, mult=(GROUP_DATA, c_last), tag=1))
    specs += [dict(tuple_cols=[(GROUP_DATA, c)], tag=0) for cols in ocols for c in cols[1:]]
    specs += [dict(tuple_cols=[(GROUP_DATA, c)], tag=0) for cols in lcols for c in cols[LINK_W:LINK_W + order_limbs]]
    specs += [dict(tuple_cols=[(GROUP_DATA, c)], tag=0) for c in pcols[pw:pw + 2 * order_limbs]]
    if tied and flat:                                                        # the FLAT table's rows (2 a + j, in_j, out_j): one term per word
        for j in range(2):
            specs.append(dict(tuple_cols=[(GROUP_DATA, fcols[j]), (GROUP_DATA, pcols[2 + j]), (GROUP_DATA, pcols[4 + j])], sign=1, mult=(GROUP_DATA, pcols[0]), tag=TIE_TAG))
    elif tied:                                                               # the table's rows, for the page-out chain to take off the bus
        specs.append(dict(tuple_cols=[(GROUP_DATA, pcols[1]), (GROUP_DATA, pcols[2]), (GROUP_DATA, pcols[3])], sign=1, mult=(GROUP_DATA, pcols[0]), tag=TIE_TAG))
    for i, s in enumerate(specs):
        b.term(i // 3, **s)
    if limbs_flag:
        for kk in range(n_words):
            b.derive_limbs((GROUP_DATA, words[kk]), limbs[kk], limb_bits)
    records = [b.derive_order([(GROUP_DATA, perm[i][0]), (GROUP_DATA, perm[i][2])], cols, limb_bits) for i, cols in enumerate(ocols)]
    # the clock (time) is carried first, then the value; the destinations in the LINK's order: linked, last, ptime, pval, the limbs
    links = []
    for c, w in zip(lcols, wcols):                                           # ports: pair 0 is the head, the others join its memory
        carried, prevs = ([(GROUP_DATA, c[-2])], [c[-1]]) if wide else ([], [])                  # wide: the second value word and its previous one
        links.append(b.derive_links(None, (GROUP_DATA, c[0]), [(GROUP_DATA, c[2]), (GROUP_DATA, c[1])] + carried, [c[3], c[4], c[6], c[5]] + prevs + c[LINK_W:LINK_W + order_limbs],
                                    limb_bits, write=None if w is None else (GROUP_DATA, w), joins=links[0] if ports and links else None))
    table = None
    if pages:
        table = b.derive_pages(links[0], pcols[:pw + 2 * order_limbs], limb_bits, flats=fcols) if flat else b.derive_pages(links[0], pcols, limb_bits)
    # words = sum of their limbs, on active rows
    inner = b.true()
    for kk in range(n_words):
        acc = None
        for j in range(n_limbs):
            v = data(limbs[kk][j]) if j == 0 else b.mul(b.const(1 << (j * limb_bits)), data(limbs[kk][j]))
            acc = v if acc is None else b.add(acc, v)
        inner = b.and_eqz(inner, b.sub(data(words[kk]), acc))
    chain = b.and_cond(b.true(), active, inner)
    chain = b.arguments(chain, first, body, last)
    if records:
        inner = b.true()
        for rec in records:
            inner = b.order_constraints(inner, rec)
        chain = b.and_cond(chain, body, inner)
    if links:                                                                # every active row is an access, the first one included
        inner = b.true()
        for rec in links:
            inner = b.link_constraints(inner, rec)
        if table is not None:
            inner, body_inner = b.page_constraints(inner, b.true(), table)
        chain = b.and_cond(chain, active, inner)
        if table is not None:
            chain = b.and_cond(chain, body, body_inner)
    chain = b.and_eqz(chain, b.mul(active, b.sub(one, active)))
    chain = b.and_eqz(chain, b.mul(first, b.sub(one, first)))
    chain = b.and_eqz(chain, b.sub(b.sub(active, first), body))
    return b.finish_all(chain)


def syn_lookup_tiny() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY)


def syn_lookup() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL)


def syn_lookup_tiny_derived() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, derive=True)


def syn_lookup_derived() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, derive=True)


def syn_lookup_tiny_sorted() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, sort=True)


def syn_lookup_sorted() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, sort=True)


def syn_lookup_tiny_linked() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, link=True)


def syn_lookup_linked() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, link=True)


def syn_lookup_tiny_reads() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, link=True, reads=True)


def syn_lookup_reads() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, link=True, reads=True)


def syn_lookup_tiny_paged() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, link=True, reads=True, pages=True)


def syn_lookup_paged() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, link=True, reads=True, pages=True)


def syn_lookup_tiny_tied() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, link=True, reads=True, pages=True, tied=True)


def syn_lookup_tied() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, link=True, reads=True, pages=True, tied=True)


def syn_lookup_tiny_tied_wide() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(TINY, link=True, reads=True, pages=True, tied=True, wide=True, flat=True)


def syn_lookup_tied_wide() -> Tuple[np.ndarray, np.ndarray]:
    return build_syn_lookup(FULL, link=True, reads=True, pages=True, tied=True, wide=True, flat=True)


def _enc(x) -> np.ndarray:
    return ((np.asarray(x, dtype=np.uint64) % np.uint64(P)) * np.uint64((1 << 32) % P) % np.uint64(P)).astype(np.uint32)


def witness(shape: Shape, po2: int, zk_cycles: int, seed: int = 1, count: bool = True, sort: bool = True, addr_range: int = 1 << 20,
            sort_keys: Tuple[int, ...] = SORT_KEYS, limbs: bool = True, order=None, order_limbs: int = ORDER_LIMBS, link=None,
            reads: bool = False, pages=None, image=None, ports: bool = False, wide: bool = False, flat: bool = False):
    """-> (code, data, out_global) host arrays of raw Montgomery words: random words below min(P, 2^(n_limbs L)) split into limbs
    (limbs=False: zero, for the library to split), the table's multiplicities (count=False: zero, for the library to derive), random
    memory tuples (addresses below `addr_range`) and their copy stably sorted by the tuple positions `sort_keys`, (addr, time)
    (sort=False: zero, for the library to sort); blinding rows of data from the same seeded generator.
    order: None = the plain shape; True / False = SYN-LOOKUP-ordered's witness (`build_syn_lookup(order=True)`), its order columns
    filled from the sorted copy (and their limbs counted in the multiplicities) / left zero for the library.
    link: None = no link; True / False = SYN-LOOKUP-linked's witness (`build_syn_lookup(link=True)`): no copy, the times are the row
    numbers, and linked, last, pval, ptime and the limbs of time - ptime - 1 are host-made by a walk over the rows with a dictionary,
    one access after another (and the limbs counted) / left zero for the library.
    reads: SYN-LOOKUP-reads' witness (`build_syn_lookup(link=True, reads=True)`; it needs `link` True or False): a load / store trace.
    Every access draws a write flag, and a load takes the value the previous access to its address left, or 0 without one; the write
    flags are the host's column whatever `link` says.
    pages: None = no paging; True / False = SYN-LOOKUP-paged's witness (`build_syn_lookup(link=True, reads=True, pages=True)`; it needs
    `link`, `reads` and `image`, the W raw Montgomery words of the memory image, each below P): the times are row + 1, the addresses
    below min(addr_range, W), a load takes the last store or else the image's word, an access without a previous one has (pval, ptime) =
    (image word, 0) and the limbs of time - 1, and the page table is host-made by a walk over the sorted distinct addresses (its limbs
    counted) / left zero for the library.
    ports: SYN-LOOKUP-reads-ported's witness (`build_syn_lookup(..., ports=True)`; it needs `link` and `reads`): the n_mem pairs are the
    ports of one memory.  The accesses are ordered by (row, port), access (r, q) has the time n_mem r + q (+ 1 when paged), a load takes
    what the previous access of ANY port left at its address, and the link columns (and the one page table) are host-made by one walk
    over that order with a dictionary.
    wide: SYN-LOOKUP-paged-wide's witness (`build_syn_lookup(..., pages=True, wide=True)`; it needs `pages`): two value words per address.
    `image` is the FLAT image of 2 W words, word j of address a at 2 a + j; every access has a second value column, a load takes both
    words of the last store or of the image, and the page table carries p_in_0, p_in_1, p_out_0, p_out_1.  The addresses, write flags and
    clocks of a seed are those of the witness without `wide` over an image of W words.
    flat: the witness of `build_syn_lookup(..., wide=True, flat=True)` (it needs `wide`): the page table's two flat-address columns,
    2 a_i + j on the table's rows, host-made when `pages` is True and zero when it is False.  Nothing new is drawn: the addresses, flags,
    clocks and values of a seed are those of the wide witness (the blinding rows, drawn last, cover two more columns)"""
    if flat and not wide:
        raise ValueError("witness: flat=True adds the flat-address columns of a memory of two value words per address: it needs wide=True")
    if wide and pages is None:
        raise ValueError("witness: wide=True gives the paged memory two value words per address: it needs pages=")
    if ports and (link is None or not reads):
        raise ValueError("witness: ports=True makes the pairs the ports of one memory with the read rule: it needs link= and reads=True")
    if pages is not None and (link is None or not reads or image is None):
        raise ValueError("witness: pages= pages the memory of the LINK record with the read rule: it needs link=, reads=True and image=")
    if reads and link is None:
        raise ValueError("witness: reads=True is the read rule of the LINK records: it needs link=True or link=False")
    n_words, n_limbs, limb_bits, n_mem = shape
    words, limb_cols, m_col, mem, perm = layout(n_words, n_limbs, n_mem)
    limbs_on, limbs = limbs, limb_cols
    ocols = order_layout(n_words, n_limbs, n_mem, order_limbs) if order is not None else []
    lcols = link_layout(n_words, n_limbs, n_mem, order_limbs, wide) if link is not None else []
    wd = m_col + 1 + (sum(len(c) for c in lcols) + n_mem * bool(reads) if lcols else 2 * MEM_W * n_mem + sum(len(c) for c in ocols))
    wcols = reads_layout(n_words, n_limbs, n_mem, order_limbs, wide) if reads else []
    pcols = pages_layout(n_words, n_limbs, n_mem, order_limbs, wide, flat) if pages is not None else []
    V = 2 if wide else 1
    wd += len(pcols)
    pcols, fcols = (pcols[:-2], pcols[-2:]) if flat else (pcols, [])         # the walks fill the table's own columns, then the flat ones
    n = 1 << po2
    A = n - zk_cycles
    T = 1 << limb_bits
    if pcols:
        assert n_mem == 1 or ports, "one memory is paged"
        image = np.asarray(image, dtype=np.uint32).reshape(-1)
        assert (image < P).all(), "the witness holds canonical Montgomery words: an image word >= P has no host-made twin"
        assert (n_mem if ports else 1) * A < 1 << (order_limbs * limb_bits), f"times reach {(n_mem if ports else 1) * A}: they do not fit {order_limbs} limbs of {limb_bits} bits"
        held0 = (image.astype(np.uint64) * np.uint64(pow((1 << 32) % P, -1, P)) % np.uint64(P)).tolist()     # the image, canonical
        assert image.size % V == 0, "the flat image of a wide memory has two words per address"
        addr_range = min(addr_range, image.size // V, 1 << (order_limbs * limb_bits))
    assert A >= T, f"po2 {po2}: {A} active rows do not hold the {T}-row table"
    rng = np.random.default_rng(seed)
    code = np.zeros((N_CODE, n), dtype=np.uint64)
    rows = np.arange(n, dtype=np.uint64)
    code[0, :A] = 1
    code[1, 0] = 1
    code[2, 1:A] = 1
    code[3, :A] = rows[:A]
    code[4, A - 1] = 1
    code[5, :T] = 1
    code[6, :T] = rows[:T]
    data = np.zeros((wd, n), dtype=np.uint64)
    hi = min(P, 1 << (n_limbs * limb_bits))
    counts = np.zeros(T, dtype=np.int64)
    for kk in range(n_words):
        w = rng.integers(0, hi, size=A, dtype=np.uint64)
        data[words[kk], :A] = w
        for j in range(n_limbs):
            limb = (w >> np.uint64(j * limb_bits)) & np.uint64(T - 1)
            if limbs_on:
                data[limbs[kk][j], :A] = limb
            counts += np.bincount(limb.astype(np.int64), minlength=T)
    if ports:
        _ported_witness(data, rng, lcols, wcols, pcols, held0 if pcols else None, A, addr_range, limb_bits, order_limbs, link, pages, counts, wide, fcols)
    for i in range(0 if ports else n_mem):
        addr = rng.integers(0, addr_range, size=A, dtype=np.uint64)
        val = rng.integers(0, P, size=A, dtype=np.uint64)
        time = rng.permutation(A).astype(np.uint64)
        if wcols:                                                            # a load returns what the previous access left, or 0
            store = rng.integers(0, 2, size=A, dtype=np.uint64)
            val1 = rng.integers(0, P, size=A, dtype=np.uint64) if wide else None       # drawn last: the other draws are those of the narrow witness
            held = {}
            for r, a in enumerate(addr.tolist()):
                if not store[r]:
                    val[r] = held.get(a, held0[V * a] if pcols else 0)
                held[a] = val[r]
            held = {}
            for r, a in enumerate(addr.tolist() if wide else []):            # the second word: a load takes the last store's, or the image's
                if not store[r]:
                    val1[r] = held.get(a, held0[2 * a + 1])
                held[a] = val1[r]
            data[wcols[i], :A] = store
        if pcols:
            _paged_witness(data, lcols[i], pcols, addr, val, held0, A, limb_bits, order_limbs, link, pages, counts, val1 if wide else None, fcols)
            continue
        if lcols:
            _link_witness(data, lcols[i], addr, val, A, limb_bits, order_limbs, link, counts)
            continue
        tup = (addr, val, time)
        by = np.lexsort(tuple(tup[pos] for pos in sort_keys[::-1]))
        for e, v in enumerate(tup):
            data[mem[i][e], :A] = v
            if sort:
                data[perm[i][e], :A] = v[by]
        if ocols:                                                            # the order witness of the sorted (addr, time)
            k0, k1 = addr[by].astype(np.int64), time[by].astype(np.int64)
            same = np.zeros(A, dtype=np.int64)
            same[1:] = k0[1:] == k0[:-1]
            d = np.zeros(A, dtype=np.int64)
            d[1:] = np.where(same[1:] == 1, k1[1:] - k1[:-1], k0[1:] - k0[:-1] - 1)
            assert (d >= 0).all() and (d >> (order_limbs * limb_bits) == 0).all(), "an ordered difference does not fit the order limbs"
            if order:
                data[ocols[i][0], :A] = same.astype(np.uint64)
            for j in range(order_limbs):
                limb = (d >> (j * limb_bits)) & (T - 1)
                if order:
                    data[ocols[i][1 + j], :A] = limb.astype(np.uint64)
                counts += np.bincount(limb, minlength=T)
    if count:
        data[m_col, :T] = counts.astype(np.uint64)
    data[:, A:] = rng.integers(0, P, size=(wd, n - A), dtype=np.uint64)
    return _enc(code).reshape(-1), _enc(data).reshape(-1), np.zeros(4, dtype=np.uint32)


def _link_witness(data, cols, addr, val, A, limb_bits, order_limbs, fill, counts):
    """one memory pair of SYN-LOOKUP-linked: the host's way, a sequential walk with the last access of every address in a dictionary"""
    c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *c_limbs = cols
    T = 1 << limb_bits
    time = np.arange(A, dtype=np.uint64)
    data[c_addr, :A], data[c_val, :A], data[c_time, :A] = addr, val, time
    seen, prev = {}, [-1] * A
    for r, a in enumerate(addr.tolist()):                                    # the walk: the last access to every address so far
        prev[r] = seen.get(a, -1)
        seen[a] = r
    prev = np.asarray(prev, dtype=np.int64)
    on = prev >= 0
    q = np.where(on, prev, 0)
    linked, last = on.astype(np.uint64), np.ones(A, dtype=np.uint64)
    last[prev[on]] = 0
    pval, ptime = np.where(on, val[q], 0).astype(np.uint64), np.where(on, time[q], 0).astype(np.uint64)
    d = np.where(on, np.arange(A, dtype=np.int64) - q - 1, 0)
    assert (d >> (order_limbs * limb_bits) == 0).all(), "a time difference does not fit the link limbs"
    if fill:
        data[c_linked, :A], data[c_last, :A], data[c_pval, :A], data[c_ptime, :A] = linked, last, pval, ptime
    for j, c in enumerate(c_limbs):
        limb = (d >> (j * limb_bits)) & (T - 1)
        if fill:
            data[c, :A] = limb.astype(np.uint64)
        counts += np.bincount(limb, minlength=T)


def _paged_witness(data, cols, pcols, addr, val, image, A, limb_bits, order_limbs, fill, fill_pages, counts, val1=None, fcols=()):
    """the memory pair of SYN-LOOKUP-paged: `_link_witness` with times row + 1 and the image (canonical words) behind every first access,
    and the page table from a walk over the distinct addresses in order.  val1: the second value word of every access (wide: the image
    is flat, two words per address, and the pair's columns end on val1, pval1).  fcols: the two flat-address columns, or none"""
    c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *c_limbs = cols
    V = 1 if val1 is None else 2
    if V == 2:
        *c_limbs, c_val1, c_pval1 = c_limbs
    T = 1 << limb_bits
    time = np.arange(1, A + 1, dtype=np.uint64)
    data[c_addr, :A], data[c_val, :A], data[c_time, :A] = addr, val, time
    seen, first, prev = {}, {}, [-1] * A
    for r, a in enumerate(addr.tolist()):
        prev[r] = seen.get(a, -1)
        first.setdefault(a, r)
        seen[a] = r
    prev = np.asarray(prev, dtype=np.int64)
    on = prev >= 0
    q = np.where(on, prev, 0)
    linked, last = on.astype(np.uint64), np.ones(A, dtype=np.uint64)
    last[prev[on]] = 0
    img = np.asarray(image, dtype=np.uint64)
    pval, ptime = np.where(on, val[q], img[V * addr.astype(np.int64)]).astype(np.uint64), np.where(on, time[q], 0).astype(np.uint64)
    d = time.astype(np.int64) - ptime.astype(np.int64) - 1
    assert (d >> (order_limbs * limb_bits) == 0).all(), "a time difference does not fit the link limbs"
    if V == 2:
        data[c_val1, :A] = val1
    if fill:
        data[c_linked, :A], data[c_last, :A], data[c_pval, :A], data[c_ptime, :A] = linked, last, pval, ptime
        if V == 2:
            data[c_pval1, :A] = np.where(on, val1[q], img[2 * addr.astype(np.int64) + 1]).astype(np.uint64)
    for j, c in enumerate(c_limbs):
        limb = (d >> (j * limb_bits)) & (T - 1)
        if fill:
            data[c, :A] = limb.astype(np.uint64)
        counts += np.bincount(limb, minlength=T)
    below = -1
    for i, a in enumerate(sorted(seen)):                                     # the page table: one row per distinct address, in order
        gap = a - below - 1 if i else 0
        ins, outs = [image[V * a + j] for j in range(V)], [int(val[seen[a]])] + ([int(val1[seen[a]])] if V == 2 else [])
        row = [1, a] + ins + outs + [int(time[seen[a]])] + [(a >> (j * limb_bits)) & (T - 1) for j in range(order_limbs)] + \
            [(gap >> (j * limb_bits)) & (T - 1) for j in range(order_limbs)]
        assert a >> (order_limbs * limb_bits) == 0
        if fill_pages:
            data[pcols, i] = row
            if len(fcols):
                data[fcols, i] = [2 * a, 2 * a + 1]
        for v in row[3 + 2 * V:]:
            counts[v] += 1
        below = a
    counts[0] += 2 * order_limbs * (A - len(seen))                           # the rows below the table look their zero limbs up as well


def _ported_witness(data, rng, lcols, wcols, pcols, image, A, addr_range, limb_bits, order_limbs, fill, fill_pages, counts, wide=False, fcols=()):
    """the k memory pairs of SYN-LOOKUP-reads-ported as the ports of ONE memory, the host's way: one sequential walk over the accesses in
    (row, port) order with the last access of every address in a dictionary.  image: the paged memory's image (canonical words), or None.
    wide: two value words per address (the image flat, the pairs' columns ending on val1, pval1)"""
    k, T, paged, V = len(lcols), 1 << limb_bits, image is not None, 2 if wide else 1
    assert k * A < 1 << (order_limbs * limb_bits), f"times reach {k * A}: they do not fit {order_limbs} limbs of {limb_bits} bits"
    addr = [rng.integers(0, addr_range, size=A, dtype=np.uint64).tolist() for _ in range(k)]
    val = [rng.integers(0, P, size=A, dtype=np.uint64).tolist() for _ in range(k)]
    store = [rng.integers(0, 2, size=A, dtype=np.uint64).tolist() for _ in range(k)]
    val1 = [rng.integers(0, P, size=A, dtype=np.uint64).tolist() for _ in range(k)] if wide else None     # drawn last: the other draws are the narrow witness's
    seen, first = {}, {}                                                     # address -> (row, port) of its last / first access so far
    cols = [np.zeros((LINK_W + order_limbs + 2 * wide, A), dtype=np.uint64) for _ in range(k)]
    for r in range(A):
        for q in range(k):                                                   # the walk: every access after the one before it in (row, port) order
            a, time = addr[q][r], k * r + q + paged
            at = seen.get(a)
            if not store[q][r]:                                              # a load returns what the previous access left, the image's word or 0
                val[q][r] = val[at[1]][at[0]] if at is not None else image[V * a] if paged else 0
                if wide:
                    val1[q][r] = val1[at[1]][at[0]] if at is not None else image[2 * a + 1]
            pval, ptime = (val[at[1]][at[0]], k * at[0] + at[1] + paged) if at is not None else (image[V * a] if paged else 0, 0)
            d = time - ptime - 1 if at is not None or paged else 0
            assert 0 <= d < 1 << (order_limbs * limb_bits), "a time difference does not fit the link limbs"
            limbs = [(d >> (j * limb_bits)) & (T - 1) for j in range(order_limbs)]
            more = [val1[q][r], val1[at[1]][at[0]] if at is not None else image[2 * a + 1]] if wide else []
            cols[q][:, r] = [a, val[q][r], time, at is not None, 1, pval, ptime] + limbs + more
            if at is not None:
                cols[at[1]][4, at[0]] = 0                                    # it is no longer the last access of its address
            for v in limbs:
                counts[v] += 1
            first.setdefault(a, (r, q))
            seen[a] = (r, q)
    for q in range(k):
        keep = slice(0, None) if fill else slice(0, 3)                       # addr, val, time are the host's whoever fills the rest
        data[lcols[q][keep], :A] = cols[q][keep]
        if wide:
            data[lcols[q][-2], :A] = cols[q][-2]                             # ... and so is the second value word
        data[wcols[q], :A] = store[q]
    if not paged:
        return
    below = -1
    for i, a in enumerate(sorted(seen)):                                     # the page table: one row per distinct address, in order
        gap = a - below - 1 if i else 0
        (r, q) = seen[a]
        ins, outs = [image[V * a + j] for j in range(V)], [val[q][r]] + ([val1[q][r]] if wide else [])
        row = [1, a] + ins + outs + [k * r + q + 1] + [(a >> (j * limb_bits)) & (T - 1) for j in range(order_limbs)] + \
            [(gap >> (j * limb_bits)) & (T - 1) for j in range(order_limbs)]
        assert a >> (order_limbs * limb_bits) == 0
        if fill_pages:
            data[pcols, i] = row
            if len(fcols):
                data[fcols, i] = [2 * a, 2 * a + 1]
        for v in row[3 + 2 * V:]:
            counts[v] += 1
        below = a
    counts[0] += 2 * order_limbs * (A - len(seen))                           # the rows below the table look their zero limbs up as well


def fork_page(shape: Shape, data, po2: int, zk_cycles: int, image, order_limbs: int = ORDER_LIMBS):
    """-> (a copy of SYN-LOOKUP-paged's host-made `data` in which one address is paged in TWICE, the row of the second page).  A store r
    that is linked (it has an earlier access to its address a) is cut loose: it takes (image[a], 0) as its previous access, as a first
    access would, with the limbs of time - 1.  The tuple its earlier access left is then paged out by a second table row for a, put
    right after a's own (the rows below move down by one; the limbs are a's, the gap limbs zeros, which the table holds): + p_on
    (a, image[a]) twice against the two removals, and the bus balances.  The multiplicities have to be counted again.  Only
    logup.page_constraints objects, on the second row: its address does not exceed the one before."""
    n = 1 << po2
    A = n - zk_cycles
    d = np.array(data, dtype=np.uint32).reshape(-1, n)
    image = np.asarray(image, dtype=np.uint32).reshape(-1)
    c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *c_limbs = link_layout(shape.n_words, shape.n_limbs, shape.n_mem, order_limbs)[0]
    c_w = reads_layout(shape.n_words, shape.n_limbs, shape.n_mem, order_limbs)[0]
    pcols = pages_layout(shape.n_words, shape.n_limbs, shape.n_mem, order_limbs)
    R, T = (1 << 32) % P, 1 << shape.limb_bits
    rinv = pow(R, -1, P)
    dec = lambda v: int(v) % P * rinv % P
    D = int((d[pcols[0], :A] != 0).sum())
    assert D < A, "the table has no free row"
    r = next(r for r in range(A // 2, A) if d[c_w, r] != 0 and d[c_linked, r] != 0)      # a linked store
    a = dec(d[c_addr, r])
    i = next(i for i in range(D) if dec(d[pcols[1], i]) == a)
    second = [R, d[c_addr, r], image[a], d[c_pval, r], d[c_ptime, r]] + [d[pcols[PAGE_W + j], i] for j in range(order_limbs)] + [0] * order_limbs
    d[pcols, i + 2:D + 1] = d[pcols, i + 1:D].copy()
    d[pcols, i + 1] = second
    d[c_pval, r], d[c_ptime, r] = image[a], 0
    for j, c in enumerate(c_limbs):
        d[c, r] = ((dec(d[c_time, r]) - 1) >> (j * shape.limb_bits)) % T * R % P
    return d.reshape(-1), i + 1


def witness_equal_keys(shape: Shape, po2: int, zk_cycles: int, seed: int = 1, sort: bool = True, addr_range: int = 5):
    """the witness of `build_syn_lookup(shape, sort=True, sort_keys=(0,))`: addresses from a handful of values and the address the only
    key, so that every key is shared by many rows of distinct (val, time) and only a STABLE sort reproduces the permuted copy"""
    return witness(shape, po2, zk_cycles, seed=seed, sort=sort, addr_range=addr_range, sort_keys=(0,))


def corrupt_limb(shape: Shape, data, po2: int, row: int, word: int = 0) -> np.ndarray:
    """a copy of `data` in which limb 0 of word `word` on `row` is raised by 2^L — outside the table — and the word by the same
    amount, so that the decomposition still holds and only the lookup can object; the multiplicities are unchanged"""
    words, limbs, _m, _mem, _perm = layout(shape.n_words, shape.n_limbs, shape.n_mem)
    n = 1 << po2
    d = np.array(data, dtype=np.uint32).reshape(-1, n)
    add = (1 << shape.limb_bits) * ((1 << 32) % P) % P
    for c in (limbs[word][0], words[word]):
        d[c, row] = (int(d[c, row]) + add) % P
    return d.reshape(-1)


def swap_sorted_rows(shape: Shape, data, po2: int, row: int, pair: int = 0) -> np.ndarray:
    """a copy of `data` in which rows `row` and `row + 1` of the sorted copy of memory pair `pair` change places: still a permutation of
    the memory tuples, so the bus balances, but no longer in (addr, time) order — only SYN-LOOKUP-ordered's constraints object"""
    perm = layout(shape.n_words, shape.n_limbs, shape.n_mem)[4][pair]
    d = np.array(data, dtype=np.uint32).reshape(-1, 1 << po2)
    d[perm, row], d[perm, row + 1] = d[perm, row + 1].copy(), d[perm, row].copy()
    return d.reshape(-1)


def relink_row(shape: Shape, data, po2: int, row: int, pair: int = 0, order_limbs: int = ORDER_LIMBS) -> np.ndarray:
    """a copy of SYN-LOOKUP-linked's `data` in which the access `row` points at the NEXT access to its address (row2) instead of the
    previous one.  The other pointers move so that every tuple is still removed exactly once and the bus balances: row2 takes over
    what `row` pointed at, and the access after row2 (row3) points at `row`; where row2 is the last one, `last` moves from row2 to
    `row` instead.  The limbs of the rows touched are set to those of |time - ptime - 1| — in the table's range, so the lookups can be
    answered once the multiplicities are counted again — and only logup.link_constraints on `row`, linked forward in time, objects"""
    n = 1 << po2
    d = np.array(data, dtype=np.uint32).reshape(-1, n)
    c_addr, c_val, c_time, c_linked, c_last, c_pval, c_ptime, *c_limbs = link_layout(shape.n_words, shape.n_limbs, shape.n_mem, order_limbs)[pair]
    later = row + 1 + np.nonzero((d[c_addr, row + 1:] == d[c_addr, row]) & (d[c_linked, row + 1:] != 0))[0]
    assert later.size, f"row {row} is the last access to its address: nothing to relink it to"
    row2 = int(later[0])
    rinv, R = pow((1 << 32) % P, -1, P), (1 << 32) % P
    dec = lambda c, r: int(d[c, r]) % P * rinv % P
    old = [d[c, row].copy() for c in (c_linked, c_pval, c_ptime)]
    d[c_linked, row], d[c_pval, row], d[c_ptime, row] = d[c_linked, row2], d[c_val, row2], d[c_time, row2]
    d[c_linked, row2], d[c_pval, row2], d[c_ptime, row2] = old
    touched = [row, row2]
    if later.size > 1:
        row3 = int(later[1])
        d[c_pval, row3], d[c_ptime, row3] = d[c_val, row], d[c_time, row]
        touched.append(row3)
    else:
        d[c_last, row], d[c_last, row2] = d[c_last, row2], d[c_last, row]
    for r in touched:
        diff = abs(dec(c_time, r) - dec(c_ptime, r) - 1) if dec(c_linked, r) else 0
        for j, c in enumerate(c_limbs):
            d[c, r] = ((diff >> (j * shape.limb_bits)) & ((1 << shape.limb_bits) - 1)) * R % P
    return d.reshape(-1)


def misread_row(shape: Shape, data, po2: int, zk_cycles: int, row=None, pair: int = 0, order_limbs: int = ORDER_LIMBS):
    """-> (a copy of SYN-LOOKUP-reads' host-made `data` in which the load at `row` returns its value plus one, row).  row = None picks a
    load that is the last access to its address, from the middle of the trace on: its +1 and -last terms take the forged value from the
    same row, so the bus balances as it is.  A load that has a next access gets that access's pval moved with it, and the bus balances
    again.  No lookup reads a value, so the multiplicities are the same when they are counted again.  Only the read rule objects: on
    `row`, and, where the next access is a load itself, on that later row as well"""
    n = 1 << po2
    A = n - zk_cycles
    d = np.array(data, dtype=np.uint32).reshape(-1, n)
    c_addr, c_val, _time, _linked, c_last, c_pval, *_ = link_layout(shape.n_words, shape.n_limbs, shape.n_mem, order_limbs)[pair]
    c_w = reads_layout(shape.n_words, shape.n_limbs, shape.n_mem, order_limbs)[pair]
    if row is None:
        loads = np.nonzero((d[c_w, :A] == 0) & (d[c_last, :A] != 0))[0]
        assert loads.size, "no load is the last access to its address"
        row = int(loads[np.searchsorted(loads, A // 2) % loads.size])
    assert d[c_w, row] == 0, f"row {row} is a store"
    d[c_val, row] = (int(d[c_val, row]) + (1 << 32) % P) % P
    later = row + 1 + np.nonzero(d[c_addr, row + 1:A] == d[c_addr, row])[0]
    if later.size:
        d[c_pval, int(later[0])] = d[c_val, row]
    return d.reshape(-1), row
