"""Lookup and permutation arguments as data: log-derivative ("LogUp") sums in the accum group (DESIGN.md §2 ARGUMENTS).

One source gives two artefacts:
  * the ordinary ZKC1 description (desc.py) whose constraints check the accum columns — the prover, the eval_check generator,
    the bound verifier and both verifiers read it unchanged;
  * the ZKA1 argument blob that tells the library's built-in accumulate (csrc/accumulate.hip, zkh_accumulate) how to fill those
    columns from (code, data, mix).  csrc/arguments.hip decodes it into the mirror of `Arguments` below and checks the same rules.

A TERM of accum Fp4 column c has the value on row r

    t(r) = sign * sel(r) * m(r) / (alpha - (tag + beta v_0(r) + beta^2 v_1(r) + ... + beta^w v_{w-1}(r)))

with alpha, beta Fp4 challenges read from the mix globals (drawn after code and data are committed), sel a code column (or 1),
m a code / data column (or 1), v_j code / data columns at back 0 (w <= 4).  Accum column c holds the running sum over the active
rows, S_c[r] = sum_{r' <= r} sum_{terms i of c} t_i(r'); rows [A, n) are blinding noise.  The tags make the terms one bus: all
terms of all arguments together sum to zero, sum_c S_c[A-1] = 0.

Constraints (Fp steps, Fp4 arithmetic written out as syn_air.py's ext_mul), with D = prod_i d_i over the terms of c:
  first: S_c D - sum_i sign_i sel_i m_i prod_{l != i} d_l = 0
  body : (S_c - S_c@1) D - (the same) = 0
  last : sum_c S_c = 0
The degree of a column's constraint is 1 (gate) + max(1 + t, max_i(deg sel_i + deg m_i) + t - 1) for t terms; CHECK_SIZE 16
(4 pieces) bounds it at 5, so a column holds at most 3 terms.  The builder refuses anything above 5.

ZKA1 layout (u32 words; canonical integers, not Montgomery words)::

    [0] magic 'ZKA1' = 0x5a4b4131   [1] version = 1 .. 11     [2] k = accum Fp4 columns   [3] alpha mix word offset
    [4] beta mix word offset       [5] n_terms       [6] reserved = 0 (version 4: n_records)
    [7] reserved = 0 (version 6: the number of LINK records with READS, at least 1; version 7: that number | 0x10000)
    terms: n_terms x 16 words, sorted by column:
      col, neg (0: +1, 1: -1), sel (code column or NONE), m_group (NONE = constant 1, else GROUP_CODE / GROUP_DATA), m_col,
      tag, w, flags, then w (group, column) pairs of the tuple, unused pairs 0
    flags (word 7): version 1 writes 0 and reads nothing; version 2: bit 0 = the multiplicity is DERIVED by the library
    (zkh_derive_multiplicities), any other bit is refused.  The builder writes version 2 only when a term is derived.
    Version 3: bit 0 as in version 2; bit 1 = this term D is a DERIVED SORTED COPY (zkh_derive_sorted) of its source term S, and then
    bits 4..6 = nkeys (1..min(w, 3)), bits 8 + 2j, 9 + 2j = the tuple position of sort key j (most significant key first),
    bits 16..31 = the blob index of S.  Without bit 1 everything above bit 0 is zero; bits 2, 3, 7 and the position fields of unused
    keys are reserved and refused.  The builder writes version 3 only when a term is a sorted copy.
    Version 4: word 7 as in version 3; header word 6 = n_records, and n_records DERIVED-COLUMN RECORDS of 16 words follow the terms:
      kind (1 = LIMBS, 2 = ORDER), L = limb bits (1..16), nl = limbs (1..8, L nl <= 32), n_src (LIMBS: 1; ORDER: 1 or 2),
      two (group, column) source pairs (the unused one 0), then 8 destination data columns (ORDER with two keys: the flag column
      first, then the nl <= 7 limb columns; unused words 0).  The builder writes version 4 only when a record exists.
    Version 5: as version 4, and a record may be of kind 3 = LINK, which takes two 16-word slots (32 words; n_records counts records, not
    slots).  LINK records come after every LIMBS / ORDER record.  Its words:
      [0] kind = 3   [1] L = limb bits (1..16)   [2] nl = limbs (0..4, L nl <= 29)   [3] nc = carried columns (1..3)
      [4] sel (code column or NONE)   [5] reserved = 0   [6], [7] the key's (group, column)
      [8 + 2j], [9 + 2j] the (group, column) of carried column c_j, j < 3 (unused pairs 0)   [14], [15] reserved = 0
      [16 ..] the 2 + nc + nl destination data columns: linked, last, prev_0 .. prev_{nc-1}, limb_0 .. limb_{nl-1}; the words after
      them up to [31] reserved = 0.  The builder writes version 5 only when a LINK record exists.
    Version 6: as version 5, and a LINK record may carry the READ RULE.  LINK word [5] is a flag word: bit 0 = READS, every other bit
    is refused; with READS words [14], [15] are the (group, column) of the WRITE FLAG w, without it they are 0.  READS needs nc >= 2 (a
    clock and a value column).  Header word 7 = the number of LINK records with READS; a version-6 blob in which it is 0 is no ZKA1
    blob, and one in which it is not that number is refused.  The builder writes version 6 only when a LINK record has READS.

    Version 7: as version 6, and the blob holds ONE record of kind 4 = PAGES (32 words), after every LINK record:
      [0] kind = 4   [1] L = limb bits (1..16)   [2] ng = limbs (1..4, L ng <= 29)   [3] the blob record index of the LINK record it pages
      [4 .. 15] reserved = 0   [16 ..] the 5 + 2 ng destination data columns p_on, p_addr, p_in, p_out, p_time, alimb_0 .. alimb_{ng-1},
      gap_0 .. gap_{ng-1}; the words after them reserved = 0.  The LINK it names has READS and nc = 2 (a clock and one value column); its own
      32 words are what version 6 writes.  Header word 7 = (the READS count) | 0x10000: a version-7 blob without bit 16 is no ZKA1 blob, bit
      16 without a PAGES record is refused.  The builder writes version 7 only when a PAGES record exists (`derive_pages`).

    Version 8: version 7's layout, and the blob ends on ONE record of kind 5 = OPEN (16 words), after every other record:
      [0] kind = 5   [1] the open tag   [2], [3], [4] the `out` word offsets of alpha, beta and the total (4 words each, pairwise
      disjoint)   [5] the circuit's `out` words   [6 .. 15] reserved = 0.  Header words 3, 4 repeat the offsets of alpha and beta: they
      are `out` offsets, not mix offsets.  Header word 7 = (the READS count) | 0x10000 exactly when the blob holds a PAGES record | 0x20000:
      a version-8 blob without bit 17 is no ZKA1 blob, bit 17 without an OPEN record is refused; neither a READS count nor a PAGES record
      is required.  The builder writes version 8 only when an OPEN record exists.

    Version 9: version 8's layout, but the OPEN record is no longer required, and a LINK record may JOIN the memory of an earlier LINK
      record, its HEAD.  LINK word [5]: bit 0 = READS, bit 1 = JOINS, every other bit is refused; with JOINS word [31] is the blob record
      index of the head, without it word [31] stays reserved = 0.  Header word 7 = (the READS count) | 0x10000 exactly when the blob holds a
      PAGES record | 0x20000 exactly when it holds an OPEN record | 0x40000 (bit 18, PORTS) exactly when a LINK joins: a version-9 blob
      without bit 18 is no ZKA1 blob, bit 18 with no joining record is refused.  The builder writes version 9 only when a record joins
      (`derive_links(..., joins=head)`).

    Version 10: version 9's layout, and the PAGES record may page a memory of V = 2 VALUE WORDS per address: it may name a LINK with READS
      and nc = 3 (a clock and two value columns; its ports, if any, share the head's nc as they must).  PAGES word [4] holds V - 1: 0 means
      one word, which is what every earlier blob holds there; a value above 1, and one that is not the LINK's nc - 2, is refused.  The
      record has 3 + 2 V + 2 ng destinations, in this order: p_on, p_addr, p_in_0 .. p_in_{V-1}, p_out_0 .. p_out_{V-1}, p_time, alimb_*,
      gap_* (V = 2 and ng = 4: 15 of the 16 slots).  Header word 7 = (the READS count) | bits 16, 17, 18 exactly when the blob holds a PAGES
      record, an OPEN record, a LINK that joins | 0x80000 (bit 19, WIDE) exactly when V = 2: a version-10 blob without bit 19 is no ZKA1
      blob, bit 19 with V = 1 is refused.  The builder writes version 10 only then (`derive_pages` on a LINK that carries two values takes
      the wider destination list).

    Version 11: version 10's layout, and the PAGES record may have the two FLAT-ADDRESS destinations.  PAGES word [5] holds F, their
      number: 0 or 2, and 2 only with V = 2; any other value, and F = 2 with V = 1, is refused.  Words [6], [7] hold the data columns
      p_flat_0, p_flat_1 (0 when F = 0); words 8..15 stay reserved.  The 16 destination slots could not take them: V = 2 with ng = 4 uses
      15.  Header word 7 carries bit 20 (0x100000, FLAT) exactly when F = 2: a version-11 blob without bit 20 is no ZKA1 blob, bit 20 with
      no record of F = 2 is refused; bits 16 .. 19 are set exactly when the blob holds what they name.  p_flat_j are destinations like the
      others: one writer, no record reads them, none is a multiplicity (still only p_on); terms may read them.  The builder writes
      version 11 only when a PAGES record has flats (`derive_pages(..., flats=)`).

PORTS (a LINK record with JOINS, ZKA1 version 9): several accesses per row to ONE memory.  A memory is a run of k <= 8 consecutive LINK
records: the head, then the records that join it, in blob order; port q is the record at head + q, and every port has the head's nc, L, nl
and READS-ness.  The memory's accesses are all the (row r < A, port q) whose record's selector is 1 at r, ordered by (r, q); the previous
access of (r, q) with address K = x(key_q, r) is the greatest (r', q') < (r, q) in that order with x(key_q', r') = K.  Everything below keeps
its meaning with "the previous access" read that way: prev_j of (r, q) is the raw word of record q' carried column j at r', the limbs are those
of x(clock_q, r) - x(clock_q', r') - 1, the read rule compares record q's value columns at r with record q' value columns at r'.  Destinations
stay per record: port q writes its own linked, last, prev and limb columns at row r.  A refusal names the port's own record and, where the
previous access lies in another record, says so ("at row R of record Q").  A PAGES record names the head: an unlinked access of any port
takes the image's word, the heads and tails of the page table are those of the merged order, p_addr and p_in come from the head access's
record, p_out and p_time from the tail access's.  A memory of one record is what it always was, message for message.

THE OPEN BUS (the OPEN record; `LogupBuilder(..., open_bus=...)`, zkh_accumulate_open; DESIGN.md §2 "THE TIE"): a bus across seals.  The
challenges are words of `out` (a hash of the data roots of every seal of the group, drawn after all of them are committed:
prover.seal_tied), every term reads them there, and the `last` constraint closes on sum_c S_c = out[total .. total + 4) instead of
zero.  The terms of the open tag are the ones another seal answers: they are no lookups of this seal, so no derived multiplicity and
no sorted copy has that tag, and a bus check (`reference_bus`, zkh_check_bus) skips its keys.  Every other term nets to zero inside
the seal, so the total is the sum of the open tag's terms: `table_fingerprint` of the rows they carry.

THE SPLIT CLOSURE (`LogupBuilder(..., open_bus=..., split_close=True)`; p2_tree_tied.py).  "Every other term nets to zero inside the seal"
is what the prover's accumulate finds, not what the one closing equation sum_c S_c = F constrains: a closed term left over in one seal
only moves that seal's F, and the group check sum F = 0 then balances the closed tuples across the GROUP.  A circuit whose closed bus
must balance per seal (P2-TREE's digest bus: a child produced in one part must not be consumed in another) asks for the split closure:
a column is open when all its terms carry the open tag and closed when none does (a mixed column is refused), and `last` states
sum over closed columns S_c = 0 and sum over open columns S_c = out[total ..].  The challenge is drawn after every data root of the
group is fixed, so the closed bus balances inside the seal with the usual probability and F is the open terms alone.  The blob is the
same version-8 blob: the accumulate, the bus check and the OPEN record do not know how the description closes.

A derived term is the table side of a lookup (`check_derived`): sign -1, its multiplicity a data column that no tuple and no other
term names, and every other term of its tag a lookup of sign +1.  Its multiplicity column is then a function of the traces:
on each table key's representative (the entry of smallest (blob term index, row)) the number of lookups of that key, 0 on the
other active rows (`reference_multiplicities`; DESIGN.md §2 ARGUMENTS).

A sorted copy D of S is the permuted side of a multiset equality (`check_sorted`): sign -1 against S's +1, the same tag, width and
selector, constant multiplicities, and tuple columns that are data columns nothing else in the blob names.  Those columns are then
a function of the traces: S's selected active rows, stably sorted by the canonical values of the key positions, written onto the
same selected rows (`reference_sorted`).

A derived-column record (`check_columns`, zkh_derive_columns) makes data columns a function of other columns, row by row over the
active rows (`reference_columns`).  x = the canonical value of a source cell.  LIMBS: dst_j = (x >> jL) & (2^L - 1); refused when
x >= 2^(L nl).  ORDER over keys (k0) or (k0, k1) that are sorted: row 0 gets zeros; on row r >= 1, e = [k0 = k0@1] (two keys; the flag
column) and d = k0 - k0@1 (one key), or e ? k1 - k1@1 : k0 - k0@1 - 1 (two keys), split into limbs like a LIMBS value; refused when
d < 0 ("not ordered") or d >= 2^(L nl).

A LINK record (`check_links`, zkh_derive_links) gives every memory access the previous access to its own address: the witness of a
memory argument without a sorted copy.  A row r < A is an ACCESS when its selector is 1 (no selector: every active row); a selector
other than 0 / 1 is refused.  With x(c, r) the canonical value of a cell, K = x(key, r) and r' the greatest access below r with the
same K (`reference_links`): linked[r] = [r' exists], last[r] = [no access above r has key K] (Montgomery 0 / 1); prev_j[r] = the raw
word of carried column c_j at r' (0 when r is not linked); limb_j[r] = limb j of d = x(c_0, r) - x(c_0, r') - 1, c_0 being the clock
(0 when not linked), refused when d < 0 ("clock not increasing") or d >= 2^(L nl).  Active rows that are no access get zeros in every
destination.  Selectors are checked, over all records, before any clock.  L nl <= 29 for the reason `order_constraints` gives.

THE READ RULE (a LINK record with READS, ZKA1 version 6): a load returns the last store.  The write flag w is a source of the record,
a code or data column of the host's like the others.  On every access r: w(r) = x(w, r) must be 0 or 1, anything else is refused.  A
store (w = 1) is free.  A load (w = 0) must have, for every carried column j = 1 .. nc - 1 (the clock c_0 is exempt),
x(c_j, r) = x(c_j, r') when r is linked and x(c_j, r) = 0 when it is not: memory starts zeroed.  Values are compared as residues
mod P (a raw word P is a zero).  The rule adds no destination.  On one row the write flag is looked at first, then the clock, then
the read rule, lowest j first; the lowest (record, row) over all of these refusals is the one named.  Records without READS are
what they were.

PAGING (the PAGES record, ZKA1 version 7; `check_pages`, `reference_links(..., image)`, zkh_derive_links_paged): the memory of the paged
LINK record starts from an IMAGE of W raw Montgomery words, image[a] the word of address a = x(key, r); a >= W is refused ("address A
outside the image of W words").  An UNLINKED access r of the paged record takes the image as its previous access: prev_1[r] = the raw
word image[a] (a copy, as prev always is), prev_0[r] = 0 (clock 0 is the image's), the limbs those of d = x(clock, r) - 0 - 1; a clock 0 is
refused ("clock 0 is the image's"), a d that does not fit by the range refusal, and an unlinked load must return image[a] (residues)
where it had to return 0.  linked and last keep their meaning; linked accesses and the other LINK records are what they were.  On one
row the order is write flag, address, clock, read rule.  THE PAGE TABLE: a_0 < .. < a_{D-1} the distinct addresses of the record's
accesses; on the active rows i < D p_on = Montgomery(1), p_addr = the raw key word of a_i's first access, p_in = the raw word
image[a_i], p_out / p_time = the raw value / clock word of a_i's last access, alimb_j = limb j of a_i (refused under the PAGES record's
index when a_i >= 2^(L ng)), gap_j = limb j of a_i - a_{i-1} - 1 (zeros on row 0); active rows [D, A) get zeros in all destinations, rows
[A, n) are never touched; D <= A always fits.  A refusal leaves the data unchanged; the lowest (record, row) over all refusals is named.
PAGE-OUT (`reference_page_out`, zkh_page_out): image[x(p_addr, i)] = p_out[i] on every active row with p_on = 1; refused, with the image
unchanged, on the lowest row whose p_on is not 0 / 1, whose address is >= W or does not follow a smaller one on a row with p_on = 1 (a
table that repeats an address is REFUSED, not resolved: the rows with p_on = 1 are a prefix of strictly increasing addresses).
THE IMAGE'S COMMITMENT (`reference_image_tree`, `reference_image_root`; zkh_image_commit, zkh_page_out_tree): a Merkle tree over the
image's RESIDUES (image[a] and image[a] + P are one memory and give one root).  L = the smallest power of two >= ceil(W / 8); 2 L digests
in heap order, digest 0 eight zeros; leaf L + j, word k = image[8 j + k] % P for 8 j + k < W, else 0: eight memory words verbatim, not a
hash; node i (1 <= i < L) = hash_pair(node 2 i, node 2 i + 1), the operation P2-JOIN constrains; the root is digest 1.
zkh_page_out_tree is the page-out followed by the update of the nodes on the paged words' paths: afterwards the nodes are those of a
fresh commit of the new image.
THE UPDATE'S PROOF, ZKU1 (`reference_page_out_proof`, `check_page_out_proof`; zkh_page_out_proof, zkh_image_proof_verify; the format in
full: include/zkhal.h): the page table's (address, in, out) rows, the old leaves they touch and the clean sibling digests of every layer,
from which root_before and root_after both follow by one hash_pair per dirty node: who holds root_before and the proof reaches
root_after without the image.
THE WALK has two homes with one verdict: zkh_image_proof_verify on the host (`check_page_out_proof` is its numpy twin) and
zkh_image_proof_walk on the device, from the buffer zkh_page_out_proof wrote and the proof's own length (HipHal.image_proof_walk;
SegmentProver.page_out(..., proof=True, walk=True) checks the proof it returns against the tree's root after the page-out).  For every
(proof, root_before) both succeed with the same root_after or fail with the same message after their prefixes; the host verifier's
order of causes decides when several apply, and this module's `check_page_out_proof` states that order.
THE DIRTY-NODE TABLE, ZKN1 (`reference_page_out_nodes`, `image_dirty_words`; zkh_image_proof_nodes, zkh_image_dirty_words; csrc/zkn1.h):
the walk keeping what it recomputes: per layer the heap ids of the dirty nodes and, per node, its two children old and new, which is
what a P2-TREE block of any part reads (zkh_page_tree_witgen_nodes), so a part is sealed from (proof, root_before) without the trees.
WIDE (the PAGES record with V = 2, ZKA1 version 10): BabyBear is a 31-bit field, so a 32-bit machine word is two field elements, and the
paged memory holds V value words per address, V the paged LINK's nc - 1 (1 or 2).  Everything above is V = 1; with V = 2, stated once:
  * THE IMAGE is V W raw Montgomery words, FLAT: word j of address a is image[V a + j].  An image whose length is no multiple of V is
    refused before anything else ("an image of N words is not a whole number of addresses of V value words"); a >= W is refused with
    the text above, W counted in addresses.
  * An unlinked access of the paged memory takes prev_{1+j} = image[V a + j] (copies) and prev_0 = 0; an unlinked load must return both
    words, compared as residues, and a refusal names the lowest j first, as the read rule does.
  * THE PAGE TABLE: the head access writes p_in_j = image[V a_i + j], the tail access p_out_j from its own record's value columns.
  * PAGE-OUT sets image[V a_i + j] = p_out_j[i].  The proof's fourth rule: p_in_j is the word the tree's leaf layer holds at V a_i + j
    ("p_in word j X at address A" in its text only when V = 2).
  * THE FLAT TABLE.  To everything behind the page-out (the tree's update, ZKU1, the walk, ZKN1, the page-out circuits) a wide page table
    of D rows is the table of V D rows (V a_i + j, in_j, out_j), i major, j minor: strictly increasing flat addresses over a flat image
    of V W words.  None of that code knows V; image_proof_words is asked about (V W, V D).
  * PAGING FROM A TABLE: `table` is the flat one and image_words the flat image's.  The head of page i reads rows V i .. V i + V - 1 and
    checks each row's address against V a + j; D pages of the trace must meet V D rows.  The three table refusals keep their shape and
    name the flat row.
FLAT (the PAGES record's flats, ZKA1 version 11): the tie puts one row (address, in, out) per word of the flat table on the open bus, and
a wide page row holds two of them, so the trace carries their addresses.  Stated once:
  * For page i < D with address a_i: p_flat_j[i] = the canonical Montgomery encoding of the integer 2 a_i + j, j = 0, 1.  p_addr stays the
    raw key word and may be >= P; the flat columns come from the decoded address and never are.  Rows D <= i < A hold 0, like the rest
    of the table.  In image and in table mode, with and without ports; the check passes and every refusal are what they were.
  * THE CONSTRAINT (`page_constraints`): p_on (p_flat_j - 2 p_addr - j) = 0.  The address limbs bound p_addr below 2^29, so
    2 p_addr + 1 < 2^30 < P and the field equation names one integer; page addresses increase strictly, so the flat addresses are distinct.
    A row with p_on = 0 is not constrained and need not be: every term that reads p_flat_j has the multiplicity p_on.
  * THE TIE: the terms +p_on (p_flat_j, p_in_j, p_out_j) under TIE_TAG are the rows of the flat table, so the open total of a wide
    segment is `table_fingerprint` of its flat table, and nothing behind the page-out knows V.
Left out: one paged memory per blob; the tie of a wide memory WITHOUT flats is refused.  The circuits that check p_in /
p_out against those roots are the page-out circuits (p2_page.py and after it), and THE OPEN BUS below ties their rows to this table.

WHO WRITES A DATA COLUMN (`_check_owned` behind `check_columns` and `check_links`; csrc/arguments.h says the same).  A data column
has at most one writer, and a derive reads only what the stages before it have finished writing.  The writers: a sorted copy (its
tuple columns), a LIMBS / ORDER record and a LINK record (their destinations), a derived multiplicity (its column); every other
column is the host's.  The library runs one stage after the other, each over the whole trace: sorted -> columns -> links ->
multiplicities.  Of the columns a derive writes, the sort reads none (`check_sorted`, and no record writes into a source term's
tuple); a LIMBS / ORDER record reads a sorted copy's columns and no record's destination (records never chain); a LINK reads none;
the multiplicities count lookup tuples, and those read every derived column freely: a lookup may count a limb.  Nothing reads a derived
multiplicity (`check_derived`).  A term's multiplicity is the host's column or a derived one, with one exception: `linked` and
`last` of a LINK record (only they) may be the multiplicity of a term that is not derived: -linked (addr, prev) removes the old tuple
from the bus and -last (addr, val, clock) pages the final one out.  The PAGES record is one more writer of the links stage: it reads what
its LINK reads, and of its destinations p_on (only it) may be such a multiplicity.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .desc import GLOBAL_MIX, GLOBAL_OUT, GROUP_ACCUM, GROUP_CODE, GROUP_DATA, P, CircuitBuilder, Fp

ARGS_MAGIC = 0x5A4B4131
ARGS_HEADER = 8
TERM_WORDS = 16
NONE = 0xFFFFFFFF
MAX_DEGREE = 5
MAX_TUPLE = 4
NBETA = P - 11


@dataclass(frozen=True)
class Term:
    col: int                                   # accum Fp4 column
    tuple_cols: Tuple[Tuple[int, int], ...]    # (group, column) of v_0 .. v_{w-1}
    sign: int = 1
    sel: Optional[int] = None                  # code column, or None = 1
    mult: Optional[Tuple[int, int]] = None     # (group, column), or None = 1
    tag: int = 0
    derive: bool = False                       # the multiplicity is derived by the library (ZKA1 version 2)
    sorted_from: Optional[int] = None          # this term is the sorted copy of that term (its index in the same list; version 3)
    sort_keys: Tuple[int, ...] = ()            # tuple positions of the sort keys, most significant first

    def flags(self) -> int:
        """word 7 of the term's record"""
        f = int(self.derive)
        if self.sorted_from is not None:
            f |= 2 | len(self.sort_keys) << 4 | self.sorted_from << 16
            for j, pos in enumerate(self.sort_keys):
                f |= pos << (8 + 2 * j)
        return f

    def degree(self, n_terms: int) -> int:
        """degree of the numerator summand sign * sel * m * prod_{l != i} d_l"""
        return (self.sel is not None) + (self.mult is not None) + n_terms - 1


def check_derived(terms: Sequence[Term]) -> Optional[str]:
    """the first derived term that breaks a rule, named by its index in `terms`, or None: (a) sign -1, (b) a data-group multiplicity,
    (c) that column named by no tuple and no other term's multiplicity, (d) every other term of its tag of sign +1 or derived"""
    for i, t in enumerate(terms):
        if not t.derive:
            continue
        if t.sign != -1:
            return f"term {i}: a derived multiplicity needs sign -1 (the table side of a lookup)"
        if t.mult is None or t.mult[0] != GROUP_DATA:
            return f"term {i}: a derived multiplicity must be a data-group column"
        for j, u in enumerate(terms):
            if j != i and u.mult == t.mult:
                return f"term {i}: its derived multiplicity column (data {t.mult[1]}) is also the multiplicity of term {j}"
            if t.mult in u.tuple_cols:
                return f"term {i}: its derived multiplicity column (data {t.mult[1]}) is read by the tuple of term {j}"
            if u.tag % P == t.tag % P and not u.derive and u.sign != 1:
                return f"term {i}: term {j} of its tag {t.tag % P} has sign -1 and is not derived (the lookups of a derived tag have sign +1)"
    return None


MAX_SORT_KEYS = 3


def check_sorted(terms: Sequence[Term]) -> Optional[str]:
    """the first sorted-copy term D that breaks a rule, named by its index in `terms`, or None.  With S its source: (a) D has sign -1
    and no derived multiplicity, S is another term of sign +1 without a flag and the source of no other copy; (b) the same tag, tuple
    width and selector, both multiplicities the constant 1; (c) D's tuple columns are pairwise distinct data columns that no other
    tuple and no multiplicity names; (d) 1..3 key positions, distinct and below the width; (e) no derived multiplicity in D's tag"""
    for i, t in enumerate(terms):
        if t.sorted_from is None:
            continue
        s, w = t.sorted_from, len(t.tuple_cols)
        if t.sign != -1:
            return f"term {i}: a sorted copy needs sign -1 (the permuted side of a multiset equality)"
        if t.derive:
            return f"term {i}: a sorted copy cannot also have a derived multiplicity"
        if s == i or not 0 <= s < len(terms):
            return f"term {i}: its source term {s} is not another term of the arguments"
        u = terms[s]
        if u.sign != 1:
            return f"term {i}: its source term {s} needs sign +1"
        if u.derive or u.sorted_from is not None:
            return f"term {i}: its source term {s} is itself derived or a sorted copy"
        for j, x in enumerate(terms):
            if j != i and x.sorted_from == s:
                return f"term {i}: its source term {s} is also the source of term {j}"
        if u.tag % P != t.tag % P or len(u.tuple_cols) != w or u.sel != t.sel:
            return f"term {i}: its source term {s} has another tag, tuple width or selector"
        if t.mult is not None or u.mult is not None:
            return f"term {i}: a sorted copy and its source term {s} have the constant multiplicity 1"
        for e, (g, c) in enumerate(t.tuple_cols):
            if g != GROUP_DATA:
                return f"term {i}: tuple column ({g}, {c}) of a sorted copy must be a data-group column"
            if (g, c) in t.tuple_cols[:e]:
                return f"term {i}: its sorted column (data {c}) appears twice in its tuple"
            for j, x in enumerate(terms):
                if j != i and (g, c) in x.tuple_cols:
                    return f"term {i}: its sorted column (data {c}) is read by the tuple of term {j}"
                if x.mult == (g, c):
                    return f"term {i}: its sorted column (data {c}) is the multiplicity of term {j}"
        k = t.sort_keys
        if not 1 <= len(k) <= min(w, MAX_SORT_KEYS):
            return f"term {i}: {len(k)} sort keys (1..{min(w, MAX_SORT_KEYS)}: at most {MAX_SORT_KEYS}, and no more than the tuple width {w})"
        if len(set(k)) != len(k) or any(not 0 <= pos < w for pos in k):
            return f"term {i}: its sort key positions must be distinct and below the tuple width {w}"
        for j, x in enumerate(terms):
            if x.derive and x.tag % P == t.tag % P:
                return f"term {i}: term {j} of its tag {t.tag % P} has a derived multiplicity"
    return None


KIND_LIMBS, KIND_ORDER = 1, 2
RECORD_WORDS = 16
MAX_LIMBS = 8
MAX_ORDER_BITS = 29                            # order_constraints: keys and differences below 2^29 keep a negative difference out of range


@dataclass(frozen=True)
class Record:
    """A derived-column record as the blob holds it (ZKA1 version 4): the fields are the blob's words, `check_columns` the rules"""
    kind: int                                  # KIND_LIMBS / KIND_ORDER
    limb_bits: int                             # L
    nl: int                                    # limb count
    srcs: Tuple[Tuple[int, int], ...]          # n_src (group, column) pairs
    dsts: Tuple[int, ...]                      # data columns: (ORDER with two keys: the flag,) then the nl limbs
    reserved: bool = False                     # a word the format reserves was not 0 (parser only)
    n_src_word: Optional[int] = None           # the blob's n_src where it is not len(srcs) (parser only: an n_src out of range)

    @property
    def n_src(self) -> int:
        return len(self.srcs) if self.n_src_word is None else self.n_src_word

    def n_dsts(self) -> int:
        return self.nl + (self.kind == KIND_ORDER and len(self.srcs) == 2)

    def words(self) -> List[int]:
        w = [self.kind, self.limb_bits, self.nl, len(self.srcs)]
        for g, c in self.srcs:
            w += [g, c]
        w += [0] * (8 - len(w))
        w += list(self.dsts)
        return w + [0] * (RECORD_WORDS - len(w))


def _columns_clause_a(i: int, r: Record, group_sizes) -> Optional[str]:
    if r.kind not in (KIND_LIMBS, KIND_ORDER):
        return f"record {i}: kind {r.kind} (1 = LIMBS, 2 = ORDER)"
    if not (1 <= r.limb_bits <= 16 and 1 <= r.nl <= MAX_LIMBS and r.limb_bits * r.nl <= 32):
        return f"record {i}: {r.nl} limbs of {r.limb_bits} bits (1..8 limbs of 1..16 bits, at most 32 bits in all)"
    if not 1 <= r.n_src <= (1 if r.kind == KIND_LIMBS else 2):
        return f"record {i}: {r.n_src} sources (LIMBS: 1; ORDER: 1 or 2)"
    if len(r.srcs) == 2 and r.nl > MAX_LIMBS - 1:
        return f"record {i}: an ORDER record with two keys has at most {MAX_LIMBS - 1} limbs (its flag column is the first destination)"
    if r.reserved or len(r.dsts) != r.n_dsts():
        return f"record {i}: a reserved word is not 0 (the unused source pair and the unused destination words)"
    return None


def check_columns(terms: Sequence[Term], records: Sequence[Record], group_sizes=None) -> Optional[str]:
    """the first LIMBS / ORDER record that breaks a rule, named by its index in `records` (they are one another's only peers), or None:
    (a) the ranges of kind, L, nl, n_src and the reserved words, then (b) .. (e) of `_check_owned`"""
    return _check_owned(terms, records, None, _columns_clause_a, group_sizes)


KIND_LINK = 3
LINK_WORDS = 32
MAX_CARRIED = 3
MAX_LINK_LIMBS = 4
LINK_JOINS = 2                                 # LINK word 5, bit 1 (version 9): the record joins the memory of the head that word 31 names
MAX_PORTS = 8                                  # the records of one memory, the head included
PORTS_BIT = 0x40000                            # header word 7, bit 18 (version 9): a LINK record joins


@dataclass(frozen=True)
class Link:
    """A LINK record as the blob holds it (ZKA1 version 5): the fields are the blob's words, `check_links` the rules"""
    sel: Optional[int]                         # selector code column, or None = 1
    key: Tuple[int, int]                       # (group, column) of the address
    carried: Tuple[Tuple[int, int], ...]       # nc (group, column) pairs, c_0 the clock
    limb_bits: int                             # L
    nl: int                                    # limb count
    dsts: Tuple[int, ...]                      # data columns: linked, last, prev_0 .. prev_{nc-1}, limb_0 .. limb_{nl-1}
    reserved: bool = False                     # a word the format reserves was not 0 (parser only)
    nc_word: Optional[int] = None              # the blob's nc where it is not len(carried) (parser only: an nc out of range)
    write: Optional[Tuple[int, int]] = None    # READS (version 6): the (group, column) of the write flag; None = no read rule
    flag_word: Optional[int] = None            # the blob's word 5 where it sets a bit other than READS (parser only)
    stray_write: bool = False                  # words 14, 15 are not 0 although READS is not set (parser only, version 6)
    joins: Optional[int] = None                # JOINS (version 9): the blob record index of the head whose memory this record is a port of
    ports_word: bool = field(default=False, compare=False)   # the blob's version reads bit 1 of word 5 as JOINS (parser only: the text of the flag word's refusal)
    kind = KIND_LINK

    @property
    def nc(self) -> int:
        return len(self.carried) if self.nc_word is None else self.nc_word

    @property
    def srcs(self) -> Tuple[Tuple[int, int], ...]:
        return (self.key,) + self.carried + (() if self.write is None else (self.write,))

    @property
    def linked(self) -> int:
        return self.dsts[0]

    @property
    def last(self) -> int:
        return self.dsts[1]

    @property
    def prevs(self) -> Tuple[int, ...]:
        return self.dsts[2: 2 + len(self.carried)]

    @property
    def limbs(self) -> Tuple[int, ...]:
        return self.dsts[2 + len(self.carried):]

    def n_dsts(self) -> int:
        return 2 + len(self.carried) + self.nl

    def words(self) -> List[int]:
        w = [KIND_LINK, self.limb_bits, self.nl, len(self.carried), NONE if self.sel is None else self.sel,
             int(self.write is not None) | (LINK_JOINS if self.joins is not None else 0), self.key[0], self.key[1]]
        for g, c in self.carried:
            w += [g, c]
        w += [0] * (14 - len(w)) + list(self.write or (0, 0))
        w += list(self.dsts)
        w += [0] * (LINK_WORDS - len(w))
        if self.joins is not None:
            w[LINK_WORDS - 1] = self.joins
        return w


def _links_clause_a(i: int, r: Link, group_sizes) -> Optional[str]:
    if not (1 <= r.nc <= MAX_CARRIED and 1 <= r.limb_bits <= 16 and 0 <= r.nl <= MAX_LINK_LIMBS and r.limb_bits * r.nl <= MAX_ORDER_BITS):
        return (f"record {i}: a LINK of {r.nc} carried columns and {r.nl} limbs of {r.limb_bits} bits (1..{MAX_CARRIED} carried columns, "
                f"0..{MAX_LINK_LIMBS} limbs of 1..16 bits, at most {MAX_ORDER_BITS} bits in all)")
    if r.flag_word is not None and r.ports_word:
        return f"record {i}: word 5 of a LINK is {r.flag_word:#x} (bit 0: READS, the read rule; bit 1: JOINS, a port of its head's memory; the other bits are reserved)"
    if r.flag_word is not None:
        return f"record {i}: word 5 of a LINK is {r.flag_word:#x} (bit 0: READS, the read rule; the other bits are reserved)"
    if r.stray_write:
        return f"record {i}: words 14, 15 of a LINK name a write flag, but bit 0 of word 5 (READS) is not set"
    if r.write is not None and r.nc < 2:
        return f"record {i}: READS needs a clock and a value column (2..{MAX_CARRIED} carried columns), this LINK carries {r.nc}"
    if r.reserved or len(r.dsts) != r.n_dsts():
        return f"record {i}: a reserved word of a LINK is not 0 (words 5, 14, 15, the unused carried pairs and the unused destination words)"
    if r.sel is not None and (r.sel >= NONE or (group_sizes is not None and not 0 <= r.sel < group_sizes[GROUP_CODE])):
        return f"record {i}: selector {r.sel} is not a code column"
    return None


def _joins_rule(i: int, r: Link, records: Sequence) -> Optional[str]:
    """the rules of a joiner (version 9): its head is a LINK record without JOINS before it, every record between them joins the same
    head, it has the head's nc, L, nl and READS-ness, and it is one of the head's first MAX_PORTS - 1 joiners"""
    h = r.joins
    if h is None:
        return None
    head = records[h] if 0 <= h < i else None
    if not isinstance(head, Link) or head.joins is not None:
        return f"record {i}: a LINK joins record {h}, which is no LINK record without JOINS before it (a port joins the head of its memory)"
    for j in range(h + 1, i):
        if not isinstance(records[j], Link) or records[j].joins != h:
            return f"record {i}: a LINK joins record {h}, but record {j} between them does not (a memory is a run of consecutive LINK records)"
    if (r.nc, r.limb_bits, r.nl, r.write is None) != (head.nc, head.limb_bits, head.nl, head.write is None):
        return f"record {i}: a LINK joins record {h} with another nc, L, nl or READS (the ports of a memory have their head's)"
    if i - h >= MAX_PORTS:
        return f"record {i}: port {i - h} of the memory of record {h} (a memory has at most {MAX_PORTS} records)"
    return None


def memory_ports(records: Sequence, head: int) -> List[int]:
    """the blob record indices of the ports of the memory whose head is the LINK record `head`: the head, then its joiners"""
    ports = [head]
    while ports[-1] + 1 < len(records) and isinstance(records[ports[-1] + 1], Link) and records[ports[-1] + 1].joins == head:
        ports.append(ports[-1] + 1)
    return ports


def check_links(terms: Sequence[Term], records: Sequence, group_sizes=None) -> Optional[str]:
    """the first LINK record that breaks a rule, named by its index among all `records` (all of them are its peers), or None: (a) the
    ranges of nc, L, nl, the flag word and the write flag's words (version 6), the reserved words and the selector a code column, then
    (version 9) a joiner's rules: its head a LINK without JOINS before it, the records between them joiners of the same head, the head's
    nc, L, nl and READS-ness, at most MAX_PORTS records in the memory; then (b) .. (e) of `_check_owned`; the write flag of a READS
    record is one of its sources.  A port is a LINK like any other: one writer per column, and it reads no derived column"""
    return _check_owned(terms, records, Link, lambda i, r, sizes: _links_clause_a(i, r, sizes) or _joins_rule(i, r, records), group_sizes)


KIND_PAGES = 4
PAGES_WORDS = 32
MAX_PAGE_LIMBS = 4
MAX_PAGE_WORDS = 2                             # V, the value words per address of a paged memory (version 10: 1 or 2)
PAGES_BIT = 0x10000                            # header word 7, bit 16 (version 7): the blob has a PAGES record
WIDE_BIT = 0x80000                             # header word 7, bit 19 (version 10): the PAGES record pages two value words per address
FLAT_BIT = 0x100000                            # header word 7, bit 20 (version 11): the PAGES record has the two flat-address destinations


@dataclass(frozen=True)
class Pages:
    """A PAGES record as the blob holds it (ZKA1 version 7; version 10: `nv`; version 11: `flats`): the fields are the blob's words,
    `check_pages` the rules"""
    limb_bits: int                             # L
    ng: int                                    # limbs of a page address and of a gap
    link: int                                  # the blob record index of the LINK record it pages
    dsts: Tuple[int, ...]                      # data columns: p_on, p_addr, p_in_0 .., p_out_0 .., p_time, alimb_0 .. alimb_{ng-1}, gap_0 .. gap_{ng-1}
    reserved: bool = False                     # a word the format reserves was not 0 (parser only)
    nv: int = 1                                # V, the value words per address (version 10: word 4 holds V - 1); the paged LINK's nc - 1
    nv_word: Optional[int] = None              # the blob's word 4 where it is above 1 (parser only, version 10)
    wide_word: bool = field(default=False, compare=False)    # the blob's version reads word 4 as V - 1 (parser only: the text of the reserved words' refusal)
    flats: Tuple[int, ...] = ()                # the flat-address destinations p_flat_0, p_flat_1 (version 11: word 5 holds F = 0 or 2, words 6, 7 the columns)
    nf_word: Optional[int] = None              # the blob's word 5 where it is neither 0 nor 2 (parser only, version 11)
    flat_word: bool = field(default=False, compare=False)    # the blob's version reads word 5 as F (parser only: the text of the reserved words' refusal)
    kind = KIND_PAGES

    p_on = property(lambda self: self.dsts[0])
    p_addr = property(lambda self: self.dsts[1])
    p_in = property(lambda self: self.dsts[2])
    p_ins = property(lambda self: self.dsts[2: 2 + self.nv])
    p_out = property(lambda self: self.dsts[2 + self.nv])
    p_outs = property(lambda self: self.dsts[2 + self.nv: 2 + 2 * self.nv])
    p_time = property(lambda self: self.dsts[2 + 2 * self.nv])
    alimbs = property(lambda self: self.dsts[3 + 2 * self.nv: 3 + 2 * self.nv + self.ng])
    gaps = property(lambda self: self.dsts[3 + 2 * self.nv + self.ng:])

    def n_dsts(self) -> int:
        return 3 + 2 * self.nv + 2 * self.ng

    def words(self) -> List[int]:
        w = [KIND_PAGES, self.limb_bits, self.ng, self.link, self.nv - 1, len(self.flats)] + list(self.flats) + [0] * (10 - len(self.flats)) + list(self.dsts)
        return w + [0] * (PAGES_WORDS - len(w))


def _paged_link(records: Sequence, r: "Pages") -> Optional[Link]:
    """the LINK record that the PAGES record `r` names, where it is one the rules allow: READS, a clock and V = r.nv value columns"""
    t = records[r.link] if 0 <= r.link < len(records) else None
    return t if isinstance(t, Link) and t.write is not None and t.nc == 1 + r.nv and len(t.carried) == 1 + r.nv else None


def check_pages(terms: Sequence[Term], records: Sequence, group_sizes=None) -> Optional[str]:
    """the PAGES record that breaks a rule, named by its index among all `records` (all of them are its peers), or None: (a) the ranges
    of L and ng, the reserved words, word 4 (version 10: V - 1, 0 or 1), word 5 (version 11: F, 0 or 2, and 2 only with V = 2), and its target a LINK record with READS and nc = 1 + V that joins
    no other (version 9: the head of its memory, whose ports then have READS and the same nc as well); then (b) .. (e) of `_check_owned`,
    its sources being its LINK's and p_on the one destination that may be a multiplicity (p_flat_j are destinations like the others)"""
    def clause_a(i, r, _sizes):
        if not (1 <= r.limb_bits <= 16 and 1 <= r.ng <= MAX_PAGE_LIMBS and r.limb_bits * r.ng <= MAX_ORDER_BITS):
            return (f"record {i}: a PAGES record of {r.ng} limbs of {r.limb_bits} bits (1..{MAX_PAGE_LIMBS} limbs of 1..16 bits, at most "
                    f"{MAX_ORDER_BITS} bits in all)")
        if r.nv_word is not None:
            return f"record {i}: word 4 of a PAGES record is {r.nv_word} (V - 1: 0 = one value word per address, 1 = two)"
        if r.nf_word is not None:
            return f"record {i}: word 5 of a PAGES record is {r.nf_word} (F, the flat-address destinations: 0 or 2)"
        if r.flats and r.nv == 1:
            return f"record {i}: a PAGES record of one value word per address has {len(r.flats)} flat-address destinations (they are the flat addresses of two value words)"
        if (r.reserved or len(r.dsts) != r.n_dsts()) and (r.flat_word or r.flats):
            return f"record {i}: a reserved word of a PAGES record is not 0 (words 8..15, words 6 and 7 without flat-address destinations, and the unused destination words)"
        if r.reserved or len(r.dsts) != r.n_dsts():
            return (f"record {i}: a reserved word of a PAGES record is not 0 (words 5..15 and the unused destination words)" if r.wide_word or r.nv > 1 else
                    f"record {i}: a reserved word of a PAGES record is not 0 (words 4..15 and the unused destination words)")
        if _paged_link(records, r) is None and r.nv > 1:
            return (f"record {i}: a PAGES record of two value words per address pages record {r.link}, which is no LINK record with READS and three carried "
                    f"columns (a clock and two values)")
        if _paged_link(records, r) is None:
            return f"record {i}: a PAGES record pages record {r.link}, which is no LINK record with READS and two carried columns (a clock and one value)"
        if _paged_link(records, r).joins is not None:
            return f"record {i}: a PAGES record pages record {r.link}, which joins record {_paged_link(records, r).joins} (a PAGES record names the head of a memory)"
        return None
    return _check_owned(terms, records, Pages, clause_a, group_sizes)


KIND_OPEN = 5
OPEN_WORDS = 16
OPEN_BIT = 0x20000                             # header word 7, bit 17 (version 8): the blob has an OPEN record


@dataclass(frozen=True)
class Open:
    """The OPEN record as the blob holds it (ZKA1 version 8): the fields are the blob's words, `check_open` the rules"""
    tag: int                                   # the terms of this tag are answered by another seal
    alpha: int                                 # `out` word offsets: the two challenges and the bus total, 4 words each
    beta: int
    total: int
    out_words: int                             # the circuit's `out` words
    reserved: bool = False                     # a word the format reserves was not 0 (parser only)
    kind = KIND_OPEN

    def words(self) -> List[int]:
        w = [KIND_OPEN, self.tag % P, self.alpha, self.beta, self.total, self.out_words]
        return w + [0] * (OPEN_WORDS - len(w))


def check_open(terms: Sequence[Term], records: Sequence, header=None) -> Optional[str]:
    """the OPEN record that breaks a rule, named by its index among all `records`, or None: it is the last record and the only one of
    its kind; its reserved words are 0; its tag is below P, some term carries it, and none of them is derived or a sorted copy; alpha,
    beta and the total are three disjoint runs of 4 words inside `out`.  header = the blob's (alpha, beta) words, which repeat them."""
    at = [i for i, r in enumerate(records) if isinstance(r, Open)]
    if not at:
        return None
    i, r = at[0], records[at[0]]
    if len(at) > 1:
        return f"record {at[1]}: a second OPEN record (record {i} is one: a seal closes on one total)"
    if i != len(records) - 1:
        return f"record {i + 1}: a record after the OPEN record {i} (the OPEN record comes last)"
    if r.reserved:
        return f"record {i}: a reserved word of the OPEN record is not 0 (words 6..15)"
    if r.tag >= P:
        return f"record {i}: the open tag {r.tag} is not below P"
    for name, off in (("alpha", r.alpha), ("beta", r.beta), ("the total", r.total)):
        if off + 4 > r.out_words:
            return f"record {i}: {name} at out words {off}..{off + 3}, the circuit has {r.out_words}"
    runs = sorted((r.alpha, r.beta, r.total))
    if runs[0] + 4 > runs[1] or runs[1] + 4 > runs[2]:
        return f"record {i}: alpha, beta and the total overlap in out (words {r.alpha}, {r.beta}, {r.total}: 4 words each)"
    if header is not None and tuple(header) != (r.alpha, r.beta):
        return f"record {i}: header words 3, 4 are {header[0]}, {header[1]}, the OPEN record's alpha, beta are {r.alpha}, {r.beta}"
    mine = [j for j, t in enumerate(terms) if t.tag % P == r.tag]
    if not mine:
        return f"record {i}: no term has the open tag {r.tag}"
    for j in mine:
        if terms[j].derive or terms[j].sorted_from is not None:
            return f"record {i}: term {j} of the open tag {r.tag} is derived or a sorted copy (another seal answers the open tag)"
    return None


class _Owned(NamedTuple):
    """A record of either kind as the ownership rule sees it"""
    index: int                                 # its index among the records
    srcs: Tuple[Tuple[int, int], ...]          # the (group, column) pairs it reads: the data-group ones have a writer or none
    dsts: Tuple[int, ...]                      # the data columns it writes
    link: bool                                 # a LINK or the PAGES record: it runs after every LIMBS / ORDER record
    free: int = 0                              # its first `free` destinations may be the multiplicity of a term that is not derived


def _check_owned(terms: Sequence[Term], records: Sequence, of, clause_a, group_sizes=None) -> Optional[str]:
    """The ownership rule (the module docstring) over the records of `records` of the class `of` (Link, Pages; None: all of them): the
    first that breaks a clause, or None.  Per record, in this order: `clause_a`, the kind's own ranges; (b) its sources are code or data columns
    (of the circuit, when `group_sizes` = (accum, code, data) is given), its destinations pairwise distinct data columns.  Then, per
    record again: (c) no source is a destination of any record (records never chain) or a derived multiplicity, and a LINK's is no
    sorted copy's column either; (d) no destination is written twice: by another record, a sorted copy or a derived multiplicity;
    (e) no destination is read by the source term of a sorted copy (the sort runs first) or, a LINK's, by any record, and none is a
    term's multiplicity, a LINK's `linked` and `last` and a PAGES record's `p_on` apart.  A PAGES record reads what its LINK reads.
    Lookup tuples read destinations freely."""
    def view(i, r):
        if isinstance(r, Pages):
            t = _paged_link(records, r)
            return _Owned(i, () if t is None else tuple(t.srcs), tuple(r.dsts) + tuple(r.flats), True, 1)
        return _Owned(i, tuple(r.srcs), tuple(r.dsts), isinstance(r, Link), 2 if isinstance(r, Link) else 0)
    peers = [view(i, r) for i, r in enumerate(records)]
    mine = peers if of is None else [v for v in peers if isinstance(records[v.index], of)]
    for i, srcs, dsts, _, _ in mine:
        problem = clause_a(i, records[i], group_sizes)
        if problem:
            return problem
        for g, c in srcs:
            if g not in (GROUP_CODE, GROUP_DATA) or (group_sizes is not None and not 0 <= c < group_sizes[g]):
                return f"record {i}: source ({g}, {c}) is not a code or data column"
        for e, c in enumerate(dsts):
            if group_sizes is not None and not 0 <= c < group_sizes[GROUP_DATA]:
                return f"record {i}: destination {c} is not a data column"
            if c in dsts[:e]:
                return f"record {i}: its destination (data {c}) appears twice"
    for i, srcs, dsts, link, free in mine:
        for g, c in srcs:
            if g != GROUP_DATA:
                continue
            for j, t in enumerate(terms):
                if link and t.sorted_from is not None and (g, c) in t.tuple_cols:
                    return f"record {i}: its source (data {c}) is written by the sorted copy term {j} (a LINK reads what no derive writes)"
            for x in peers:
                if c in x.dsts:
                    return f"record {i}: its source (data {c}) is a destination of record {x.index} (records never chain)"
            for j, t in enumerate(terms):
                if t.derive and t.mult == (g, c):
                    return f"record {i}: its source (data {c}) is the derived multiplicity of term {j}"
        for e, c in enumerate(dsts):
            for x in peers:
                if x.index != i and c in x.dsts:
                    return f"record {i}: its destination (data {c}) is also written by record {x.index}"
            for j, t in enumerate(terms):
                if t.sorted_from is not None and (GROUP_DATA, c) in t.tuple_cols:
                    return f"record {i}: its destination (data {c}) is written by the sorted copy term {j}"
                if t.derive and t.mult == (GROUP_DATA, c):
                    return f"record {i}: its destination (data {c}) is the derived multiplicity of term {j}"
            for x in peers:
                if link and (GROUP_DATA, c) in x.srcs:
                    return f"record {i}: its destination (data {c}) is read by record {x.index} (the links run after the columns, and never chain)"
            for t in terms:
                if t.sorted_from is not None and 0 <= t.sorted_from < len(terms) and (GROUP_DATA, c) in terms[t.sorted_from].tuple_cols:
                    return f"record {i}: its destination (data {c}) is read by term {t.sorted_from}, the source of a sorted copy (the sort runs first)"
            for j, t in enumerate(terms):
                if t.mult == (GROUP_DATA, c) and e >= free:
                    return (f"record {i}: its destination (data {c}) is the multiplicity of term {j}"
                            + ((" (of a LINK's destinations only linked and last may be)" if free == 2 else
                                " (of a PAGES record's destinations only p_on may be)") if link else ""))
    return None


def _check_records(terms: Sequence[Term], records: Sequence, group_sizes=None) -> Optional[str]:
    """check_columns over the LIMBS / ORDER records (they come first, so the indices are the blob's), then check_links, then (version 7)
    check_pages over the one PAGES record, which comes last; the OPEN record (version 8) comes after all of them (`check_open`)"""
    problem = check_open(terms, records)
    if problem:
        return problem
    records = [r for r in records if not isinstance(r, Open)]
    pages = [i for i, r in enumerate(records) if isinstance(r, Pages)]
    if pages and pages[0] != len(records) - 1:
        j = pages[0] + 1
        if isinstance(records[j], Pages):
            return f"record {j}: a second PAGES record (record {pages[0]} is one: a blob pages one memory)"
        return f"record {j}: a record after the PAGES record {pages[0]} (the PAGES record comes last)"
    n_cols = sum(isinstance(r, Record) for r in records)
    for i, r in enumerate(records[:n_cols]):
        if isinstance(r, Link):
            j = next(j for j in range(i, len(records)) if isinstance(records[j], Record))
            return f"record {j}: a LIMBS / ORDER record after the LINK record {i} (LINK records come last)"
    return check_columns(terms, records[:n_cols], group_sizes) or check_links(terms, records, group_sizes) or check_pages(terms, records, group_sizes)


def _by_column(terms: Sequence[Term]) -> List[Term]:
    """the terms sorted by accum column (stable: the blob order), the source indices of sorted copies following their terms"""
    order = sorted(range(len(terms)), key=lambda i: terms[i].col)
    if order == list(range(len(terms))):
        return list(terms)
    new = {old: pos for pos, old in enumerate(order)}
    return [terms[i] if terms[i].sorted_from is None else replace(terms[i], sorted_from=new.get(terms[i].sorted_from, terms[i].sorted_from))
            for i in order]


def column_degree(terms: Sequence[Term]) -> int:
    """degree of the first / body constraint of a column with these terms (the gate included)"""
    t = len(terms)
    return 1 + max([1 + t] + [x.degree(t) for x in terms])


@dataclass
class Arguments:
    """Parsed view of a ZKA1 blob."""
    k: int
    alpha: int
    beta: int
    terms: List[Term]
    records: List[Record] = field(default_factory=list)

    @property
    def reads(self) -> int:
        """the LINK records with READS (header word 7 of version 6)"""
        return sum(isinstance(r, Link) and r.write is not None for r in self.records)

    @property
    def pages(self) -> Optional["Pages"]:
        """the PAGES record (version 7: bit 16 of header word 7), or None"""
        return next((r for r in self.records if isinstance(r, Pages)), None)

    @property
    def open(self) -> Optional["Open"]:
        """the OPEN record (version 8), or None: the bus closes on zero and the challenges are mix words"""
        return next((r for r in self.records if isinstance(r, Open)), None)

    @property
    def ports(self) -> bool:
        """a LINK record joins another's memory (version 9: bit 18 of header word 7)"""
        return any(isinstance(r, Link) and r.joins is not None for r in self.records)

    @property
    def wide(self) -> bool:
        """the PAGES record pages two value words per address (version 10: bit 19 of header word 7)"""
        return self.pages is not None and self.pages.nv > 1

    @property
    def flat(self) -> bool:
        """the PAGES record has the flat-address destinations (version 11: bit 20 of header word 7)"""
        return self.pages is not None and len(self.pages.flats) > 0

    @property
    def version(self) -> int:
        if self.flat:
            return 11
        if self.wide:
            return 10
        if self.ports:
            return 9
        if self.open is not None:
            return 8
        if self.pages is not None:
            return 7
        if self.reads:
            return 6
        if any(isinstance(r, Link) for r in self.records):
            return 5
        if self.records:
            return 4
        if any(t.sorted_from is not None for t in self.terms):
            return 3
        return 2 if any(t.derive for t in self.terms) else 1

    def blob(self) -> np.ndarray:
        words = [ARGS_MAGIC, self.version, self.k, self.alpha, self.beta, len(self.terms), len(self.records),
                 self.reads | (PAGES_BIT if self.pages is not None else 0) | (OPEN_BIT if self.open is not None else 0) |
                 (PORTS_BIT if self.ports else 0) | (WIDE_BIT if self.wide else 0) | (FLAT_BIT if self.flat else 0)]
        for t in _by_column(self.terms):
            rec = [t.col, 0 if t.sign == 1 else 1, NONE if t.sel is None else t.sel,
                   NONE if t.mult is None else t.mult[0], 0 if t.mult is None else t.mult[1], t.tag % P, len(t.tuple_cols), t.flags()]
            for g, c in t.tuple_cols:
                rec += [g, c]
            rec += [0] * (TERM_WORDS - len(rec))
            words += rec
        for r in self.records:
            words += r.words()
        return np.asarray(words, dtype=np.uint32)

    @staticmethod
    def parse(blob: Sequence[int]) -> "Arguments":
        d = [int(x) for x in np.asarray(blob, dtype=np.uint32)]
        if len(d) < ARGS_HEADER or d[0] != ARGS_MAGIC or d[1] not in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11) or (d[1] == 6 and d[7] == 0) or \
                (d[1] == 7 and not d[7] & PAGES_BIT) or (d[1] == 8 and not d[7] & OPEN_BIT) or (d[1] == 9 and not d[7] & PORTS_BIT) or \
                (d[1] == 10 and not d[7] & WIDE_BIT) or (d[1] == 11 and not d[7] & FLAT_BIT):
            raise ValueError("not a ZKA1 argument blob")
        version = d[1]
        k, alpha, beta, n = d[2], d[3], d[4], d[5]
        n_rec = d[6] if version >= 4 else 0
        at, sizes = ARGS_HEADER + TERM_WORDS * n, []
        for _ in range(n_rec):                                                # a LINK record (version 5) takes two slots
            if at > len(d):                                                   # past the blob's end: refused below, whatever n_rec says
                break
            wide = at < len(d) and ((version >= 5 and d[at] == KIND_LINK) or (version >= 7 and d[at] == KIND_PAGES))
            sizes.append(LINK_WORDS if wide else RECORD_WORDS)
            at += sizes[-1]
        if len(d) != at:
            raise ValueError(f"ZKA1: {len(d)} words for {n} terms" + (f" and {n_rec} records" if version >= 4 else ""))
        terms = []
        for i in range(n):
            r = d[ARGS_HEADER + TERM_WORDS * i: ARGS_HEADER + TERM_WORDS * (i + 1)]
            w = r[6]
            if not 1 <= w <= MAX_TUPLE:
                raise ValueError(f"ZKA1 term {i}: tuple width {w}")
            if version == 2 and r[7] > 1:
                raise ValueError(f"ZKA1 term {i}: word 7 is {r[7]} (bit 0: derived multiplicity; the other bits are reserved)")
            src, keys = None, ()
            if version >= 3:
                f = r[7]
                nkeys = f >> 4 & 7
                if f & 0x8C or (not f & 2 and f > 1) or any(f >> (8 + 2 * j) & 3 for j in range(nkeys, 4)):
                    raise ValueError(f"ZKA1 term {i}: word 7 is {f:#x} (bit 0: derived multiplicity; bit 1: sorted copy, with its keys in "
                                     f"bits 4..15 and its source term in bits 16..31; the other bits are reserved)")
                if f & 2:
                    src, keys = f >> 16, tuple(f >> (8 + 2 * j) & 3 for j in range(nkeys))
            terms.append(Term(col=r[0], tuple_cols=tuple((r[8 + 2 * j], r[9 + 2 * j]) for j in range(w)), sign=-1 if r[1] else 1,
                              sel=None if r[2] == NONE else r[2], mult=None if r[3] == NONE else (r[3], r[4]), tag=r[5],
                              derive=version >= 2 and r[7] & 1 == 1, sorted_from=src, sort_keys=keys))
        records = []
        for i in range(n_rec):
            at = ARGS_HEADER + TERM_WORDS * n + sum(sizes[:i])
            r = d[at: at + sizes[i]]
            if version >= 8 and r[0] == KIND_OPEN:
                records.append(Open(r[1], r[2], r[3], r[4], r[5], bool(any(r[6:]))))
                continue
            if sizes[i] == PAGES_WORDS and r[0] == KIND_PAGES:
                nv = 1 + min(r[4], MAX_PAGE_WORDS - 1) if version >= 10 else 1      # version 10: word 4 holds V - 1; reserved before
                n_dst = min(16, 3 + 2 * nv + 2 * min(r[2], 8))
                nf = 2 if version >= 11 and r[5] == 2 else 0                # version 11: word 5 holds F, words 6, 7 the columns; reserved before
                records.append(Pages(r[1], r[2], r[3], tuple(r[16: 16 + n_dst]),
                                     bool(any(r[6 + nf if version >= 11 else 5 if version >= 10 else 4:16]) or any(r[16 + n_dst:])), nv,
                                     r[4] if version >= 10 and r[4] >= MAX_PAGE_WORDS else None, version >= 10, tuple(r[6: 6 + nf]),
                                     r[5] if version >= 11 and r[5] not in (0, 2) else None, version >= 11))
                continue
            if sizes[i] == LINK_WORDS:
                nc = min(r[3], MAX_CARRIED)
                n_dst = min(16, 2 + nc + min(r[2], 16))
                joins = version >= 9 and r[5] & LINK_JOINS != 0             # version 9: bit 1 of word 5, and word 31 names the head
                reserved = bool(any(r[8 + 2 * nc:14]) or any(r[16 + n_dst:LINK_WORDS - 1 if joins else LINK_WORDS]))
                reads = version >= 6 and r[5] & 1 == 1                     # version 5 reserves words 5, 14, 15; version 6 reads them
                if version < 6:
                    reserved = reserved or bool(r[5] or r[14] or r[15])
                records.append(Link(None if r[4] == NONE else r[4], (r[6], r[7]), tuple((r[8 + 2 * j], r[9 + 2 * j]) for j in range(nc)), r[1], r[2],
                                    tuple(r[16: 16 + n_dst]), reserved, None if r[3] == nc else r[3], (r[14], r[15]) if reads else None,
                                    r[5] if version >= 6 and r[5] > (3 if version >= 9 else 1) else None,
                                    bool(version >= 6 and not reads and (r[14] or r[15])), r[LINK_WORDS - 1] if joins else None, version >= 9))
                continue
            n_src = r[3]
            n_dst = min(8, r[2] + (r[0] == KIND_ORDER and n_src == 2))
            reserved = any(r[4 + 2 * min(n_src, 2):8]) or any(r[8 + n_dst:])
            records.append(Record(r[0], r[1], r[2], tuple((r[4 + 2 * j], r[5 + 2 * j]) for j in range(min(n_src, 2))), tuple(r[8: 8 + n_dst]),
                                  reserved, None if n_src <= 2 else n_src))
        n_reads = sum(isinstance(r, Link) and r.write is not None for r in records)
        has_pages = any(isinstance(r, Pages) for r in records)
        word7 = d[7] ^ PAGES_BIT if version == 7 or (version >= 8 and d[7] & PAGES_BIT) else d[7]     # bit 16 says PAGES, the rest counts as before
        has_open = any(isinstance(r, Open) for r in records)
        if version == 8 or (version >= 9 and d[7] & OPEN_BIT):
            word7 ^= OPEN_BIT                                                # bit 17 says OPEN
        if version == 9 or (version >= 10 and d[7] & PORTS_BIT):
            word7 ^= PORTS_BIT                                               # bit 18 says PORTS
        if version == 10 or (version >= 11 and d[7] & WIDE_BIT):
            word7 ^= WIDE_BIT                                                # bit 19 says WIDE
        if version >= 11:
            word7 ^= FLAT_BIT                                                # bit 20 says FLAT
        if version >= 6 and word7 != n_reads:
            raise ValueError(f"ZKA1: header word 7 is {word7}, the blob has {n_reads} LINK records with READS")
        if version >= 7 and d[7] & PAGES_BIT and not has_pages:
            raise ValueError("ZKA1: header word 7 has bit 16 (PAGES), but the blob has no PAGES record")
        if version >= 8 and has_pages and not d[7] & PAGES_BIT:
            raise ValueError("ZKA1: the blob has a PAGES record, but header word 7 lacks bit 16 (PAGES)")
        if version >= 8 and d[7] & OPEN_BIT and not has_open:
            raise ValueError("ZKA1: header word 7 has bit 17 (OPEN), but the blob has no OPEN record")
        if version >= 9 and has_open and not d[7] & OPEN_BIT:
            raise ValueError("ZKA1: the blob has an OPEN record, but header word 7 lacks bit 17 (OPEN)")
        joiner = any(isinstance(r, Link) and r.joins is not None for r in records)
        if (version == 9 or (version >= 10 and d[7] & PORTS_BIT)) and not joiner:
            raise ValueError("ZKA1: header word 7 has bit 18 (PORTS), but no LINK record joins")
        if version >= 10 and joiner and not d[7] & PORTS_BIT:
            raise ValueError("ZKA1: a LINK record joins, but header word 7 lacks bit 18 (PORTS)")
        two = any(isinstance(r, Pages) and (r.nv > 1 or r.nv_word is not None) for r in records)
        if (version == 10 or (version >= 11 and d[7] & WIDE_BIT)) and not two:
            raise ValueError("ZKA1: header word 7 has bit 19 (WIDE), but no PAGES record pages two value words per address")
        if version >= 11 and two and not d[7] & WIDE_BIT:
            raise ValueError("ZKA1: a PAGES record pages two value words per address, but header word 7 lacks bit 19 (WIDE)")
        if version >= 11 and not any(isinstance(r, Pages) and (r.flats or r.nf_word is not None) for r in records):
            raise ValueError("ZKA1: header word 7 has bit 20 (FLAT), but no PAGES record has flat-address destinations")
        problem = check_sorted(terms) or check_derived(terms) or check_open(terms, records, (alpha, beta)) or _check_records(terms, records)
        if problem:
            raise ValueError(f"ZKA1: {problem}")
        return Arguments(k, alpha, beta, terms, records)

    def plain(self) -> "Arguments":
        """the same terms with nothing derived by the library (a version-1 blob): for a host that fills every column itself"""
        return Arguments(self.k, self.alpha, self.beta, [replace(t, derive=False, sorted_from=None, sort_keys=()) for t in self.terms])

    def by_column(self) -> List[List[Term]]:
        cols: List[List[Term]] = [[] for _ in range(self.k)]
        for t in self.terms:
            cols[t.col].append(t)
        return cols


class LogupBuilder(CircuitBuilder):
    """CircuitBuilder that also records argument terms and emits their constraints (`arguments`)."""

    def __init__(self, group_sizes, global_sizes, alpha: int = 0, beta: int = 4, kind: int = 0, open_bus: Optional[Tuple[int, int]] = None,
                 split_close: bool = False):
        """open_bus = (tag, total): the OPEN mode (the module docstring's open bus).  alpha and beta are then `out` word offsets, every
        term reads the challenges there, the terms of `tag` are answered by another seal and `arguments` closes the bus on the four
        `out` words at `total`.  The blob gets an OPEN record (ZKA1 version 8).
        split_close (open mode only; the module docstring's THE SPLIT CLOSURE): an accum column is OPEN when every term of it has the
        open tag and CLOSED when none has, a column that mixes them is refused, and `arguments` closes twice: the closed columns on
        zero, the open ones on the total.  The blob does not change: the description alone says how the bus closes."""
        super().__init__(tuple(group_sizes), tuple(global_sizes), kind=kind)
        if group_sizes[GROUP_ACCUM] % 4:
            raise ValueError("the accum group holds Fp4 columns: its width is a multiple of 4")
        for off in (alpha, beta):
            if open_bus is None and off + 4 > global_sizes[1]:
                raise ValueError(f"mix offset {off} needs {off + 4} mix words, the circuit has {global_sizes[1]}")
        self.alpha_off, self.beta_off = alpha, beta
        self.terms: List[Term] = []
        self.records: List[Record] = []
        self.open: Optional[Open] = None
        self.split_close = bool(split_close)
        if split_close and open_bus is None:
            raise ValueError("split_close is an option of the open bus (open_bus=...): a closed bus closes on zero as it stands")
        if open_bus is not None:
            self.open = Open(int(open_bus[0]), int(alpha), int(beta), int(open_bus[1]), int(global_sizes[0]))
            problem = check_open([Term(0, ((GROUP_DATA, 0),), tag=self.open.tag)], [self.open])     # the offsets; the terms come later
            if problem:
                raise ValueError(problem)

    @property
    def k(self) -> int:
        return self.group_sizes[GROUP_ACCUM] // 4

    def term(self, col: int, tuple_cols: Sequence[Tuple[int, int]], sign: int = 1, sel: Optional[int] = None,
             mult: Optional[Tuple[int, int]] = None, tag: int = 0, derive: bool = False, sorted_from: Optional[int] = None,
             sort_keys: Sequence[int] = ()) -> Term:
        """derive: the library fills `mult` (zkh_derive_multiplicities), the table side of a lookup (`check_derived`).
        sorted_from: the library fills this term's tuple columns (zkh_derive_sorted) with the rows of term `sorted_from` (its index in
        `self.terms`) stably sorted by the tuple positions `sort_keys`, most significant first (`check_sorted`)"""
        if not 0 <= col < self.k:
            raise ValueError(f"accum column {col} outside 0..{self.k - 1}")
        if sign not in (1, -1):
            raise ValueError("a term's sign is +1 or -1")
        if not 1 <= len(tuple_cols) <= MAX_TUPLE:
            raise ValueError(f"tuple width {len(tuple_cols)} outside 1..{MAX_TUPLE}")
        for g, c in list(tuple_cols) + ([mult] if mult is not None else []):
            if g not in (GROUP_CODE, GROUP_DATA) or not 0 <= c < self.group_sizes[g]:
                raise ValueError(f"column ({g}, {c}) is not a code or data column of this circuit")
        if sel is not None and not 0 <= sel < self.group_sizes[GROUP_CODE]:
            raise ValueError(f"selector {sel} is not a code column")
        if sorted_from is None and len(sort_keys):
            raise ValueError("sort_keys belong to a sorted copy (sorted_from)")
        if sorted_from is not None and not 0 <= int(sorted_from) < 1 << 16:
            raise ValueError(f"source term {sorted_from} outside 0..65535")
        t = Term(col, tuple((int(g), int(c)) for g, c in tuple_cols), sign, sel, mult, int(tag), bool(derive),
                 None if sorted_from is None else int(sorted_from), tuple(int(x) for x in sort_keys))
        self.terms.append(t)
        problem = check_sorted(self.terms) or check_derived(self.terms) or _check_records(self.terms, self.records, self.group_sizes)
        if problem:
            self.terms.pop()
            raise ValueError(problem)
        if self.split_close and len({self._is_open(x) for x in self.terms if x.col == col}) > 1:
            self.terms.pop()
            raise ValueError(f"accum column {col} mixes terms of the open tag {self.open.tag} with others (split_close: a column is open or closed)")
        deg = column_degree([x for x in self.terms if x.col == col])
        if deg > MAX_DEGREE:
            self.terms.pop()
            raise ValueError(f"accum column {col}: constraint degree {deg} exceeds {MAX_DEGREE} (at most 3 terms of single-column "
                             f"selectors and multiplicities per column)")
        return t

    def _is_open(self, t: Term) -> bool:
        return self.open is not None and t.tag % P == self.open.tag % P

    def _record(self, rec):
        # LIMBS / ORDER records, then LINK records, then the PAGES record, which names its LINK by index: that index moves with the LINK
        before = list(self.records)
        at = len(before) if isinstance(rec, Pages) else sum(isinstance(r, Record) or (isinstance(rec, Link) and isinstance(r, Link)) for r in before)
        if isinstance(rec, Link) and rec.joins is not None:                  # a joiner goes after the last port of its memory: a memory is one run
            at = memory_ports(before, rec.joins)[-1] + 1
        moved = lambda r: (replace(r, link=r.link + 1) if isinstance(r, Pages) and r.link >= at else
                           replace(r, joins=r.joins + 1) if isinstance(r, Link) and r.joins is not None and r.joins >= at else r)
        self.records = [moved(r) for r in before]
        self.records.insert(at, rec)
        problem = _check_records(self.terms, self.records, self.group_sizes)
        if problem:
            self.records = before
            raise ValueError(problem)
        return rec

    def derive_limbs(self, src: Tuple[int, int], dsts: Sequence[int], limb_bits: int) -> Record:
        """the library fills the data columns `dsts` (zkh_derive_columns) with the limbs of `limb_bits` bits of the (group, column)
        `src`, least significant first (`check_columns`); a value that does not fit them refuses the witness"""
        return self._record(Record(KIND_LIMBS, int(limb_bits), len(dsts), ((int(src[0]), int(src[1])),), tuple(int(c) for c in dsts)))

    def derive_order(self, keys: Sequence[Tuple[int, int]], dsts: Sequence[int], limb_bits: int) -> Record:
        """the library fills the data columns `dsts` with the order witness of the sorted (group, column) `keys`, one or two of them:
        with two keys dsts[0] is the flag "same k0 as the previous row" and dsts[1:] the limbs of the ordered difference, with one key
        dsts are the limbs (`reference_columns`); keys that are not in order refuse the witness"""
        keys = tuple((int(g), int(c)) for g, c in keys)
        return self._record(Record(KIND_ORDER, int(limb_bits), len(dsts) - (len(keys) == 2), keys, tuple(int(c) for c in dsts)))

    def derive_links(self, sel: Optional[int], key: Tuple[int, int], carried: Sequence[Tuple[int, int]], dsts: Sequence[int], limb_bits: int,
                     write: Optional[Tuple[int, int]] = None, joins: Optional[Link] = None) -> Link:
        """the library fills the data columns `dsts` (zkh_derive_links) = linked, last, one prev per carried column, then the limbs of
        the clock difference, for the accesses (selector code column `sel`, None = every active row) to the address `key`; `carried`
        are the (group, column) pairs whose value at the previous access is copied, carried[0] the clock (`reference_links`).
        write: the (group, column) of the write flag; the record then has READS (ZKA1 version 6) and a load that does not return the
        last store, or 0 from an address never accessed, refuses the witness (the module docstring's read rule).
        joins: a LINK record of this builder without `joins`, the head: this record is one more PORT of the head's memory (ZKA1 version
        9; the module docstring's PORTS), after the ports it has; the accesses of all ports are one memory's, ordered by (row, port)"""
        carried = tuple((int(g), int(c)) for g, c in carried)
        head = None
        if joins is not None:
            head = next((i for i, r in enumerate(self.records) if r is joins), None) if joins not in self.records else self.records.index(joins)
            if head is None:
                raise ValueError("derive_links: the head (joins=) is not one of this builder's LINK records")
        return self._record(Link(None if sel is None else int(sel), (int(key[0]), int(key[1])), carried, int(limb_bits),
                                 len(dsts) - 2 - len(carried), tuple(int(c) for c in dsts),
                                 write=None if write is None else (int(write[0]), int(write[1])), joins=head))

    def derive_pages(self, link_record: Link, dsts: Sequence[int], limb_bits: int, flats: Optional[Sequence[int]] = None) -> Pages:
        """the memory of the LINK record `link_record` (one of this builder's, with READS and a clock and one value column) is PAGED
        (ZKA1 version 7): its first access to an address takes the word of an image as its previous access, at clock 0, and the
        library fills the data columns `dsts` = p_on, p_addr, p_in, p_out, p_time, alimb_0 .., gap_0 .. (5 + 2 ng of them) with the page
        table: the distinct addresses in order, each with the image's word and what its last access left (`reference_links` with an
        image; zkh_derive_links_paged).  A LINK that carries two values (nc = 3) pages a memory of two value words per address (ZKA1
        version 10) and takes the wider list p_on, p_addr, p_in_0, p_in_1, p_out_0, p_out_1, p_time, alimb_0 .., gap_0 .. (7 + 2 ng).
        flats = (p_flat_0, p_flat_1), only on such a LINK (ZKA1 version 11): two more data columns, which the library fills with the flat
        addresses 2 a_i + j of page i (the module docstring, FLAT); `page_constraints` ties them to p_addr"""
        at = next((i for i, r in enumerate(self.records) if r is link_record), None)
        if at is None:
            at = self.records.index(link_record) if link_record in self.records else -1
        if at < 0:
            raise ValueError("derive_pages: the LINK record is not one of this builder's")
        nv = 2 if isinstance(link_record, Link) and link_record.nc == 3 else 1  # the link carries two values: the wider list
        if nv == 2 and (len(dsts) < 9 or (len(dsts) - 7) % 2):
            raise ValueError(f"derive_pages: {len(dsts)} destinations (7 + 2 ng for a LINK that carries two values: p_on, p_addr, p_in_0, p_in_1, p_out_0, "
                             f"p_out_1, p_time, ng address limbs, ng gap limbs; 5 + 2 ng for one value)")
        if nv == 1 and (len(dsts) < 7 or (len(dsts) - 5) % 2):
            raise ValueError(f"derive_pages: {len(dsts)} destinations (5 + 2 ng: p_on, p_addr, p_in, p_out, p_time, ng address limbs, ng gap limbs)")
        flats = tuple(int(c) for c in flats) if flats is not None else ()
        if flats and nv == 1:
            raise ValueError("derive_pages: flat-address columns on a LINK that carries one value (they are the flat addresses 2 a + j of a memory of two "
                             "value words per address)")
        if flats and len(flats) != 2:
            raise ValueError(f"derive_pages: {len(flats)} flat-address columns (2: p_flat_0, p_flat_1)")
        return self._record(Pages(int(limb_bits), (len(dsts) - 3 - 2 * nv) // 2, at, tuple(int(c) for c in dsts), nv=nv, flats=flats))

    def paged(self, record: Link) -> Optional[Pages]:
        """the PAGES record that pages the memory of the LINK `record` (the head it names, or a port that joins that head), or None"""
        head = record if record.joins is None or not 0 <= record.joins < len(self.records) else self.records[record.joins]
        return next((r for r in self.records if isinstance(r, Pages) and 0 <= r.link < len(self.records) and self.records[r.link] == head), None)

    def _limb_sum(self, cols, L):
        total = None
        for j, c in enumerate(cols):
            v = self.get(GROUP_DATA, c) if j == 0 else self.mul(self.const(1 << (j * L)), self.get(GROUP_DATA, c))
            total = v if total is None else self.add(total, v)
        return total

    def page_constraints(self, inner, body_inner, record: Pages):
        """and onto `inner` (which the caller gates by its active selector) p_on (1 - p_on) = 0 and sum_j 2^(jL) alimb_j = p_addr, and onto
        `body_inner` (gated by the body selector: every active row but the first) p_on (1 - p_on@1) = 0, so that p_on is a prefix, and
        p_on (p_addr - p_addr@1 - 1 - sum_j 2^(jL) gap_j) = 0 -> (inner, body_inner).  Degree 3 with the gates.  Range-checked address
        limbs and range-checked gaps (lookups, L ng <= 29 as in `order_constraints`) make the page addresses strictly increasing, hence
        distinct: no address is paged in twice, and memory cannot fork.
        A record with FLATS (ZKA1 version 11) adds onto `inner` p_on (p_flat_j - 2 p_addr - j) = 0 for j = 0, 1, degree 3 with the gate.  The
        address limbs bound p_addr below 2^29, so 2 p_addr + 1 < 2^30 < P and the field equation names one integer, the flat address; the
        page addresses increase strictly, so the flat addresses 2 a_i + j are pairwise distinct.  A record without flats emits exactly
        what it emitted."""
        if not isinstance(record, Pages):
            raise ValueError("page_constraints: not a PAGES record")
        L = record.limb_bits
        if L * record.ng > MAX_ORDER_BITS:
            raise ValueError(f"page_constraints: {record.ng} limbs of {L} bits exceed {MAX_ORDER_BITS} bits (a negative gap must stay out of range)")
        one = self.const(1)
        on, addr = self.get(GROUP_DATA, record.p_on), self.get(GROUP_DATA, record.p_addr)
        inner = self.and_eqz(inner, self.mul(on, self.sub(one, on)))
        inner = self.and_eqz(inner, self.sub(self._limb_sum(record.alimbs, L), addr))
        body_inner = self.and_eqz(body_inner, self.mul(on, self.sub(one, self.get(GROUP_DATA, record.p_on, 1))))
        gap = self.sub(self.sub(self.sub(addr, self.get(GROUP_DATA, record.p_addr, 1)), one), self._limb_sum(record.gaps, L))
        body_inner = self.and_eqz(body_inner, self.mul(on, gap))
        for j, c in enumerate(record.flats):                                 # p_on (p_flat_j - 2 p_addr - j) = 0
            flat = self.sub(self.get(GROUP_DATA, c), self.mul(self.const(2), addr))
            inner = self.and_eqz(inner, self.mul(on, flat if j == 0 else self.sub(flat, self.const(j))))
        return inner, body_inner

    def link_constraints(self, inner, record: Link):
        """and onto `inner` (which the caller gates by its body selector) the constraints that tie the LINK `record`'s witness to its
        row: linked (1 - linked) = 0, last (1 - last) = 0 and sum_j 2^(jL) limb_j = linked (c_0 - prev_0 - 1).  Degree 3 with the caller's
        gate.  Sound for clocks below 2^29 and limbs range-checked by a lookup, as `order_constraints` is: L nl <= 29.
        A record with READS adds the read rule: w (1 - w) = 0 and, per value column j >= 1, (1 - w) (c_j - linked prev_j) = 0: a load
        returns what the previous access left, or 0.  linked prev_j and not prev_j alone, so that nothing rests on the host having
        zeroed prev_j on an unlinked row.  Degree 4 with the gate.
        A PAGED record (`derive_pages`): linked, last and w are 0 / 1, and UNGATED sum_j 2^(jL) limb_j = c_0 - prev_0 - 1 and
        (1 - w) (c_j - prev_j) = 0 for every value column (j = 1; a wide memory: j = 1, 2): the first access to an address has the image's
        words at clock 0 as its previous access."""
        if not isinstance(record, Link):
            raise ValueError("link_constraints: not a LINK record")
        L, nl = record.limb_bits, record.nl
        if L * nl > MAX_ORDER_BITS:
            raise ValueError(f"link_constraints: {nl} limbs of {L} bits exceed {MAX_ORDER_BITS} bits (a negative difference must stay out of range)")
        one = self.const(1)
        linked, last = self.get(GROUP_DATA, record.linked), self.get(GROUP_DATA, record.last)
        inner = self.and_eqz(inner, self.mul(linked, self.sub(one, linked)))
        inner = self.and_eqz(inner, self.mul(last, self.sub(one, last)))
        if self.paged(record) is not None:                                   # an unlinked access has the image as its previous one: nothing is gated
            w = self.get(*record.write)
            inner = self.and_eqz(inner, self.mul(w, self.sub(one, w)))
            d = self.sub(self.sub(self.get(*record.carried[0]), self.get(GROUP_DATA, record.prevs[0])), one)
            inner = self.and_eqz(inner, self.sub(self._limb_sum(record.limbs, L), d))
            for src, prev in zip(record.carried[1:], record.prevs[1:]):      # one value, or (version 10) two
                inner = self.and_eqz(inner, self.mul(self.sub(one, w), self.sub(self.get(*src), self.get(GROUP_DATA, prev))))
            return inner
        total = self.const(0)
        for j, c in enumerate(record.limbs):
            v = self.get(GROUP_DATA, c) if j == 0 else self.mul(self.const(1 << (j * L)), self.get(GROUP_DATA, c))
            total = v if j == 0 else self.add(total, v)
        d = self.sub(self.sub(self.get(*record.carried[0]), self.get(GROUP_DATA, record.prevs[0])), one)
        inner = self.and_eqz(inner, self.sub(total, self.mul(linked, d)))
        if record.write is not None:
            load = self.sub(one, self.get(*record.write))
            inner = self.and_eqz(inner, self.mul(self.get(*record.write), load))
            for src, prev in zip(record.carried[1:], record.prevs[1:]):
                inner = self.and_eqz(inner, self.mul(load, self.sub(self.get(*src), self.mul(linked, self.get(GROUP_DATA, prev)))))
        return inner

    def order_constraints(self, inner, record: Record):
        """and onto `inner` (which the caller gates by its body selector) the constraints that the keys of the ORDER `record` are in
        order on this row against the previous one: e (1 - e) = 0, e (k0 - k0@1) = 0 and
        sum_j 2^(jL) limb_j = e (k1 - k1@1) + (1 - e) (k0 - k0@1 - 1); with one key sum_j 2^(jL) limb_j = k0 - k0@1.  Degree 3 with
        the caller's gate.  Sound for keys below 2^29 and limbs range-checked by a lookup: L nl <= 29 keeps a negative difference,
        P - |d| > 2^29, out of the limbs' range."""
        if record.kind != KIND_ORDER:
            raise ValueError("order_constraints: not an ORDER record")
        L, nl = record.limb_bits, record.nl
        if L * nl > MAX_ORDER_BITS:
            raise ValueError(f"order_constraints: {nl} limbs of {L} bits exceed {MAX_ORDER_BITS} bits (a negative difference must stay out of range)")
        two = len(record.srcs) == 2
        limbs = record.dsts[1:] if two else record.dsts
        total = None
        for j, c in enumerate(limbs):
            v = self.get(GROUP_DATA, c) if j == 0 else self.mul(self.const(1 << (j * L)), self.get(GROUP_DATA, c))
            total = v if total is None else self.add(total, v)
        d0 = self.sub(self.get(*record.srcs[0]), self.get(*record.srcs[0], 1))
        if not two:
            return self.and_eqz(inner, self.sub(total, d0))
        one = self.const(1)
        e = self.get(GROUP_DATA, record.dsts[0])
        d1 = self.sub(self.get(*record.srcs[1]), self.get(*record.srcs[1], 1))
        inner = self.and_eqz(inner, self.mul(e, self.sub(one, e)))
        inner = self.and_eqz(inner, self.mul(e, d0))
        want = self.add(self.mul(e, d1), self.mul(self.sub(one, e), self.sub(d0, one)))
        return self.and_eqz(inner, self.sub(total, want))

    # ---- Fp4 values as 4 Fp handles (None = a zero component) ----
    def _e_add(self, x, y):
        return [a if b is None else b if a is None else self.add(a, b) for a, b in zip(x, y)]

    def _e_sub(self, x, y):
        return [a if b is None else self.sub(self.const(0) if a is None else a, b) for a, b in zip(x, y)]

    def _e_scale(self, x, s: Fp):
        return [None if a is None else self.mul(a, s) for a in x]

    def _e_mul(self, x, y):
        """x * y mod (X^4 + 11)"""
        acc = [[] for _ in range(7)]
        for i in range(4):
            for j in range(4):
                if x[i] is not None and y[j] is not None:
                    acc[i + j].append(self.mul(x[i], y[j]))

        def total(lst):
            if not lst:
                return None
            s = lst[0]
            for v in lst[1:]:
                s = self.add(s, v)
            return s
        c = [total(a) for a in acc]
        nb = self.const(NBETA)
        for i in range(3):
            if c[4 + i] is not None:
                h = self.mul(nb, c[4 + i])
                c[i] = h if c[i] is None else self.add(c[i], h)
        return c[:4]

    def _mix4(self, off: int):
        """a challenge: four mix words, or in the open mode four `out` words"""
        return [self.get_global(GLOBAL_MIX if self.open is None else GLOBAL_OUT, off + i) for i in range(4)]

    def arguments(self, chain, first: Fp, body: Fp, last: Fp):
        """emit the argument constraints onto `chain`, gated by the code selectors first / body / last; returns the chain"""
        cols = [[t for t in self.terms if t.col == c] for c in range(self.k)]
        for c, ts in enumerate(cols):
            if not ts:
                raise ValueError(f"accum column {c} has no terms")
        alpha, beta = self._mix4(self.alpha_off), self._mix4(self.beta_off)
        wmax = max(len(t.tuple_cols) for t in self.terms)
        bpow = [beta]
        for _ in range(1, wmax):
            bpow.append(self._e_mul(bpow[-1], beta))
        acc = lambda c, back=0: [self.get(GROUP_ACCUM, 4 * c + i, back) for i in range(4)]
        first_inner, body_inner = self.true(), self.true()
        for c, ts in enumerate(cols):
            dens = []
            for t in ts:
                lin = [None] * 4
                for j, (g, col) in enumerate(t.tuple_cols):
                    lin = self._e_add(lin, self._e_scale(bpow[j], self.get(g, col)))
                if t.tag % P:
                    lin = self._e_add(lin, [self.const(t.tag), None, None, None])
                dens.append(self._e_sub(alpha, lin))
            den = dens[0]
            for d in dens[1:]:
                den = self._e_mul(den, d)
            num = [None] * 4
            for i, t in enumerate(ts):
                s = None
                if t.sel is not None:
                    s = self.get(GROUP_CODE, t.sel)
                if t.mult is not None:
                    m = self.get(*t.mult)
                    s = m if s is None else self.mul(s, m)
                rest = None
                for l, d in enumerate(dens):
                    if l != i:
                        rest = d if rest is None else self._e_mul(rest, d)
                if rest is None:
                    v = [s if s is not None else self.const(1), None, None, None]
                else:
                    v = rest if s is None else self._e_scale(rest, s)
                num = self._e_add(num, v) if t.sign == 1 else self._e_sub(num, v)
            cur, prev = acc(c), acc(c, 1)
            f = self._e_sub(self._e_mul(cur, den), num)
            b = self._e_sub(self._e_mul(self._e_sub(cur, prev), den), num)
            for i in range(4):
                first_inner = self.and_eqz(first_inner, f[i] if f[i] is not None else self.const(0))
                body_inner = self.and_eqz(body_inner, b[i] if b[i] is not None else self.const(0))
        chain = self.and_cond(chain, first, first_inner)
        chain = self.and_cond(chain, body, body_inner)
        if self.split_close:                                                 # two closing steps: the closed columns on zero, the open ones on the total
            last_inner = self.true()
            kinds = [{self._is_open(t) for t in ts} for ts in cols]
            for c, kind in enumerate(kinds):
                if len(kind) != 1:                                           # a column without terms was refused above: every column is in one sum
                    raise ValueError(f"accum column {c} mixes terms of the open tag {self.open.tag} with others (split_close: a column is open or closed)"
                                     if kind else f"accum column {c} has no terms")
            for is_open in (False, True):
                tot = [None] * 4
                for c, kind in enumerate(kinds):
                    if kind == {is_open}:
                        tot = self._e_add(tot, acc(c))
                if is_open:
                    tot = self._e_sub(tot, self._mix4(self.open.total))
                for i in range(4):
                    last_inner = self.and_eqz(last_inner, tot[i] if tot[i] is not None else self.const(0))
            return self.and_cond(chain, last, last_inner)
        tot = [None] * 4
        for c in range(self.k):
            tot = self._e_add(tot, acc(c))
        last_inner = self.true()
        if self.open is not None:                                            # the closing step: sum_c S_c = the total the seal states in `out`
            tot = self._e_sub(tot, self._mix4(self.open.total))
        for i in range(4):
            last_inner = self.and_eqz(last_inner, tot[i])
        return self.and_cond(chain, last, last_inner)

    def args(self) -> Arguments:
        args = Arguments(self.k, self.alpha_off, self.beta_off, _by_column(self.terms), list(self.records) + ([self.open] if self.open is not None else []))
        problem = check_open(args.terms, args.records)
        if problem:
            raise ValueError(problem)
        return args

    def finish_all(self, ret) -> Tuple[np.ndarray, np.ndarray]:
        """-> (ZKC1 description, ZKA1 argument blob)"""
        return self.finish(ret), self.args().blob()


# ---- host reference of the accumulate (numpy over canonical residues; the library's kernels work on Montgomery words) ----
_R = (1 << 32) % P
_RINV = pow(_R, -1, P)


def _dec(a):
    return (np.asarray(a, dtype=np.uint64) * np.uint64(_RINV)) % np.uint64(P)


def _enc(a):
    return ((np.asarray(a, dtype=np.uint64) % np.uint64(P)) * np.uint64(_R)) % np.uint64(P)


def _m(a, b):
    return (a * b) % np.uint64(P)


def _e_mul_np(x, y):
    c = [np.zeros_like(x[0]) for _ in range(7)]
    for i in range(4):
        for j in range(4):
            c[i + j] = (c[i + j] + _m(x[i], y[j])) % np.uint64(P)
    nb = np.uint64(NBETA)
    return [(c[i] + _m(c[i + 4], nb)) % np.uint64(P) if i < 3 else c[3] for i in range(4)]


def _fp_inv_np(a):
    r = np.ones_like(a)
    base = a.copy()
    e = P - 2
    while e:
        if e & 1:
            r = _m(r, base)
        base = _m(base, base)
        e >>= 1
    return r


def _e_inv_np(a):
    """the tower formula of fp4_inv (fp.h), canonical residues"""
    p = np.uint64(P)
    beta = np.uint64(11)
    a0, a1, a2, a3 = a
    b0 = (_m(a0, a0) + _m(beta, (_m((2 * a1) % p, a3) + p - _m(a2, a2)) % p)) % p
    b2 = (_m((2 * a0) % p, a2) + p - _m(a1, a1) + _m(beta, _m(a3, a3))) % p
    ic = _fp_inv_np((_m(b0, b0) + _m(beta, _m(b2, b2))) % p)
    b0, b2 = _m(b0, ic), _m(b2, ic)
    neg = lambda v: (p - v) % p
    return _e_mul_np([a0, neg(a1), a2, neg(a3)], [b0, np.zeros_like(b0), neg(b2), np.zeros_like(b0)])


class ReferenceError(ValueError):
    pass


def reference_accumulate(args: Arguments, po2: int, zk_cycles: int, code, data, mix, noise=None, check_balance: bool = True):
    """The accum trace (W_accum x 2^po2 raw Montgomery words) zkh_accumulate must produce, computed on the host.
    code / data / mix: raw Montgomery words as the library takes them.  noise(col) -> the zk_cycles blinding words of Fp column
    `col` (rows A..n-1), or None: zeros.  Raises ReferenceError on a vanishing denominator, and (check_balance) on a bus total
    that is not zero; returns (accum, total) with total the 4 canonical components of sum_c S_c[A-1].
    OPEN arguments (zkh_accumulate_open): `mix` is the challenge, alpha (4 words) then beta (4 words), whatever the offsets say; a
    total that is not zero is no refusal: it is what the call is for, and the seal states it in `out`."""
    n = 1 << po2
    A = n - zk_cycles
    groups = {GROUP_CODE: np.asarray(code, dtype=np.uint32).reshape(-1, n), GROUP_DATA: np.asarray(data, dtype=np.uint32).reshape(-1, n)}
    mixc = _dec(np.asarray(mix, dtype=np.uint32))
    is_open = args.open is not None
    if is_open and mixc.size != 8:
        raise ReferenceError(f"a challenge of {mixc.size} words (alpha and beta: 8)")
    alpha = [np.full(A, mixc[(0 if is_open else args.alpha) + i], dtype=np.uint64) for i in range(4)]
    beta = [np.full(A, mixc[(4 if is_open else args.beta) + i], dtype=np.uint64) for i in range(4)]
    bpow = [beta]
    for _ in range(MAX_TUPLE - 1):
        bpow.append(_e_mul_np(bpow[-1], beta))
    col = lambda g, c: _dec(groups[g][c, :A])
    accum = np.zeros((4 * args.k, n), dtype=np.uint32)
    total = [0, 0, 0, 0]
    for c, ts in enumerate(args.by_column()):
        s = [np.zeros(A, dtype=np.uint64) for _ in range(4)]
        for i, t in enumerate(ts):
            lin = [np.zeros(A, dtype=np.uint64) for _ in range(4)]
            for j, (g, cc) in enumerate(t.tuple_cols):
                v = col(g, cc)
                lin = [(lin[e] + _m(bpow[j][e], v)) % np.uint64(P) for e in range(4)]
            lin[0] = (lin[0] + np.uint64(t.tag % P)) % np.uint64(P)
            den = [(alpha[e] + np.uint64(P) - lin[e]) % np.uint64(P) for e in range(4)]
            zero = ~(den[0].astype(bool) | den[1].astype(bool) | den[2].astype(bool) | den[3].astype(bool))
            if zero.any():
                r = int(np.argmax(zero))
                raise ReferenceError(f"denominator vanishes at row {r}, accum column {c}, term {i}")
            inv = _e_inv_np(den)
            f = np.ones(A, dtype=np.uint64)
            if t.sel is not None:
                f = _m(f, col(GROUP_CODE, t.sel))
            if t.mult is not None:
                f = _m(f, col(*t.mult))
            if t.sign == -1:
                f = (np.uint64(P) - f) % np.uint64(P)
            s = [(s[e] + _m(inv[e], f)) % np.uint64(P) for e in range(4)]
        for e in range(4):
            run = np.cumsum(s[e] % np.uint64(P), dtype=np.uint64) % np.uint64(P)       # < 2^31 * 2^24: no wrap
            accum[4 * c + e, :A] = _enc(run).astype(np.uint32)
            total[e] = (total[e] + int(run[-1])) % P
            if noise is not None:
                accum[4 * c + e, A:] = np.asarray(noise(4 * c + e), dtype=np.uint32)
    if check_balance and not is_open and any(total):
        raise ReferenceError(f"the bus does not balance: total {total}")
    return accum.reshape(-1), total


def _canonical_key(terms: Sequence[Term], groups, i: int, rows) -> np.ndarray:
    """(len(rows), 5) keys (tag, v_0 .. v_3) of term i, canonical, the tuple zero-padded"""
    t = terms[i]
    key = np.zeros((len(rows), 1 + MAX_TUPLE), dtype=np.uint64)
    key[:, 0] = t.tag % P
    for j, (g, c) in enumerate(t.tuple_cols):
        key[:, 1 + j] = _dec(groups[g][c, rows])
    return key


def reference_multiplicities(args: Arguments, po2: int, zk_cycles: int, code, data) -> np.ndarray:
    """The data trace zkh_derive_multiplicities leaves (raw Montgomery words, a copy): for each derived term D and active row r,
    data[m_D][r] = the number of lookups (sum of sel * m in Fp) of the key of (D, r) if (D, r) is that key's representative (the table
    entry of smallest (blob term index, row)), else 0; rows [A, n) as given.  Raises ReferenceError on a table selector other than 0 / 1
    or on a lookup of nonzero weight whose key has no table entry."""
    n = 1 << po2
    A = n - zk_cycles
    terms = Arguments.parse(args.blob()).terms                               # blob order: the term index of the representative rule
    groups = {GROUP_CODE: np.asarray(code, dtype=np.uint32).reshape(-1, n), GROUP_DATA: np.array(data, dtype=np.uint32).reshape(-1, n)}
    out = groups[GROUP_DATA]
    rows = np.arange(A)
    tags = sorted({t.tag % P for t in terms if t.derive})
    for tag in tags:
        derived = [i for i, t in enumerate(terms) if t.derive and t.tag % P == tag]
        lookups = [i for i, t in enumerate(terms) if not t.derive and t.tag % P == tag]
        keys, owner = [], []
        for i in derived:
            t = terms[i]
            sel = np.ones(A, dtype=np.uint64) if t.sel is None else _dec(groups[GROUP_CODE][t.sel, :A])
            bad = (sel != 0) & (sel != 1)
            if bad.any():
                r = int(np.argmax(bad))
                raise ReferenceError(f"table term {i} (tag {tag}) has selector {int(sel[r])} at row {r}, not 0 or 1")
            on = rows[sel == 1]
            keys.append(_canonical_key(terms, groups, i, on))
            owner.append(np.stack([np.full(on.size, i), on], axis=1))
        tk, to = np.concatenate(keys), np.concatenate(owner)
        # sort by (key, term, row): the first entry of every distinct key is its representative
        order = np.lexsort(tuple(to[:, ::-1].T) + tuple(tk[:, ::-1].T))
        tk, to = tk[order], to[order]
        first = np.ones(len(tk), dtype=bool)
        first[1:] = (tk[1:] != tk[:-1]).any(axis=1)
        uk, uo = tk[first], to[first]
        counts = np.zeros(len(uk), dtype=np.uint64)
        for i in lookups:
            t = terms[i]
            w = np.ones(A, dtype=np.uint64)
            if t.sel is not None:
                w = _m(w, _dec(groups[GROUP_CODE][t.sel, :A]))
            if t.mult is not None:
                w = _m(w, _dec(groups[t.mult[0]][t.mult[1], :A]))
            live = rows[w != 0]
            lk = _canonical_key(terms, groups, i, live)
            allk = np.concatenate([uk, lk])
            _, inv = np.unique(allk, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
            slot = np.full(inv.max() + 1, -1, dtype=np.int64)
            slot[inv[:len(uk)]] = np.arange(len(uk))
            hit = slot[inv[len(uk):]]
            if (hit < 0).any():
                j = int(np.argmax(hit < 0))
                v = [int(x) for x in lk[j, 1:]]
                raise ReferenceError(f"lookup term {i} (tag {tag}) at row {int(live[j])} has no table entry: key ({v[0]}, {v[1]}, {v[2]}, {v[3]})")
            np.add.at(counts, hit, w[live])
        for i in derived:
            out[terms[i].mult[1], :A] = 0
        mcol = np.array([terms[i].mult[1] for i in uo[:, 0]], dtype=np.int64)
        out[mcol, uo[:, 1]] = _enc(counts % np.uint64(P)).astype(np.uint32)
    return out.reshape(-1)


def reference_sorted(args: Arguments, po2: int, zk_cycles: int, code, data) -> np.ndarray:
    """The data trace zkh_derive_sorted leaves (raw Montgomery words, a copy).  For each sorted copy D of S: r_0 < ... < r_{m-1} the
    active rows with selector 1 (no selector: all of them), pi the stable permutation that sorts them by the canonical values of
    S's key columns (lexicographic in the blob's key order); data[D.v_e][r_j] = the raw word of S.v_e at r_pi(j) for every tuple
    position e, 0 on the active rows with selector 0; rows [A, n) as given.  Raises ReferenceError on a selector other than 0 / 1."""
    n = 1 << po2
    A = n - zk_cycles
    terms = Arguments.parse(args.blob()).terms
    groups = {GROUP_CODE: np.asarray(code, dtype=np.uint32).reshape(-1, n), GROUP_DATA: np.array(data, dtype=np.uint32).reshape(-1, n)}
    out = groups[GROUP_DATA]
    copies = [(i, t) for i, t in enumerate(terms) if t.sorted_from is not None]
    on = {}
    for i, t in copies:
        sel = np.ones(A, dtype=np.uint64) if t.sel is None else _dec(groups[GROUP_CODE][t.sel, :A])
        bad = (sel != 0) & (sel != 1)
        if bad.any():
            r = int(np.argmax(bad))
            raise ReferenceError(f"sorted-copy term {i} (tag {t.tag % P}) has selector {int(sel[r])} at row {r}, not 0 or 1")
        on[i] = np.nonzero(sel == 1)[0]
    for i, t in copies:
        src, rows = terms[t.sorted_from], on[i]
        keys = [_dec(groups[src.tuple_cols[pos][0]][src.tuple_cols[pos][1], rows]) for pos in t.sort_keys]
        pi = np.lexsort(tuple(keys[::-1]))                                   # the last array is the primary key; stable
        vals = [groups[g][c, rows[pi]] for g, c in src.tuple_cols]             # read before any column of D is written
        for (_g, c), v in zip(t.tuple_cols, vals):
            out[c, :A] = 0
            out[c, rows] = v
    return out.reshape(-1)


def reference_columns(args: Arguments, po2: int, zk_cycles: int, code, data) -> np.ndarray:
    """The data trace zkh_derive_columns leaves (raw Montgomery words, a copy): every record's destination columns on the active rows
    (module docstring), rows [A, n) as given.  Raises ReferenceError, naming the lowest (record, row) and the offending value, on a
    LIMBS value or an ORDER difference that does not fit the limbs and on keys that are not in order."""
    n = 1 << po2
    A = n - zk_cycles
    groups = {GROUP_CODE: np.asarray(code, dtype=np.uint32).reshape(-1, n), GROUP_DATA: np.array(data, dtype=np.uint32).reshape(-1, n)}
    out = groups[GROUP_DATA]                                                 # sources are never destinations: no record reads what another wrote
    for i, r in enumerate(args.records):
        if not isinstance(r, Record):                                        # reference_links
            continue
        L, nl, bits = r.limb_bits, r.nl, r.limb_bits * r.nl
        k = [_dec(groups[g][c, :A]).astype(np.int64) for g, c in r.srcs]
        flag = None
        if r.kind == KIND_LIMBS:
            d = k[0]
        else:
            d = np.zeros(A, dtype=np.int64)
            if len(k) == 1:
                d[1:] = k[0][1:] - k[0][:-1]
            else:
                flag = np.zeros(A, dtype=np.int64)
                flag[1:] = k[0][1:] == k[0][:-1]
                d[1:] = np.where(flag[1:] == 1, k[1][1:] - k[1][:-1], k[0][1:] - k[0][:-1] - 1)
        bad = (d < 0) | (d >> bits != 0)
        if bad.any():
            row = int(np.argmax(bad))
            v = int(d[row])
            if r.kind == KIND_LIMBS:
                raise ReferenceError(f"record {i} at row {row}: the value {v} does not fit {nl} limbs of {L} bits")
            if v < 0:
                raise ReferenceError(f"record {i} at row {row}: not ordered (difference {v})")
            raise ReferenceError(f"record {i} at row {row}: the difference {v} does not fit {nl} limbs of {L} bits")
        dsts = list(r.dsts)
        if flag is not None:
            out[dsts.pop(0), :A] = _enc(flag).astype(np.uint32)
        for j, c in enumerate(dsts):
            out[c, :A] = _enc((d >> (j * L)) & ((1 << L) - 1)).astype(np.uint32)
    return out.reshape(-1)


def _link_chain(key, rows):
    """for the access rows `rows` (ascending) with canonical keys `key` (one per access): (prev, last) = the index into `rows` of the
    previous access to the same key (-1: none), and whether no later access has it — by one stable sort, as the library does"""
    order = np.argsort(key, kind="stable")
    sk = key[order]
    same = sk[1:] == sk[:-1]
    prev = np.full(len(rows), -1, dtype=np.int64)
    prev[order[1:][same]] = order[:-1][same]
    last = np.ones(len(rows), dtype=bool)
    last[order[:-1][same]] = False
    return prev, last


PAGES_NEED_IMAGE = "the arguments page memory: an image is required (zkh_derive_all_paged)"


def image_not_whole(words: int, nv: int) -> str:
    """the refusal of an image whose length is no multiple of the value words per address, before any launch"""
    return f"an image of {words} words is not a whole number of addresses of {nv} value words"


def reference_links(args: Arguments, po2: int, zk_cycles: int, code, data, image=None, table=None, image_words=None) -> np.ndarray:
    """The data trace zkh_derive_links leaves (raw Montgomery words, a copy): every LINK record's destination columns on the active rows
    (module docstring), rows [A, n) as given.  Raises ReferenceError on a selector other than 0 / 1 (the lowest (record, row) over all
    records, before any clock is looked at), then on the lowest (record, row) whose clock difference d = c_0 - prev_0 - 1 is negative
    ("clock not increasing") or does not fit the limbs or, in a record with READS, whose write flag is not 0 / 1 or whose load does
    not return the last store (0 when its address was never accessed); on one row in this order: write flag, clock, read rule.
    image: the W raw Montgomery words of the memory image, needed exactly when the arguments hold a PAGES record (ZKA1 version 7;
    zkh_derive_links_paged).  The paged LINK record then takes, for an unlinked access to address a (the canonical value of its key),
    the image as the previous access — prev_1 = the raw word image[a], prev_0 = 0, the limbs those of d = clock - 0 - 1 — refuses an
    address >= W, a clock 0 ("clock 0 is the image's") and an unlinked load whose residue is not image[a]'s (on one row: write flag,
    address, clock, read rule), and the PAGES record's destinations get the page table (module docstring, PAGING).
    table, image_words: the page table of a ZKU1 proof in the image's place (zkh_derive_links_paged_table): D rows (a_i, in_i, out_i) over
    an image of image_words words, exactly one of `image` / `table` being given.  The table stands for the image: with a_0 < a_1 < .. the
    distinct addresses of the paged record's accesses, an unlinked access to its address number I (page I of the trace) takes in_I where
    it took image[a].  The results and the messages are the image's (image_words in W's place), and three refusals are the table's own,
    under the PAGES record's index R: on a row, after the address and before the clock, "address A is page I of the trace, but the page
    table has D rows" and "... but row I of the page table holds address B"; and, when no row is refused, "record R: the trace pages D'
    addresses, but the page table has D rows"."""
    n = 1 << po2
    A = n - zk_cycles
    groups = {GROUP_CODE: np.asarray(code, dtype=np.uint32).reshape(-1, n), GROUP_DATA: np.array(data, dtype=np.uint32).reshape(-1, n)}
    out = groups[GROUP_DATA]                                                 # sources are never destinations
    links = [(i, r) for i, r in enumerate(args.records) if isinstance(r, Link)]
    pages = args.pages
    if image is not None and table is not None:
        raise ValueError("reference_links: exactly one of image / table")
    if pages is not None and image is None and table is None:
        raise ReferenceError(PAGES_NEED_IMAGE)
    V = pages.nv if pages is not None else 1                                # the value words per address: the image and the table are FLAT, word j of address a at V a + j
    if pages is not None and table is None:
        image = np.asarray(image, dtype=np.uint32).reshape(-1)
        if image.size % V:
            raise ReferenceError(image_not_whole(image.size, V))
        W = image.size // V
    elif pages is not None:
        if image_words is None or not 1 <= image_words <= 0xffffffff:
            raise ReferenceError(f"an image of {image_words} words (1 .. 2^32 - 1)")
        if image_words % V:
            raise ReferenceError(image_not_whole(image_words, V))
        table = np.asarray(table, dtype=np.uint32).reshape(-1, 3)
        W, R, short = image_words // V, args.records.index(pages), None
    on = {}
    for i, r in links:
        sel = np.ones(A, dtype=np.uint64) if r.sel is None else _dec(groups[GROUP_CODE][r.sel, :A])
        bad = (sel != 0) & (sel != 1)
        if bad.any():
            row = int(np.argmax(bad))
            raise ReferenceError(f"record {i} at row {row}: selector {int(sel[row])}, not 0 or 1")
        on[i] = np.nonzero(sel == 1)[0]
    writes, late = [], None                                                  # (columns, rows, words): nothing is written before every record passed
    for i0, head in links:
        if head.joins is not None:                                           # a port: its memory was its head's turn
            continue
        ports = [(i, args.records[i]) for i in memory_ports(args.records, i0)]
        L, nl = head.limb_bits, head.nl
        paged = pages is not None and pages.link == i0
        # the memory's accesses (row, port) in that order; a memory of one record: its rows
        row = np.concatenate([on[i] for i, _ in ports])
        port = np.concatenate([np.full(on[i].size, q, dtype=np.int64) for q, (i, _) in enumerate(ports)])
        by = np.lexsort((port, row))
        row, port = row[by], port[by]
        rec = np.asarray([i for i, _ in ports], dtype=np.int64)[port]

        def take(cols, rows, at):
            """the raw words of the per-port (group, column) `cols` at the accesses (rows, at)"""
            out_ = np.zeros(rows.size, dtype=np.uint32)
            for q, (g, c) in enumerate(cols):
                out_[at == q] = groups[g][c, rows[at == q]]
            return out_
        keys, carried = [r.key for _, r in ports], [[r.carried[e] for _, r in ports] for e in range(len(head.carried))]
        addr = _dec(take(keys, row, port)).astype(np.int64)
        prev, last = _link_chain(addr, row)
        linked = prev >= 0
        pat = np.where(linked, prev, 0)
        prow, pport = (row[pat], port[pat]) if row.size else (row, port)
        prec = rec[pat] if row.size else rec
        clock, pclock = _dec(take(carried[0], row, port)).astype(np.int64), _dec(take(carried[0], prow, pport)).astype(np.int64)
        d = np.where(linked, clock - pclock - 1, clock - 1 if paged else 0)
        bad = (d < 0) | (d >> (L * nl) != 0)
        if paged:
            outside = addr >= W
            if table is None:                                                # the image's words of an unlinked access: words[j] = image[V a + j]
                words = [image[V * np.where(outside, 0, addr) + j] if W else np.zeros(row.size, dtype=np.uint32) for j in range(V)]
                unlisted = np.zeros(row.size, dtype=bool)
            else:                                                            # ... by its page: the number of its address among the trace's, rows V page + j
                page = np.searchsorted(np.unique(addr), addr)
                words, listed, flat = [], np.ones(row.size, dtype=bool), np.zeros(row.size, dtype=np.int64)
                for j in reversed(range(V)):                                 # `flat`: the lowest flat row that does not list the access
                    at = V * page + j
                    row_of = np.minimum(at, max(len(table) - 1, 0))
                    here = (at < len(table)) & (table[row_of, 0] == V * addr + j if len(table) else False)
                    words.insert(0, np.where(at < len(table), table[row_of, 1] if len(table) else 0, 0).astype(np.uint32))
                    flat = np.where(here, flat, at)
                    listed &= here
                unlisted = ~linked & ~outside & ~listed
                short = (V * np.unique(addr).size, len(table), np.unique(addr).size)
            word = words[0]
            bad = bad | outside | unlisted
        if head.write is not None:
            w = _dec(take([r.write for _, r in ports], row, port))
            now = [_dec(take(cols, row, port)) for cols in carried]
            before = [np.where(linked, _dec(take(cols, prow, pport)), _dec(words[e - 1]) if paged and e >= 1 else 0) for e, cols in enumerate(carried)]
            misread = [(w == 0) & (now[e] != before[e]) for e in range(1, len(carried))]
            bad = bad | (w > 1) | np.logical_or.reduce(misread)
        if bad.any():
            cand = np.nonzero(bad)[0]
            j = int(cand[np.lexsort((row[cand], rec[cand]))[0]])             # the lowest (record, row), the record the port's own
            at = f"record {int(rec[j])} at row {int(row[j])}"
            there = f"row {int(prow[j])}" + (f" of record {int(prec[j])}" if prec[j] != rec[j] else "")      # the previous access, where it lies
            if head.write is not None and w[j] > 1:
                raise ReferenceError(f"{at}: write flag {int(w[j])}, not 0 or 1")
            if paged and outside[j]:
                raise ReferenceError(f"{at}: address {int(addr[j])} outside the image of {W} words")
            if paged and unlisted[j]:
                page_at = f"record {R} at row {int(row[j])}: address {int(addr[j])} is page {int(page[j])} of the trace, but "
                raise ReferenceError(page_at + (f"the page table has {len(table)} rows" if flat[j] >= len(table) else
                                                f"row {int(flat[j])} of the page table holds address {int(table[flat[j], 0])}"))
            if paged and not linked[j] and clock[j] == 0:
                raise ReferenceError(f"{at}: clock 0 is the image's")
            if head.write is not None and d[j] >= 0 and d[j] >> (L * nl) == 0:
                e = next(e for e in range(1, len(carried)) if misread[e - 1][j])
                raise ReferenceError(f"{at}: a load of carried column {e} returns {int(now[e][j])}, but " + (
                    f"{int(before[e][j])} was last stored ({there})" if linked[j] else
                    f"the image holds {int(before[e][j])} at its address {int(addr[j])}" if paged else "its address was never accessed: the value must be 0"))
            if d[j] < 0:
                raise ReferenceError(f"{at}: clock not increasing ({int(clock[j])} after {int(pclock[j])} at {there})")
            after = f"after {there}" if linked[j] else "after the image"
            raise ReferenceError(f"{at}: the clock difference {int(d[j])} ({after}) does not fit {nl} limbs of {L} bits")
        vals = [np.where(linked, take(cols, prow, pport), words[e - 1] if paged and e >= 1 else 0).astype(np.uint32) for e, cols in enumerate(carried)]
        for q, (_, r) in enumerate(ports):                                   # destinations stay per record: port q writes its own columns
            mine = port == q
            rows = row[mine]
            writes.append((list(r.dsts), slice(0, A), 0))
            writes.append((r.linked, rows, _enc(linked[mine].astype(np.uint64)).astype(np.uint32)))
            writes.append((r.last, rows, _enc(last[mine].astype(np.uint64)).astype(np.uint32)))
            writes += [(c, rows, v[mine]) for c, v in zip(r.prevs, vals)]
            writes += [(c, rows, _enc((d[mine] >> (j * L)) & ((1 << L) - 1)).astype(np.uint32)) for j, c in enumerate(r.limbs)]
        if paged:                                                            # the page table: the distinct addresses in order
            first, final = np.nonzero(~linked)[0], np.nonzero(last)[0]       # the first and the last access of every address ...
            first, final = first[np.argsort(addr[first], kind="stable")], final[np.argsort(addr[final], kind="stable")]       # ... by address
            a = addr[first]
            D, Lp, ng = a.size, pages.limb_bits, pages.ng
            wide = a >> (Lp * ng) != 0
            if wide.any():
                j = int(np.min(first[wide]))                             # the lowest (row, port): the accesses are in that order
                late = f"record {args.records.index(pages)} at row {int(row[j])}: address {int(addr[j])} does not fit {ng} limbs of {Lp} bits"
                continue                                                     # the PAGES record comes last: any LINK's refusal goes first
            if D > A:                                                        # only with ports: k A accesses may touch more than A addresses
                late = f"record {args.records.index(pages)}: the trace pages {D} addresses, but the page table has the {A} active rows"
                continue
            gap = np.zeros(D, dtype=np.int64)
            gap[1:] = a[1:] - a[:-1] - 1
            top = slice(0, D)
            writes.append((list(pages.dsts) + list(pages.flats), slice(0, A), 0))
            for j, c in enumerate(pages.flats):                              # FLAT: the canonical encoding of 2 a_i + j, from the decoded address
                writes.append((c, top, _enc(2 * a + j).astype(np.uint32)))
            writes.append((pages.p_on, top, np.uint32(_R)))
            writes.append((pages.p_addr, top, take(keys, row[first], port[first])))
            for j in range(V):                                               # the head writes p_in_j, the tail p_out_j from its own record
                writes.append((pages.p_ins[j], top, image[V * a + j] if table is None else table[j:V * D:V, 1] if len(table) >= V * D else 0))
                writes.append((pages.p_outs[j], top, take(carried[1 + j], row[final], port[final])))
            writes.append((pages.p_time, top, take(carried[0], row[final], port[final])))
            for j in range(ng):
                writes.append((pages.alimbs[j], top, _enc((a >> (j * Lp)) & ((1 << Lp) - 1)).astype(np.uint32)))
                writes.append((pages.gaps[j], top, _enc((gap >> (j * Lp)) & ((1 << Lp) - 1)).astype(np.uint32)))
    if late:
        raise ReferenceError(late)
    if pages is not None and table is not None and short is not None and short[0] != short[1]:
        raise ReferenceError(f"record {R}: the trace pages {short[2]} addresses, but the page table has {short[1]} rows")
    for cols, rows, words in writes:
        out[cols, rows] = words
    return out.reshape(-1)


def reference_page_out(args: Arguments, po2: int, zk_cycles: int, data, image) -> np.ndarray:
    """The image zkh_page_out leaves (raw Montgomery words, a copy): image[x(p_addr, i)] = the raw word p_out[i] on every active row i
    with p_on = 1 of the PAGES record's table in `data`.  Raises ReferenceError, with the image unchanged, on the lowest row whose
    p_on is not 0 / 1, whose address is outside the image or, the table being the host's own, whose address does not follow a smaller
    one: the page addresses of rows 0 .. D - 1 strictly increase and p_on is 1 exactly there, as the circuit demands, so no address
    is written twice (a repeated address is REFUSED, not resolved).  On one row in this order."""
    out = np.array(image, dtype=np.uint32).reshape(-1)
    d, live = _page_table(args, po2, zk_cycles, data, out.size)
    A = (1 << po2) - zk_cycles
    pages = args.pages
    for j, c in enumerate(pages.p_outs):                                     # the image is flat: word j of address a at V a + j
        out[pages.nv * _dec(d[pages.p_addr, :A][live]).astype(np.int64) + j] = d[c, :A][live]
    return out


def image_tree_leaves(image_words: int) -> int:
    """L of an image of W >= 1 words: the smallest power of two >= ceil(W / 8)"""
    L = 1
    while 8 * L < image_words:
        L <<= 1
    return L


def _hash_pairs(left, right) -> np.ndarray:
    """hash_pair of k pairs of digests, (k, 8) each, as ONE batch through the library's host permutation (zkh_poseidon2_mix_host)"""
    import ctypes as C
    from .. import hal as _hal
    _hal.load_library()
    st = np.zeros((len(left), 24), dtype=np.uint32)
    st[:, :8], st[:, 8:16] = left, right
    _hal._check(_hal._lib.zkh_poseidon2_mix_host(None, None, st.ctypes.data_as(C.POINTER(C.c_uint32)), len(left)))
    return st[:, :8].copy()


def reference_image_tree(image) -> np.ndarray:
    """THE IMAGE'S COMMITMENT (zkh_image_commit, zkh_page_out_tree; include/zkhal.h): the (2 L, 8) array of digests in heap order over an
    image of W >= 1 raw Montgomery words, W <= 2^32 - 1.  A function of the residues: image[a] and image[a] + P are one memory and give
    one tree.  L = the smallest power of two >= ceil(W / 8); digest 0 is eight zeros; leaf L + j, word k, is image[8 j + k] % P for
    8 j + k < W and 0 past the end of the image (the last partial leaf and every padding leaf): eight memory words verbatim, not a hash;
    node i, 1 <= i < L, is hash_pair(node 2 i, node 2 i + 1), the operation P2-JOIN constrains; the root is digest 1 (L = 1: the leaf)."""
    words = np.asarray(image, dtype=np.uint32).reshape(-1)
    W = words.size
    if not 1 <= W <= 0xffffffff:
        raise ReferenceError(f"an image of {W} words (1 .. 2^32 - 1)")
    L = image_tree_leaves(W)
    nodes = np.zeros((2 * L, 8), dtype=np.uint32)
    nodes[L:].reshape(-1)[:W] = words % np.uint32(P)
    width = L // 2
    while width:
        nodes[width:2 * width] = _hash_pairs(nodes[2 * width:4 * width:2], nodes[2 * width + 1:4 * width:2])
        width //= 2
    return nodes


def reference_image_root(image) -> np.ndarray:
    """the root of `reference_image_tree`: digest 1, 8 words"""
    return reference_image_tree(image)[1].copy()


PROOF_MAGIC = 0x5A4B5531                        # 'ZKU1'
PROOF_HEADER = 5


def _tree_height(image_words: int) -> int:
    return image_tree_leaves(image_words).bit_length() - 1


def image_proof_words(image_words: int, pages: int) -> int:
    """zkh_image_proof_words: the bound 5 + h + 3 D + 8 min(D, L) + 8 sum_{k<h} min(D, L >> (k + 1)) on the words of a ZKU1 proof of D
    pages over an image of W words (a clean sibling shares its pair with a dirty node: c_k is at most D and at most the pairs)"""
    L, D = image_tree_leaves(image_words), int(pages)
    h = L.bit_length() - 1
    return PROOF_HEADER + h + 3 * D + 8 * min(D, L) + 8 * sum(min(D, L >> (k + 1)) for k in range(h))


def _page_table(args: Arguments, po2: int, zk_cycles: int, data, W: int, leaves=None):
    """the check pass of the page-out family -> (d, live): the data trace as (columns, n) and the mask of the table's rows over the
    active ones; raises ReferenceError on the lowest refused row.  leaves: the tree's leaf layer as flat words (the proof's fourth
    refusal: p_in is not the word the tree holds)"""
    n = 1 << po2
    A = n - zk_cycles
    pages = args.pages
    if pages is None:
        raise ReferenceError("the arguments hold no PAGES record (ZKA1 version 7)")
    i, V = args.records.index(pages), pages.nv
    if W % V:
        raise ReferenceError(image_not_whole(W, V))
    if V > 1 and W > P:
        raise ReferenceError(f"an image of {W} words of a memory of two value words per address (at most P: its flat addresses are field elements)")
    W //= V                                                                  # W: the flat image's words on entry, its addresses from here on
    d = np.asarray(data, dtype=np.uint32).reshape(-1, n)
    on, addr = _dec(d[pages.p_on, :A]).astype(np.int64), _dec(d[pages.p_addr, :A]).astype(np.int64)
    pon, paddr = np.concatenate([[1], on[:-1]]), np.concatenate([[-1], addr[:-1]])
    live = on == 1
    follows = (pon == 1) & (paddr < addr)
    bad = (on > 1) | (live & ((addr >= W) | ~follows))
    if leaves is not None:
        held = [leaves[V * np.where(live & (addr < W), addr, 0) + j] for j in range(V)]
        differs = [live & (d[c, :A] % np.uint32(P) != held[j]) for j, c in enumerate(pages.p_ins)]
        bad |= np.logical_or.reduce(differs)
    if bad.any():
        r = int(np.argmax(bad))
        at = f"record {i} at row {r}"
        if on[r] > 1:
            raise ReferenceError(f"{at}: p_on {int(on[r])}, not 0 or 1")
        if addr[r] >= W:
            raise ReferenceError(f"{at}: address {int(addr[r])} outside the image of {W} words")
        if not follows[r]:
            raise ReferenceError(f"{at}: page address {int(addr[r])} does not follow a smaller one (row {r - 1}: p_on {int(pon[r])}, address {int(paddr[r])})")
        j = next(j for j in range(V) if differs[j][r])                      # the lowest word first; "word j" only where there are two
        raise ReferenceError(f"{at}: p_in {f'word {j} ' if V > 1 else ''}{int(_dec(d[pages.p_ins[j], r]))} at address {int(addr[r])}, the tree holds {int(_dec(held[j][r]))}")
    return d, live


def reference_page_out_proof(args: Arguments, po2: int, zk_cycles: int, data, image_words: int, nodes) -> np.ndarray:
    """The ZKU1 proof zkh_page_out_proof writes (include/zkhal.h "THE UPDATE'S PROOF"), word for word: the page table of `data` over an
    image of `image_words` words whose committed tree is `nodes` (`reference_image_tree`, before the page-out).  It hashes nothing:
    every digest is read from `nodes`.  Raises ReferenceError on the lowest refused row as `reference_page_out` does and, after its
    three refusals on a row, when p_in % P is not the word the tree holds; and on a `nodes` of another size."""
    W = int(image_words)
    L = image_tree_leaves(W)
    nodes = np.asarray(nodes, dtype=np.uint32).reshape(-1)
    if not W or nodes.size != 16 * L:
        raise ReferenceError(f"nodes of {nodes.size} words; an image of {W} words has a tree of {16 * L if W else 0} (zkh_image_tree_words)")
    nodes = nodes.reshape(-1, 8)
    d, live = _page_table(args, po2, zk_cycles, data, W, leaves=nodes[L:].reshape(-1))
    A = (1 << po2) - zk_cycles
    pages = args.pages
    V = pages.nv                                                             # THE FLAT TABLE: V rows (V a_i + j, in_j, out_j) per page, i major, j minor
    a = (V * _dec(d[pages.p_addr, :A][live]).astype(np.int64)[:, None] + np.arange(V)).reshape(-1)
    h = L.bit_length() - 1
    flat = lambda cols: np.stack([d[c, :A][live] % np.uint32(P) for c in cols], axis=1).reshape(-1)
    table = np.stack([a.astype(np.uint32), flat(pages.p_ins), flat(pages.p_outs)], axis=1)
    S = np.unique(a >> 3)
    counts, sections = [], [nodes[L + S].reshape(-1)]
    for k in range(h):
        clean = (S ^ 1)[~np.isin(S ^ 1, S)]
        counts.append(clean.size)
        sections.append(nodes[(L >> k) + clean].reshape(-1))
        S = np.unique(S >> 1)
    header = np.array([PROOF_MAGIC, W, a.size, sections[0].size // 8, h] + counts, dtype=np.uint32)
    return np.concatenate([header, table.reshape(-1)] + sections).astype(np.uint32)


def _digest_hex(d) -> str:
    return " ".join(f"{int(w):08x}" for w in d)


def check_page_out_proof(proof, root_before, keep=None) -> np.ndarray:
    """zkh_image_proof_verify in numpy, one `_hash_pairs` batch per layer: the walk from a ZKU1 proof and root_before to root_after (8
    words), with nothing else in hand.  Raises ReferenceError with the C verifier's message (after its "image_proof_verify: ").
    keep: a list that takes, per layer k = 1 .. h, (the heap ids of the layer's dirty nodes, their children as the walk hashes them: left
    old, left new, right old, right new, 8 words each): what `reference_page_out_nodes` lays out."""
    pf = np.asarray(proof, dtype=np.uint32).reshape(-1)
    rb = np.asarray(root_before, dtype=np.uint32).reshape(-1)
    if pf.size < PROOF_HEADER:
        raise ReferenceError(f"a proof of {pf.size} words: the header alone has {PROOF_HEADER}")
    magic, W, D, M, h = (int(x) for x in pf[:PROOF_HEADER])
    if magic != PROOF_MAGIC:
        raise ReferenceError(f"bad magic 0x{magic:08x} (ZKU1 is 0x{PROOF_MAGIC:08x})")
    if h != _tree_height(W):
        raise ReferenceError(f"h {h}, but an image of {W} words has h {_tree_height(W)}")
    if pf.size < PROOF_HEADER + h:
        raise ReferenceError(f"a proof of {pf.size} words, but the header describes at least {PROOF_HEADER + h}")
    c = [int(x) for x in pf[PROOF_HEADER:PROOF_HEADER + h]]
    want = PROOF_HEADER + h + 3 * D + 8 * M + 8 * sum(c)
    if pf.size != want:
        raise ReferenceError(f"a proof of {pf.size} words, but the header describes {want}")
    t0 = PROOF_HEADER + h
    l0 = t0 + 3 * D
    s0 = l0 + 8 * M
    table = pf[t0:l0].reshape(-1, 3)
    unreduced = pf >= P
    unreduced[:t0] = False
    unreduced[t0:l0:3] = False                                               # the addresses are integers
    if unreduced.any():
        at = int(np.argmax(unreduced))
        raise ReferenceError(f"word {at} is {int(pf[at])}, not below P")
    if rb.size != 8 or (rb >= P).any():
        raise ReferenceError("root_before is not 8 words below P")
    if D == 0:
        if M:
            raise ReferenceError(f"M {M}, but the table's rows lie in 0 leaves")
        for k in range(h):
            if c[k]:
                raise ReferenceError(f"layer {k}: {c[k]} siblings, but the walk takes 0")
        return rb.copy()
    a = table[:, 0].astype(np.int64)
    below = np.concatenate([[-1], a[:-1]])
    bad = (a >= W) | (a <= below)
    if bad.any():
        r = int(np.argmax(bad))
        if a[r] >= W:
            raise ReferenceError(f"row {r}: address {int(a[r])} outside the image of {W} words")
        raise ReferenceError(f"row {r}: address {int(a[r])} does not follow a smaller one (row {r - 1}: address {int(below[r])})")
    S, rank = np.unique(a >> 3, return_inverse=True)
    if S.size != M:
        raise ReferenceError(f"M {M}, but the table's rows lie in {S.size} leaves")
    old = pf[l0:s0].reshape(-1, 8).copy()
    held = old[rank, a & 7]
    if (held != table[:, 1]).any():
        r = int(np.argmax(held != table[:, 1]))
        raise ReferenceError(f"row {r}: in {int(table[r, 1])} at address {int(a[r])}, but its leaf holds {int(held[r])}")
    new = old.copy()
    new[rank, a & 7] = table[:, 2]
    at = s0
    for k in range(h):
        m = S.size
        nxt = np.concatenate([S[1:], [-1]])
        prv = np.concatenate([[-1], S[:-1]])
        first = (S & 1 == 0) & (nxt == S + 1)                                # an even node whose sibling is the next item
        second = (S & 1 == 1) & (prv == S - 1)
        lone = ~(first | second)
        take = int(lone.sum())
        if take != c[k]:
            raise ReferenceError(f"layer {k}: {c[k]} siblings, but the walk takes {take}")
        sib = pf[at:at + 8 * take].reshape(-1, 8)
        at += 8 * take
        heads = ~second
        parents = int(heads.sum())
        lo, ln, ro, rn = (np.zeros((parents, 8), dtype=np.uint32) for _ in range(4))
        slot = np.cumsum(heads) - 1                                          # the parent's rank of every item
        left, right = S & 1 == 0, S & 1 == 1
        lo[slot[left]], ln[slot[left]] = old[left], new[left]
        ro[slot[right]], rn[slot[right]] = old[right], new[right]
        lone_left = lone & left                                              # the node is the left child: its sibling goes right
        ro[slot[lone_left]] = rn[slot[lone_left]] = sib[(np.cumsum(lone) - 1)[lone_left]]
        lone_right = lone & right
        lo[slot[lone_right]] = ln[slot[lone_right]] = sib[(np.cumsum(lone) - 1)[lone_right]]
        both = _hash_pairs(np.concatenate([lo, ln]), np.concatenate([ro, rn]))
        old, new = both[:parents], both[parents:]
        S = S[heads] >> 1
        if keep is not None:
            keep.append(((image_tree_leaves(W) >> (k + 1)) + S, np.concatenate([lo, ln, ro, rn], axis=1)))
    if not np.array_equal(old[0], rb):
        raise ReferenceError(f"the proof opens root {_digest_hex(old[0])}, not root_before")
    return new[0].copy()


NODES_MAGIC = 0x5A4B4E31                                                     # 'ZKN1'
NODES_HEADER = 4


def image_dirty_words(image_words: int, pages: int) -> int:
    """zkh_image_dirty_words: the bound 4 + h + 33 sum_{k=1..h} min(D, L >> k) on the words of the dirty-node table of a page-out of D
    rows over an image of W words (a row dirties one node per layer); 0 for W = 0"""
    W, D = int(image_words), int(pages)
    if not W:
        return 0
    L = image_tree_leaves(W)
    return NODES_HEADER + _tree_height(W) + 33 * sum(min(D, L >> k) for k in range(1, _tree_height(W) + 1))


def reference_page_out_nodes(proof, root_before) -> Tuple[np.ndarray, np.ndarray]:
    """The dirty-node table zkh_image_proof_nodes writes (include/zkhal.h "THE UPDATE'S PROOF"; csrc/zkn1.h), word for word, from a ZKU1
    proof and root_before alone -> (root_after, the table).  Words: 'ZKN1', W, D, h, n_1 .. n_h; then per layer k = 1 .. h (layer 0 the
    leaves, layer h the root) the n_k heap ids of the layer's dirty nodes, increasing, and n_k records of 32 words: the node's left child
    old ‖ new, its right child old ‖ new, as the walk of `check_page_out_proof` hashes them (a clean child is the proof's sibling,
    old = new; a layer-1 node's children are two leaves).  Raises ReferenceError as check_page_out_proof does, and on D = 0."""
    pf = np.asarray(proof, dtype=np.uint32).reshape(-1)
    keep = []
    root_after = check_page_out_proof(pf, root_before, keep)
    W, D, h = int(pf[1]), int(pf[2]), int(pf[4])
    if D == 0:
        raise ReferenceError("an empty table (D = 0) has no dirty nodes: its proof is the header alone and holds no node, not even the root's children; "
                             "such a page-out is sealed from the tree (zkh_page_tree_witgen)")
    header = np.array([NODES_MAGIC, W, D, h] + [ids.size for ids, _ in keep], dtype=np.uint32)
    return root_after, np.concatenate([header] + [part.reshape(-1) for ids, records in keep for part in (ids, records)]).astype(np.uint32)


def bus_slots(A: int, distinct_keys: int) -> int:
    """the size zkh_check_bus's key table ends at: the smallest power of two >= max(64, 2 A), doubled until it is at least twice the
    number of distinct keys (the table holds one slot per key and stays at most half full)"""
    slots = 64
    while slots < 2 * A:
        slots <<= 1
    while 2 * distinct_keys > slots:
        slots <<= 1
    return slots


def reference_bus(args: Arguments, po2: int, zk_cycles: int, code, data) -> dict:
    """CHECK BUS (DESIGN.md §2 ARGUMENTS), the definition zkh_check_bus computes on the device: which key of the bus does not balance.
    No mix, no accum.  An entry is a (term i, row r < A) of non-zero weight w_i(r) = sel_i(r) m_i(r) in Fp (residues; absent = 1: the
    numerator of the accumulate); its key is (tag, v_0 .. v_3), canonical, the tuple zero-padded (`_canonical_key`); net(K) = the sum of
    sign_i w_i(r) over the entries of K in Fp, and K is unbalanced when net(K) != 0.  Distinct keys are distinct poles, so the bus
    balances for every mix exactly when every net is 0.  The representative of a key is its entry of smallest (blob term index, row),
    over all terms; the unbalanced key of smallest representative is the one reported.
    -> {"term", "row": that representative (-1, -1: every key balances; tag, key, net are then 0), "tag", "key": 4 canonical words,
    "net", "unbalanced_keys", "distinct_keys", "slots" (`bus_slots`), "per_term": an (n_terms, 4) int64 array, per blob term the
    (count, first_row, last_row, weight) of its entries of the reported key, weight their sum of w_i(r) in Fp, unsigned; (0, -1, -1, 0)
    for a term without one} — the dict of HipHal.check_bus(per_term=True)."""
    n = 1 << po2
    A = n - zk_cycles
    terms = Arguments.parse(args.blob()).terms                               # blob order: the term index of the representative rule
    groups = {GROUP_CODE: np.asarray(code, dtype=np.uint32).reshape(-1, n), GROUP_DATA: np.asarray(data, dtype=np.uint32).reshape(-1, n)}
    rows = np.arange(A)
    keys, who, weight, sign = [], [], [], []
    for i, t in enumerate(terms):
        if args.open is not None and t.tag % P == args.open.tag:              # another seal answers the open tag: its keys are no part of this check
            continue
        w = np.ones(A, dtype=np.uint64)
        if t.sel is not None:
            w = _m(w, _dec(groups[GROUP_CODE][t.sel, :A]))
        if t.mult is not None:
            w = _m(w, _dec(groups[t.mult[0]][t.mult[1], :A]))
        live = rows[w != 0]
        keys.append(_canonical_key(terms, groups, i, live))
        who.append((np.uint64(i) << np.uint64(32)) | live.astype(np.uint64))
        weight.append(w[live])
        sign.append(np.full(live.size, t.sign == -1))
    keys, who, weight, neg = np.concatenate(keys), np.concatenate(who), np.concatenate(weight), np.concatenate(sign)
    per_term = np.zeros((len(terms), 4), dtype=np.int64)
    per_term[:, 1:3] = -1
    out = {"term": -1, "row": -1, "tag": 0, "key": (0, 0, 0, 0), "net": 0, "unbalanced_keys": 0, "distinct_keys": 0,
           "slots": bus_slots(A, 0), "per_term": per_term}
    if not len(keys):
        return out
    uk, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    total = np.zeros((2, len(uk)), dtype=np.uint64)                          # at most n_terms * A < 2^33 adds below 2^31: no wrap
    np.add.at(total[0], inv[~neg], weight[~neg])
    np.add.at(total[1], inv[neg], weight[neg])
    net = (total[0] % np.uint64(P) + np.uint64(P) - total[1] % np.uint64(P)) % np.uint64(P)
    rep = np.full(len(uk), np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(rep, inv, who)
    bad = np.nonzero(net != 0)[0]
    out.update(distinct_keys=len(uk), unbalanced_keys=len(bad), slots=bus_slots(A, len(uk)))
    if not len(bad):
        return out
    k = int(bad[np.argmin(rep[bad])])
    out.update(term=int(rep[k]) >> 32, row=int(rep[k]) & 0xFFFFFFFF, tag=int(uk[k, 0]), key=tuple(int(x) for x in uk[k, 1:]), net=int(net[k]))
    mine = inv == k
    for i in np.unique(who[mine] >> np.uint64(32)):
        of = mine & (who >> np.uint64(32) == i)
        r = (who[of] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        per_term[int(i)] = (r.size, r.min(), r.max(), int(weight[of].sum() % np.uint64(P)))
    return out


BUS_LINE_TERMS = 8
TIE_TAG = 2                                     # the tag of a table row (addr, in, out) on the bus across a paging segment's seal and its page-out chain


def _f4_mul(x, y):
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += x[i] * y[j]
    return [(c[i] + (c[i + 4] * NBETA if i < 3 else 0)) % P for i in range(4)]


def _f4_inv(a):
    """1 / a in Fp4 = Fp[x] / (x^4 + 11): a * a' lies in Fp[x^2] for a'(x) = a(-x), and that quadratic element is inverted by its norm"""
    conj = [a[0], -a[1] % P, a[2], -a[3] % P]
    q = _f4_mul(a, conj)                                                     # (q0, 0, q2, 0)
    norm = (q[0] * q[0] + 11 * q[2] * q[2]) % P
    inv = pow(norm, P - 2, P)
    return _f4_mul(conj, [q[0] * inv % P, 0, -q[2] * inv % P, 0])


def table_fingerprint(table, alpha, beta, tag: int = TIE_TAG) -> np.ndarray:
    """THE TABLE'S FINGERPRINT (zkh_table_fingerprint): sum_i 1 / (alpha - (tag + beta a_i + beta^2 in_i + beta^3 out_i)) in Fp4 over the rows
    (a_i, in_i, out_i) of a page table, in plain Python integers.  table: rows as a ZKU1 proof holds them, the address an integer, in and
    out Montgomery words; alpha, beta: 4 Montgomery words each, as `out` holds them.  -> the sum as 4 Montgomery words.  It is what the
    open total of a tied paging segment must be, and minus what the totals of its page-out parts add up to.  Raises ReferenceError,
    naming the lowest row, on a denominator that vanishes."""
    dec = lambda w: int(w) % P * _RINV % P
    al, be = [dec(w) for w in alpha], [dec(w) for w in beta]
    b2 = _f4_mul(be, be)
    b3 = _f4_mul(b2, be)
    total = [0, 0, 0, 0]
    for i, (a, w_in, w_out) in enumerate(np.asarray(table, dtype=np.uint64).reshape(-1, 3).tolist()):
        a, vi, vo = a % P, dec(w_in), dec(w_out)
        den = [(al[e] - (be[e] * a + b2[e] * vi + b3[e] * vo) - (tag % P if e == 0 else 0)) % P for e in range(4)]
        if not any(den):
            raise ReferenceError(f"table_fingerprint: the denominator of row {i} vanishes")
        inv = _f4_inv(den)
        total = [(total[e] + inv[e]) % P for e in range(4)]
    return np.asarray([t * _R % P for t in total], dtype=np.uint32)


def describe_bus(bus: dict, args: Arguments) -> Optional[str]:
    """the one line that words what `reference_bus` / HipHal.check_bus(per_term=True) found, None when every key balances:

        bus: key (tag T; v0, v1, v2, v3) does not balance, net N: term i (+, sel code[c], m data[c]) has k entries, rows r0..r1, weight
        w; term j (−, …) has none; U of D keys do not balance

    The terms are those of the key's tag, blob indices: first the ones that hold entries of the key, the sign with fewer holders first
    (a table before its many lookups), then the ones that hold none and whose sign no holder has (the side that is missing: the table
    that never held the value, the store that never happened), then the other ones that hold none; each group in blob order; at most
    BUS_LINE_TERMS terms, then "… and m more"."""
    if bus["row"] < 0:
        return None
    terms = Arguments.parse(args.blob()).terms
    table = bus["per_term"]
    same = [i for i, t in enumerate(terms) if t.tag % P == bus["tag"]]
    holders = [i for i in same if table[i][0]]
    signs = {terms[i].sign for i in holders}
    of_sign = {sg: sum(terms[j].sign == sg for j in holders) for sg in signs}
    holders.sort(key=lambda i: (of_sign[terms[i].sign], i))
    order = holders + [i for i in same if not table[i][0] and terms[i].sign not in signs] + \
        [i for i in same if not table[i][0] and terms[i].sign in signs]
    group = {GROUP_CODE: "code", GROUP_DATA: "data"}
    parts = []
    for i in order[:BUS_LINE_TERMS]:
        t = terms[i]
        what = ["+" if t.sign == 1 else "−"] + ([f"sel code[{t.sel}]"] if t.sel is not None else []) + \
            ([f"m {group[t.mult[0]]}[{t.mult[1]}]"] if t.mult is not None else [])
        count, first, last, weight = (int(x) for x in table[i])
        has = f"has {count} entr{'y' if count == 1 else 'ies'}, rows {first}..{last}, weight {weight}" if count else "has none"
        parts.append(f"term {i} ({', '.join(what)}) {has}")
    if len(order) > BUS_LINE_TERMS:
        parts.append(f"… and {len(order) - BUS_LINE_TERMS} more")
    key = ", ".join(str(x) for x in bus["key"])
    return (f"bus: key (tag {bus['tag']}; {key}) does not balance, net {bus['net']}: " + "; ".join(parts) +
            f"; {bus['unbalanced_keys']} of {bus['distinct_keys']} keys do not balance")
