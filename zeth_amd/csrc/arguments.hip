// arguments.hip — the ZKA1 argument blob (layout: zeth_amd/circuits/logup.py; DESIGN.md §2 ARGUMENTS): its decoding into
// zkh::Arguments (terms, from version 4 derived-column records, from version 5 LINK records, from version 6 their read rule, from version 7 the PAGES
// record, from version 8 the OPEN record, from version 9 the ports of a memory: LINK records that join a head, from version 10 a PAGES record of two value words per address, from version 11 its flat-address destinations), the rules a circuit's arguments keep (check_sorted, check_derived, then check_owned over the LIMBS / ORDER records, over the LINK records
// and over the PAGES record), and the entry points that attach them to a circuit and ask what they derive.
// decode_arguments is the only code that knows the blob's words; everything else, here and in the consumers, reads decoded terms.
#include "arguments.h"

#include <algorithm>

using namespace zkh;

namespace {

// Term word 7, the flags.  Version 1 leaves it unread.  Version 2: bit 0 = "multiplicity derived by the library"
// (zkh_derive_multiplicities); every other bit is reserved.  Version 3 adds bit 1 = "this term D is a sorted copy derived by the
// library" (zkh_derive_sorted) of its source term S (bits 16..31), by nkeys (bits 4..6) tuple positions (2 bits each from bit 8, most
// significant key first); bits 2, 3, 7, the position fields of unused keys and, without bit 1, everything above bit 0 are reserved.
// A reserved bit is recorded, not refused: the rules refuse it where they reach the term (flag_word_rule), after the circuit-shape checks.
const char* decode_arguments(const uint32_t* a, size_t words, Arguments* out) {
    ZKH_REQUIRE(words >= ARGS_HEADER && a[0] == ARGS_MAGIC && a[1] >= 1 && a[1] <= 11 && (a[1] != 6 || a[7] != 0) && (a[1] != 7 || (a[7] & PAGES_BIT)) && (a[1] != 8 || (a[7] & OPEN_BIT)) &&
                (a[1] != 9 || (a[7] & PORTS_BIT)) && (a[1] != 10 || (a[7] & WIDE_BIT)) && (a[1] != 11 || (a[7] & FLAT_BIT)),
                "set_arguments: not a ZKA1 (version 1) argument blob");
    const uint32_t n_terms = a[5], n_records = a[1] >= 4 ? a[6] : 0;            // header word 6: the records of version 4, reserved before
    const size_t rec0 = ARGS_HEADER + (size_t)TERM_WORDS * n_terms;
    size_t end = rec0;                                                          // a LINK record (version 5) takes two slots; past the blob's end the walk stops
    for (uint32_t i = 0; i < n_records && end <= words; i++)                    // ... and so does the PAGES record (version 7)
        end += end < words && ((a[1] >= 5 && a[end] == KIND_LINK) || (a[1] >= 7 && a[end] == KIND_PAGES)) ? LINK_WORDS : RECORD_WORDS;
    const bool fits = words == end;
    ZKH_REQUIRE(fits || a[1] < 4, "set_arguments: %zu words for %u terms and %u records", words, n_terms, n_records);
    ZKH_REQUIRE(fits, "set_arguments: %zu words for %u terms", words, n_terms);
    out->version = a[1]; out->k = a[2]; out->alpha = a[3]; out->beta = a[4];
    out->terms.assign(n_terms, Term{});
    for (uint32_t i = 0; i < n_terms; i++) {
        const uint32_t* r = a + ARGS_HEADER + (size_t)TERM_WORDS * i;
        Term& t = out->terms[i];
        t.col = r[0]; t.neg = r[1]; t.sel = r[2]; t.mg = r[3]; t.mc = r[4]; t.tag = r[5]; t.w = r[6];
        for (uint32_t e = 0; e < MAX_TUPLE; e++) { t.tg[e] = r[8 + 2 * e]; t.tc[e] = r[9 + 2 * e]; }
        const uint32_t f = t.flags = out->version >= 2 ? r[7] : 0;
        t.derive = f & 1;
        t.reserved = f > 1;
        if (out->version >= 3) {
            t.sorted = f & 2;
            t.sorted_from = f >> 16;
            t.nkeys = (f >> 4) & 7;
            for (uint32_t j = 0; j < 4; j++) t.key[j] = (f >> (8 + 2 * j)) & 3;
            t.reserved = (f & 0x8c) || (!t.sorted && f > 1);
            for (uint32_t j = t.nkeys; j < 4; j++) t.reserved |= t.key[j] != 0;
        }
    }
    // Derived-column records (version 4): kind, L, nl, n_src, two (group, column) source pairs, eight destination data columns.  As
    // with the flags, a reserved word that is set is recorded here and refused by the rules (columns_clause_a).
    // LINK records (version 5, kind 3, 32 words): L, nl, nc, sel, 0, the key's (group, column), three carried (group, column) pairs, 0, 0,
    // then from word 16 the destinations linked, last, prev_0 .. prev_{nc-1}, limb_0 .. limb_{nl-1}, the rest 0 (links_clause_a).
    // Version 6: word 5 is a flag word (bit 0 = READS), words 14, 15 the write flag's (group, column) with READS and 0 without; header
    // word 7 counts the records with READS (0 there is no ZKA1 blob: above).
    // The PAGES record (version 7, kind 4, 32 words): L, ng, the blob index of its LINK, words 4 .. 15 reserved, then from word 16 the
    // destinations p_on, p_addr, p_in, p_out, p_time, alimb_0 .. alimb_{ng-1}, gap_0 .. gap_{ng-1}, the rest 0 (pages_clause_a).  Header
    // word 7 carries bit 16 beside the READS count.
    // The OPEN record (version 8, kind 5, 16 words), after every other record: the open tag, the `out` offsets of alpha, beta and the total, the
    // circuit's `out` words, words 6 .. 15 reserved (open_rule).  Header words 3, 4 repeat alpha and beta; header word 7 carries bit 17 beside
    // the READS count and, exactly when the blob holds a PAGES record, bit 16.
    // WIDE (version 10): PAGES word 4 holds V - 1 (reserved = 0 before), the record has 3 + 2 V + 2 ng destinations p_on, p_addr, p_in_0 ..,
    // p_out_0 .., p_time, alimb_*, gap_*, and header word 7 carries bit 19 exactly when V = 2 (bits 16, 17, 18 exactly when the blob holds
    // a PAGES record, an OPEN record, a LINK that joins).
    // FLAT (version 11): PAGES word 5 holds F, the number of flat-address destinations (0 or 2, and 2 only with V = 2; reserved = 0 before),
    // words 6, 7 the data columns p_flat_0, p_flat_1 (0 when F = 0), words 8 .. 15 stay reserved; header word 7 carries bit 20 exactly when
    // F = 2 (bits 16 .. 19 exactly when the blob holds what they name).
    out->records.clear();
    out->links.clear();
    out->heads.clear();
    out->pages.clear();
    out->open.clear();
    const uint32_t* r = a + rec0;
    for (uint32_t i = 0; i < n_records; i++) {
        if (!out->open.empty() && out->after_open == NONE) { out->after_open = i; out->second_open = r[0] == KIND_OPEN; }
        if (out->version >= 8 && r[0] == KIND_OPEN) {
            Open x{};
            x.index = i; x.tag = r[1]; x.alpha = r[2]; x.beta = r[3]; x.total = r[4]; x.out_words = r[5];
            for (uint32_t j = 6; j < OPEN_WORDS; j++) x.reserved |= r[j];
            out->open.push_back(x);
            r += OPEN_WORDS;
            continue;
        }
        if (!out->pages.empty() && out->after_pages == NONE) { out->after_pages = i; out->second_pages = out->version >= 7 && r[0] == KIND_PAGES; }
        if (out->version >= 7 && r[0] == KIND_PAGES) {
            Pages x{};
            x.index = i; x.L = r[1]; x.ng = r[2]; x.link = r[3];
            x.word4 = r[4];                             // version 10: V - 1; reserved before
            x.V = out->version >= 10 ? 1 + (r[4] < MAX_PAGE_WORDS - 1 ? r[4] : MAX_PAGE_WORDS - 1) : 1;
            const uint32_t nd = 3 + 2 * x.V + 2 * (x.ng < 8 ? x.ng : 8);
            x.n_dst = nd < MAX_PAGE_DSTS ? nd : MAX_PAGE_DSTS;
            for (uint32_t j = 0; j < x.n_dst; j++) x.dst[j] = r[16 + j];
            x.word5 = out->version >= 11 ? r[5] : 0;    // version 11: F; reserved before
            x.F = x.word5 == MAX_PAGE_FLATS ? MAX_PAGE_FLATS : 0;
            for (uint32_t j = 0; j < x.F; j++) x.flat[j] = r[6 + j];
            for (uint32_t j = out->version >= 11 ? 6 + x.F : out->version >= 10 ? 5 : 4; j < 16; j++) x.reserved |= r[j];
            for (uint32_t j = 16 + (nd < 16 ? nd : 16); j < PAGES_WORDS; j++) x.reserved |= r[j];
            out->pages.push_back(x);
            r += PAGES_WORDS;
            continue;
        }
        if (out->version >= 5 && r[0] == KIND_LINK) {
            Link x{};
            x.index = i; x.L = r[1]; x.nl = r[2]; x.nc = r[3]; x.sel = r[4]; x.kg = r[6]; x.kc = r[7];
            for (uint32_t j = 0; j < MAX_CARRIED; j++) { x.cg[j] = r[8 + 2 * j]; x.cc[j] = r[9 + 2 * j]; }
            for (uint32_t j = 0; j < MAX_LINK_DSTS; j++) x.dst[j] = r[16 + j];
            const uint32_t nc = x.nc < MAX_CARRIED ? x.nc : MAX_CARRIED;
            const uint64_t nd = 2ull + nc + x.nl;
            x.n_dst = nd < MAX_LINK_DSTS ? (uint32_t)nd : MAX_LINK_DSTS;
            if (out->version >= 6) { x.flags = r[5]; x.wg = r[14]; x.wc = r[15]; }
            else x.reserved = r[5] | r[14] | r[15];
            out->reads += x.flags & LINK_READS;
            for (uint32_t j = nc; j < MAX_CARRIED; j++) x.reserved |= x.cg[j] | x.cc[j];
            const bool joins = out->version >= 9 && (x.flags & LINK_JOINS);      // version 9: bit 1 of word 5, and word 31 names the head
            for (uint32_t j = 16 + x.n_dst; j < LINK_WORDS - (joins ? 1 : 0); j++) x.reserved |= r[j];
            out->links.push_back(x);
            out->heads.push_back(joins ? r[LINK_WORDS - 1] : NONE);
            r += LINK_WORDS;
            continue;
        }
        if (!out->links.empty() && out->late_record == NONE) { out->late_record = i; out->late_after = out->links[0].index; }
        Record x{};
        x.kind = r[0]; x.L = r[1]; x.nl = r[2]; x.n_src = r[3];
        for (uint32_t j = 0; j < 2; j++) { x.sg[j] = r[4 + 2 * j]; x.sc[j] = r[5 + 2 * j]; }
        for (uint32_t j = 0; j < MAX_LIMBS; j++) x.dst[j] = r[8 + j];
        const uint64_t nd = (uint64_t)x.nl + (x.kind == KIND_ORDER && x.n_src == 2);
        x.n_dst = nd < MAX_LIMBS ? (uint32_t)nd : MAX_LIMBS;
        for (uint32_t j = x.n_src < 2 ? x.n_src : 2; j < 2; j++) x.reserved |= x.sg[j] | x.sc[j];
        for (uint32_t j = x.n_dst; j < MAX_LIMBS; j++) x.reserved |= x.dst[j];
        out->records.push_back(x);
        r += RECORD_WORDS;
    }
    const bool paged = out->version == 7 || (out->version >= 8 && (a[7] & PAGES_BIT));
    const bool opened = out->version == 8 || (out->version >= 9 && (a[7] & OPEN_BIT));
    const bool ported = out->version == 9 || (out->version >= 10 && (a[7] & PORTS_BIT));
    const bool widened = out->version == 10 || (out->version >= 11 && (a[7] & WIDE_BIT));
    // bit 16 says PAGES, bit 17 OPEN, bit 18 (version 9) PORTS, bit 19 (version 10) WIDE, bit 20 (version 11) FLAT, the rest counts as before
    const uint32_t word7 = (paged ? a[7] ^ PAGES_BIT : a[7]) ^ (opened ? OPEN_BIT : 0) ^ (ported ? PORTS_BIT : 0) ^ (widened ? WIDE_BIT : 0) ^ (out->version >= 11 ? FLAT_BIT : 0);
    ZKH_REQUIRE(out->version < 6 || word7 == out->reads, "set_arguments: header word 7 is %u, the blob has %u LINK records with READS", word7, out->reads);
    ZKH_REQUIRE(!paged || !out->pages.empty(), "set_arguments: header word 7 has bit 16 (PAGES), but the blob has no PAGES record");
    ZKH_REQUIRE(out->version < 8 || paged || out->pages.empty(), "set_arguments: the blob has a PAGES record, but header word 7 lacks bit 16 (PAGES)");
    ZKH_REQUIRE(!opened || !out->open.empty(), "set_arguments: header word 7 has bit 17 (OPEN), but the blob has no OPEN record");
    ZKH_REQUIRE(out->version < 9 || opened || out->open.empty(), "set_arguments: the blob has an OPEN record, but header word 7 lacks bit 17 (OPEN)");
    ZKH_REQUIRE(!ported || out->ports(), "set_arguments: header word 7 has bit 18 (PORTS), but no LINK record joins");
    ZKH_REQUIRE(out->version < 10 || ported || !out->ports(), "set_arguments: a LINK record joins, but header word 7 lacks bit 18 (PORTS)");
    const bool two = std::any_of(out->pages.begin(), out->pages.end(), [](const Pages& g) { return g.word4 != 0; });
    ZKH_REQUIRE(!widened || two, "set_arguments: header word 7 has bit 19 (WIDE), but no PAGES record pages two value words per address");
    ZKH_REQUIRE(out->version < 11 || widened || !two, "set_arguments: a PAGES record pages two value words per address, but header word 7 lacks bit 19 (WIDE)");
    ZKH_REQUIRE(out->version < 11 || std::any_of(out->pages.begin(), out->pages.end(), [](const Pages& g) { return g.word5 != 0; }),
                "set_arguments: header word 7 has bit 20 (FLAT), but no PAGES record has flat-address destinations");
    return nullptr;
}

const char* flag_word_rule(const Arguments& a, uint32_t i) {
    const Term& t = a.terms[i];
    if (!t.reserved) return nullptr;
    if (a.version >= 3)
        return make_err("set_arguments: term %u: word 7 is %#x (bit 0: derived multiplicity; bit 1: sorted copy, with its keys in bits 4..15 "
                        "and its source term in bits 16..31; the other bits are reserved)", i, t.flags);
    return make_err("set_arguments: term %u: word 7 is %u (bit 0: derived multiplicity; the other bits are reserved)", i, t.flags);
}

bool in_tuple(const Term& t, uint32_t width, uint32_t g, uint32_t col) {       // (g, col) among the first `width` tuple columns of t
    for (uint32_t e = 0; e < width; e++)
        if (t.tg[e] == g && t.tc[e] == col) return true;
    return false;
}

// logup.check_derived: the first derived term that breaks a rule.  A derived term is (a) of sign -1, (b) with a data-group
// multiplicity column (c) that no tuple and no other term's multiplicity names, and (d) every other term of its tag is a lookup of
// sign +1.
const char* check_derived(const Arguments& a) {
    const uint32_t n_terms = (uint32_t)a.terms.size();
    for (uint32_t i = 0; i < n_terms; i++) {
        const Term& t = a.terms[i];
        ZKH_TRY(flag_word_rule(a, i));
        if (!t.derive) continue;
        ZKH_REQUIRE(t.neg == 1, "set_arguments: term %u: a derived multiplicity needs sign -1 (the table side of a lookup)", i);
        ZKH_REQUIRE(t.mg == GROUP_DATA, "set_arguments: term %u: a derived multiplicity must be a data-group column", i);
        for (uint32_t j = 0; j < n_terms; j++) {
            const Term& u = a.terms[j];
            ZKH_REQUIRE(j == i || !(u.mg == GROUP_DATA && u.mc == t.mc), "set_arguments: term %u: its derived multiplicity column (data %u) is "
                        "also the multiplicity of term %u", i, t.mc, j);
            ZKH_REQUIRE(!in_tuple(u, u.w, GROUP_DATA, t.mc), "set_arguments: term %u: its derived multiplicity column (data %u) is read by the "
                        "tuple of term %u", i, t.mc, j);
            ZKH_REQUIRE(u.tag != t.tag || u.derive || u.neg == 0, "set_arguments: term %u: term %u of its tag %u has sign -1 and is not derived "
                        "(the lookups of a derived tag have sign +1)", i, j, t.tag);
        }
    }
    return nullptr;
}

// logup.check_sorted: the first sorted-copy term D that breaks a rule.  With S its source: (a) D has sign -1 and no derived
// multiplicity, S is another term of sign +1 without a flag and the source of no other copy; (b) the same tag, tuple width and
// selector, both multiplicities the constant 1; (c) D's tuple columns are pairwise distinct data columns that no other tuple and no
// multiplicity names; (d) 1..3 key positions, distinct and below the width; (e) no derived multiplicity in D's tag.
const char* check_sorted(const Arguments& a) {
    const uint32_t n_terms = (uint32_t)a.terms.size();
    for (uint32_t i = 0; i < n_terms; i++) {
        const Term& t = a.terms[i];
        ZKH_TRY(flag_word_rule(a, i));
        if (!t.sorted) continue;
        const uint32_t s = t.sorted_from, w = t.w;
        ZKH_REQUIRE(t.neg == 1, "set_arguments: term %u: a sorted copy needs sign -1 (the permuted side of a multiset equality)", i);
        ZKH_REQUIRE(!t.derive, "set_arguments: term %u: a sorted copy cannot also have a derived multiplicity", i);
        ZKH_REQUIRE(s != i && s < n_terms, "set_arguments: term %u: its source term %u is not another term of the arguments", i, s);
        const Term& u = a.terms[s];
        ZKH_REQUIRE(u.neg == 0, "set_arguments: term %u: its source term %u needs sign +1", i, s);
        ZKH_REQUIRE(u.flags == 0, "set_arguments: term %u: its source term %u is itself derived or a sorted copy", i, s);
        for (uint32_t j = 0; j < n_terms; j++)
            ZKH_REQUIRE(j == i || !a.terms[j].sorted || a.terms[j].sorted_from != s, "set_arguments: term %u: its source term %u is also the "
                        "source of term %u", i, s, j);
        ZKH_REQUIRE(u.tag == t.tag && u.w == w && u.sel == t.sel, "set_arguments: term %u: its source term %u has another tag, tuple width or selector", i, s);
        ZKH_REQUIRE(t.mg == NONE && u.mg == NONE, "set_arguments: term %u: a sorted copy and its source term %u have the constant multiplicity 1", i, s);
        for (uint32_t e = 0; e < w; e++) {
            const uint32_t g = t.tg[e], col = t.tc[e];
            ZKH_REQUIRE(g == GROUP_DATA, "set_arguments: term %u: tuple column (%u, %u) of a sorted copy must be a data-group column", i, g, col);
            ZKH_REQUIRE(!in_tuple(t, e, g, col), "set_arguments: term %u: its sorted column (data %u) appears twice in its tuple", i, col);
            for (uint32_t j = 0; j < n_terms; j++) {
                const Term& x = a.terms[j];
                ZKH_REQUIRE(j == i || !in_tuple(x, x.w, g, col), "set_arguments: term %u: its sorted column (data %u) is read by the tuple of "
                            "term %u", i, col, j);
                ZKH_REQUIRE(!(x.mg == g && x.mc == col), "set_arguments: term %u: its sorted column (data %u) is the multiplicity of term %u", i, col, j);
            }
        }
        const uint32_t kmax = w < MAX_SORT_KEYS ? w : MAX_SORT_KEYS;
        ZKH_REQUIRE(t.nkeys >= 1 && t.nkeys <= kmax, "set_arguments: term %u: %u sort keys (1..%u: at most %u, and no more than the tuple width %u)", i,
                    t.nkeys, kmax, MAX_SORT_KEYS, w);
        for (uint32_t j = 0; j < t.nkeys; j++) {
            bool ok = t.key[j] < w;
            for (uint32_t j2 = 0; j2 < j; j2++) ok &= t.key[j2] != t.key[j];
            ZKH_REQUIRE(ok, "set_arguments: term %u: its sort key positions must be distinct and below the tuple width %u", i, w);
        }
        for (uint32_t j = 0; j < n_terms; j++)
            ZKH_REQUIRE(!(a.terms[j].derive && a.terms[j].tag == t.tag), "set_arguments: term %u: term %u of its tag %u has a derived multiplicity", i, j, t.tag);
    }
    return nullptr;
}

bool is_column(const zkh_circuit* c, uint32_t g, uint32_t col) { return (g == GROUP_CODE || g == GROUP_DATA) && col < c->group_size[g]; }

// A record of either kind as the ownership rule (arguments.h) sees it
struct Owned {
    uint32_t index;                                     // its index among the blob's records
    bool link;                                          // a LINK or the PAGES record: it runs after every LIMBS / ORDER record
    uint32_t n_src, sg[2 + MAX_CARRIED], sc[2 + MAX_CARRIED];   // the (group, column) pairs it reads (LINK: the key, the carried columns, with READS the write flag)
    uint32_t n_dst, dst[MAX_PAGE_DSTS + MAX_PAGE_FLATS];    // the data columns it writes (a PAGES record: its destinations, then its flats)
    uint32_t free;                                      // its first `free` destinations may be the multiplicity of a term that is not derived
    bool writes(uint32_t col) const { return std::find(dst, dst + n_dst, col) != dst + n_dst; }
    bool reads(uint32_t col) const {                    // data column `col` among its sources
        for (uint32_t s = 0; s < n_src; s++)
            if (sg[s] == GROUP_DATA && sc[s] == col) return true;
        return false;
    }
};
// the LINK that a PAGES record names, where it is one the rules allow: READS, a clock and V value columns
const Link* paged_link(const Arguments& a, const Pages& g) {
    for (const Link& r : a.links)
        if (r.index == g.link) return (r.flags & LINK_READS) && r.nc == 1 + g.V ? &r : nullptr;
    return nullptr;
}
static_assert(MAX_PAGE_DSTS >= MAX_LINK_DSTS && MAX_PAGE_DSTS >= MAX_LIMBS, "Owned::dst holds any record's destinations");
// the LIMBS / ORDER records, then the LINK records, then the PAGES record: the blob's order (a blob that has it otherwise is refused before anything reads this)
std::vector<Owned> owned(const Arguments& a) {
    std::vector<Owned> all;
    for (const Record& r : a.records) {
        Owned v{(uint32_t)all.size(), false, std::min(r.n_src, 2u), {}, {}, r.n_dst, {}, 0};
        std::copy(r.sg, r.sg + v.n_src, v.sg); std::copy(r.sc, r.sc + v.n_src, v.sc); std::copy(r.dst, r.dst + r.n_dst, v.dst);
        all.push_back(v);
    }
    for (const Link& r : a.links) {
        const uint32_t nc = std::min(r.nc, MAX_CARRIED);
        Owned v{r.index, true, 1 + nc, {r.kg}, {r.kc}, r.n_dst, {}, 2};
        std::copy(r.cg, r.cg + nc, v.sg + 1); std::copy(r.cc, r.cc + nc, v.sc + 1); std::copy(r.dst, r.dst + r.n_dst, v.dst);
        if (r.flags & LINK_READS) { v.sg[v.n_src] = r.wg; v.sc[v.n_src++] = r.wc; }
        all.push_back(v);
    }
    const size_t n_rec = a.records.size();
    for (const Pages& g : a.pages) {                    // it reads what its LINK reads
        Owned v{g.index, true, 0, {}, {}, g.n_dst, {}, 1};
        if (const Link* t = paged_link(a, g)) {
            const Owned& l = all[n_rec + (t - a.links.data())];
            v.n_src = l.n_src; std::copy(l.sg, l.sg + l.n_src, v.sg); std::copy(l.sc, l.sc + l.n_src, v.sc);
        }
        std::copy(g.dst, g.dst + g.n_dst, v.dst);
        std::copy(g.flat, g.flat + g.F, v.dst + g.n_dst);       // version 11: p_flat_j are destinations like the others
        v.n_dst += g.F;
        all.push_back(v);
    }
    return all;
}

// logup.check_columns' own clause (a): the ranges of kind, L, nl, n_src and the reserved words
const char* columns_clause_a(const Record& r, uint32_t i) {
    ZKH_REQUIRE(r.kind == KIND_LIMBS || r.kind == KIND_ORDER, "set_arguments: record %u: kind %u (1 = LIMBS, 2 = ORDER)", i, r.kind);
    ZKH_REQUIRE(r.L >= 1 && r.L <= 16 && r.nl >= 1 && r.nl <= MAX_LIMBS && r.L * r.nl <= 32, "set_arguments: record %u: %u limbs of %u bits "
                "(1..8 limbs of 1..16 bits, at most 32 bits in all)", i, r.nl, r.L);
    ZKH_REQUIRE(r.n_src >= 1 && r.n_src <= (r.kind == KIND_LIMBS ? 1u : 2u), "set_arguments: record %u: %u sources (LIMBS: 1; ORDER: 1 or 2)", i, r.n_src);
    ZKH_REQUIRE(r.n_src < 2 || r.nl <= MAX_LIMBS - 1, "set_arguments: record %u: an ORDER record with two keys has at most %u limbs (its flag column is "
                "the first destination)", i, MAX_LIMBS - 1);
    ZKH_REQUIRE(!r.reserved, "set_arguments: record %u: a reserved word is not 0 (the unused source pair and the unused destination words)", i);
    return nullptr;
}
// logup.check_links' own clause (a): the ranges of nc, L, nl, the flag word and the write flag's words (version 6), the reserved words, and the
// selector a code column
const char* links_clause_a(const zkh_circuit* c, const Arguments& a, const Link& r) {
    const uint32_t i = r.index;
    ZKH_REQUIRE(r.nc >= 1 && r.nc <= MAX_CARRIED && r.L >= 1 && r.L <= 16 && r.nl <= MAX_LINK_LIMBS && r.L * r.nl <= MAX_ORDER_BITS,
                "set_arguments: record %u: a LINK of %u carried columns and %u limbs of %u bits (1..%u carried columns, 0..%u limbs of 1..16 bits, at most "
                "%u bits in all)", i, r.nc, r.nl, r.L, MAX_CARRIED, MAX_LINK_LIMBS, MAX_ORDER_BITS);
    ZKH_REQUIRE(a.version < 9 || r.flags <= (LINK_READS | LINK_JOINS), "set_arguments: record %u: word 5 of a LINK is %#x (bit 0: READS, the read rule; bit 1: JOINS, "
                "a port of its head's memory; the other bits are reserved)", i, r.flags);
    ZKH_REQUIRE(a.version >= 9 || r.flags <= LINK_READS, "set_arguments: record %u: word 5 of a LINK is %#x (bit 0: READS, the read rule; the other bits are reserved)", i, r.flags);
    ZKH_REQUIRE((r.flags & LINK_READS) || !(r.wg | r.wc), "set_arguments: record %u: words 14, 15 of a LINK name a write flag, but bit 0 of word 5 (READS) is not set", i);
    ZKH_REQUIRE(!(r.flags & LINK_READS) || r.nc >= 2, "set_arguments: record %u: READS needs a clock and a value column (2..%u carried columns), this LINK carries %u", i,
                MAX_CARRIED, r.nc);
    ZKH_REQUIRE(!r.reserved, "set_arguments: record %u: a reserved word of a LINK is not 0 (words 5, 14, 15, the unused carried pairs and the unused "
                "destination words)", i);
    ZKH_REQUIRE(r.sel == NONE || r.sel < c->group_size[GROUP_CODE], "set_arguments: record %u: selector %u is not a code column", i, r.sel);
    // logup._joins_rule (version 9): a joiner's head is a LINK record without JOINS before it, the records between them join the same head
    // (the records of a blob that reaches this rule are in their order: whatever lies between two LINK records is a LINK record), it has the
    // head's nc, L, nl and READS-ness, and a memory has at most MAX_PORTS records
    const uint32_t h = a.heads[&r - a.links.data()];
    if (h == NONE) return nullptr;
    const Link* head = nullptr;
    for (size_t p = 0; p < a.links.size(); p++)
        if (a.links[p].index == h && h < i && a.heads[p] == NONE) head = &a.links[p];
    ZKH_REQUIRE(head, "set_arguments: record %u: a LINK joins record %u, which is no LINK record without JOINS before it (a port joins the head of its memory)", i, h);
    for (size_t p = 0; p < a.links.size(); p++)
        ZKH_REQUIRE(a.links[p].index <= h || a.links[p].index >= i || a.heads[p] == h, "set_arguments: record %u: a LINK joins record %u, but record %u between them "
                    "does not (a memory is a run of consecutive LINK records)", i, h, a.links[p].index);
    ZKH_REQUIRE(r.nc == head->nc && r.L == head->L && r.nl == head->nl && (r.flags & LINK_READS) == (head->flags & LINK_READS), "set_arguments: record %u: a LINK joins "
                "record %u with another nc, L, nl or READS (the ports of a memory have their head's)", i, h);
    ZKH_REQUIRE(i - h < MAX_PORTS, "set_arguments: record %u: port %u of the memory of record %u (a memory has at most %u records)", i, i - h, h, MAX_PORTS);
    return nullptr;
}

// logup.check_pages' own clause (a): the ranges of L and ng, word 4 (version 10: V - 1), word 5 (version 11: F), the reserved words, and the target a LINK with READS and nc = 1 + V
const char* pages_clause_a(const Arguments& a, const Pages& g) {
    const uint32_t i = g.index;
    ZKH_REQUIRE(g.L >= 1 && g.L <= 16 && g.ng >= 1 && g.ng <= MAX_PAGE_LIMBS && g.L * g.ng <= MAX_ORDER_BITS, "set_arguments: record %u: a PAGES record of %u limbs "
                "of %u bits (1..%u limbs of 1..16 bits, at most %u bits in all)", i, g.ng, g.L, MAX_PAGE_LIMBS, MAX_ORDER_BITS);
    ZKH_REQUIRE(a.version < 10 || g.word4 < MAX_PAGE_WORDS, "set_arguments: record %u: word 4 of a PAGES record is %u (V - 1: 0 = one value word per address, 1 = two)", i,
                g.word4);
    ZKH_REQUIRE(g.word5 == 0 || g.word5 == MAX_PAGE_FLATS, "set_arguments: record %u: word 5 of a PAGES record is %u (F, the flat-address destinations: 0 or 2)", i, g.word5);
    ZKH_REQUIRE(g.F == 0 || g.V > 1, "set_arguments: record %u: a PAGES record of one value word per address has %u flat-address destinations (they are the flat addresses "
                "of two value words)", i, g.F);
    ZKH_REQUIRE(!g.reserved || a.version < 11, "set_arguments: record %u: a reserved word of a PAGES record is not 0 (words 8..15, words 6 and 7 without flat-address "
                "destinations, and the unused destination words)", i);
    ZKH_REQUIRE(!g.reserved || a.version < 10, "set_arguments: record %u: a reserved word of a PAGES record is not 0 (words 5..15 and the unused destination words)", i);
    ZKH_REQUIRE(!g.reserved, "set_arguments: record %u: a reserved word of a PAGES record is not 0 (words 4..15 and the unused destination words)", i);
    ZKH_REQUIRE(paged_link(a, g) || g.V == 1, "set_arguments: record %u: a PAGES record of two value words per address pages record %u, which is no LINK record with READS "
                "and three carried columns (a clock and two values)", i, g.link);
    ZKH_REQUIRE(paged_link(a, g), "set_arguments: record %u: a PAGES record pages record %u, which is no LINK record with READS and two carried columns (a clock "
                "and one value)", i, g.link);
    const uint32_t h = a.heads[paged_link(a, g) - a.links.data()];
    ZKH_REQUIRE(h == NONE, "set_arguments: record %u: a PAGES record pages record %u, which joins record %u (a PAGES record names the head of a memory)", i, g.link, h);
    return nullptr;
}

// logup._check_owned, the ownership rule (arguments.h) over one kind of record: the LIMBS / ORDER records, whose peers are one another
// (logup.check_columns), the LINK records (kind 1) or the PAGES record (kind 2), whose peers are all records (logup.check_links,
// logup.check_pages).  The first record that breaks a clause.
// Per record: the kind's clause (a); (b) its sources are code or data columns of the circuit, its destinations pairwise distinct data
// columns.  Then, per record again: (c) no source is a destination of any record (records never chain) or a derived multiplicity, and a
// LINK's is no sorted copy's column either; (d) no destination is written twice: by another record, a sorted copy or a derived
// multiplicity; (e) no destination is read by the source term of a sorted copy (the sort runs first; check_sorted has bounded
// sorted_from) or, a LINK's or the PAGES record's, by any record, and none is a term's multiplicity, a LINK's linked and last and a PAGES
// record's p_on apart.  kind: 0 = LIMBS / ORDER, 1 = LINK, 2 = PAGES.
const char* check_owned(const zkh_circuit* c, const Arguments& a, const std::vector<Owned>& all, int kind) {
    const bool links = kind != 0;                       // a LINK or the PAGES record
    const size_t n_rec = a.records.size(), n_link = n_rec + a.links.size();
    const size_t lo = kind == 0 ? 0 : kind == 1 ? n_rec : n_link, top = kind == 0 ? n_rec : kind == 1 ? n_link : all.size();   // the kind is [lo, top) ...
    const size_t hi = links ? all.size() : n_rec;       // ... its peers [0, hi)
    const uint32_t n_terms = (uint32_t)a.terms.size();
    auto is_mult = [](const Term& t, uint32_t col) { return t.mg == GROUP_DATA && t.mc == col; };
    for (size_t p = lo; p < top; p++) {
        const Owned& v = all[p];
        const uint32_t i = v.index;
        ZKH_TRY(kind == 2 ? pages_clause_a(a, a.pages[p - n_link]) : links ? links_clause_a(c, a, a.links[p - n_rec]) : columns_clause_a(a.records[p], i));
        for (uint32_t s = 0; s < v.n_src; s++)
            ZKH_REQUIRE(is_column(c, v.sg[s], v.sc[s]), "set_arguments: record %u: source (%u, %u) is not a code or data column", i, v.sg[s], v.sc[s]);
        for (uint32_t e = 0; e < v.n_dst; e++) {
            ZKH_REQUIRE(v.dst[e] < c->group_size[GROUP_DATA], "set_arguments: record %u: destination %u is not a data column", i, v.dst[e]);
            for (uint32_t e2 = 0; e2 < e; e2++)
                ZKH_REQUIRE(v.dst[e2] != v.dst[e], "set_arguments: record %u: its destination (data %u) appears twice", i, v.dst[e]);
        }
    }
    for (size_t p = lo; p < top; p++) {
        const Owned& v = all[p];
        const uint32_t i = v.index;
        for (uint32_t s = 0; s < v.n_src; s++) {
            const uint32_t col = v.sc[s];
            if (v.sg[s] != GROUP_DATA) continue;
            for (uint32_t j = 0; links && j < n_terms; j++)
                ZKH_REQUIRE(!(a.terms[j].sorted && in_tuple(a.terms[j], a.terms[j].w, GROUP_DATA, col)), "set_arguments: record %u: its source (data %u) is written "
                            "by the sorted copy term %u (a LINK reads what no derive writes)", i, col, j);
            for (size_t q = 0; q < hi; q++)
                ZKH_REQUIRE(!all[q].writes(col), "set_arguments: record %u: its source (data %u) is a destination of record %u (records never chain)", i, col,
                            all[q].index);
            for (uint32_t j = 0; j < n_terms; j++)
                ZKH_REQUIRE(!(a.terms[j].derive && is_mult(a.terms[j], col)), "set_arguments: record %u: its source (data %u) is the derived multiplicity of term %u",
                            i, col, j);
        }
        for (uint32_t e = 0; e < v.n_dst; e++) {
            const uint32_t col = v.dst[e];
            for (size_t q = 0; q < hi; q++)
                ZKH_REQUIRE(q == p || !all[q].writes(col), "set_arguments: record %u: its destination (data %u) is also written by record %u", i, col, all[q].index);
            for (uint32_t j = 0; j < n_terms; j++) {
                const Term& t = a.terms[j];
                ZKH_REQUIRE(!(t.sorted && in_tuple(t, t.w, GROUP_DATA, col)), "set_arguments: record %u: its destination (data %u) is written by the sorted copy "
                            "term %u", i, col, j);
                ZKH_REQUIRE(!(t.derive && is_mult(t, col)), "set_arguments: record %u: its destination (data %u) is the derived multiplicity of term %u", i, col, j);
            }
            for (size_t q = 0; links && q < hi; q++)
                ZKH_REQUIRE(!all[q].reads(col), "set_arguments: record %u: its destination (data %u) is read by record %u (the links run after the columns, and never "
                            "chain)", i, col, all[q].index);
            for (const Term& t : a.terms)
                ZKH_REQUIRE(!(t.sorted && in_tuple(a.terms[t.sorted_from], a.terms[t.sorted_from].w, GROUP_DATA, col)), "set_arguments: record %u: its destination "
                            "(data %u) is read by term %u, the source of a sorted copy (the sort runs first)", i, col, t.sorted_from);
            for (uint32_t j = 0; j < n_terms; j++) {
                ZKH_REQUIRE(links || !is_mult(a.terms[j], col), "set_arguments: record %u: its destination (data %u) is the multiplicity of term %u", i, col, j);
                ZKH_REQUIRE(kind != 1 || e < v.free || !is_mult(a.terms[j], col), "set_arguments: record %u: its destination (data %u) is the multiplicity of term %u (of a "
                            "LINK's destinations only linked and last may be)", i, col, j);
                ZKH_REQUIRE(kind != 2 || e < v.free || !is_mult(a.terms[j], col), "set_arguments: record %u: its destination (data %u) is the multiplicity of term %u (of a "
                            "PAGES record's destinations only p_on may be)", i, col, j);
            }
        }
    }
    return nullptr;
}

// logup.check_open: the OPEN record is the last record and the only one of its kind; its reserved words are 0; its tag is below P, some term
// carries it and none of them is derived or a sorted copy; alpha, beta and the total are three disjoint runs of 4 words inside the circuit's
// `out`; header words 3, 4 repeat alpha and beta
const char* open_rule(const zkh_circuit* c, const Arguments& a) {
    if (a.open.empty()) return nullptr;
    const Open& o = a.open[0];
    const uint32_t i = o.index;
    if (a.after_open != NONE) {
        ZKH_REQUIRE(!a.second_open, "set_arguments: record %u: a second OPEN record (record %u is one: a seal closes on one total)", a.after_open, i);
        return make_err("set_arguments: record %u: a record after the OPEN record %u (the OPEN record comes last)", a.after_open, i);
    }
    ZKH_REQUIRE(!o.reserved, "set_arguments: record %u: a reserved word of the OPEN record is not 0 (words 6..15)", i);
    ZKH_REQUIRE(o.tag < P, "set_arguments: record %u: the open tag %u is not below P", i, o.tag);
    ZKH_REQUIRE(o.out_words == c->global_size[GLOBAL_OUT], "set_arguments: record %u: the OPEN record is of a circuit with %u out words, this one has %u", i,
                o.out_words, c->global_size[GLOBAL_OUT]);
    const uint32_t off[3] = {o.alpha, o.beta, o.total};
    const char* name[3] = {"alpha", "beta", "the total"};
    for (int e = 0; e < 3; e++)
        ZKH_REQUIRE((uint64_t)off[e] + 4 <= o.out_words, "set_arguments: record %u: %s at out words %u..%u, the circuit has %u", i, name[e], off[e], off[e] + 3,
                    o.out_words);
    for (int e = 0; e < 3; e++)
        for (int f = 0; f < e; f++)
            ZKH_REQUIRE(off[e] + 4 <= off[f] || off[f] + 4 <= off[e], "set_arguments: record %u: alpha, beta and the total overlap in out (words %u, %u, %u: 4 words each)",
                        i, o.alpha, o.beta, o.total);
    ZKH_REQUIRE(a.alpha == o.alpha && a.beta == o.beta, "set_arguments: record %u: header words 3, 4 are %u, %u, the OPEN record's alpha, beta are %u, %u", i,
                a.alpha, a.beta, o.alpha, o.beta);
    bool any = false;
    for (uint32_t j = 0; j < a.terms.size(); j++) {
        if (a.terms[j].tag != o.tag) continue;
        any = true;
        ZKH_REQUIRE(!a.terms[j].derive && !a.terms[j].sorted, "set_arguments: record %u: term %u of the open tag %u is derived or a sorted copy (another seal answers "
                    "the open tag)", i, j, o.tag);
    }
    ZKH_REQUIRE(any, "set_arguments: record %u: no term has the open tag %u", i, o.tag);
    return nullptr;
}

// the arguments against the circuit's shape, then the rules of sorted copies, then those of derived multiplicities
const char* check_arguments(const zkh_circuit* c, const Arguments& a) {
    const uint32_t k = a.k;
    ZKH_REQUIRE(k >= 1 && 4ull * k == c->group_size[GROUP_ACCUM], "set_arguments: %u accum Fp4 columns, the circuit's accum group is %u wide",
                k, c->group_size[GROUP_ACCUM]);
    const uint32_t mix = c->global_size[GLOBAL_MIX];
    ZKH_REQUIRE(a.is_open() || ((uint64_t)a.alpha + 4 <= mix && (uint64_t)a.beta + 4 <= mix), "set_arguments: alpha / beta at mix words %u / %u, the circuit has %u",
                a.alpha, a.beta, mix);
    std::vector<uint32_t> per_col(k, 0);
    uint32_t prev = 0;
    for (uint32_t i = 0; i < a.terms.size(); i++) {
        const Term& t = a.terms[i];
        ZKH_REQUIRE(t.col < k && t.col >= prev, "set_arguments: term %u: accum column %u (columns 0..%u, terms sorted by column)", i, t.col, k - 1);
        prev = t.col;
        ZKH_REQUIRE(++per_col[t.col] <= MAX_TERMS, "set_arguments: accum column %u has more than %u terms (the degree bound)", t.col, MAX_TERMS);
        ZKH_REQUIRE(t.neg <= 1 && t.tag < P, "set_arguments: term %u: sign word %u / tag %u", i, t.neg, t.tag);
        ZKH_REQUIRE(t.sel == NONE || t.sel < c->group_size[GROUP_CODE], "set_arguments: term %u: selector %u is not a code column", i, t.sel);
        ZKH_REQUIRE(t.mg == NONE || is_column(c, t.mg, t.mc), "set_arguments: term %u: multiplicity column (%u, %u) is not a code or data column", i,
                    t.mg, t.mc);
        ZKH_REQUIRE(t.w >= 1 && t.w <= MAX_TUPLE, "set_arguments: term %u: tuple width %u (1..%u)", i, t.w, MAX_TUPLE);
        for (uint32_t e = 0; e < t.w; e++)
            ZKH_REQUIRE(is_column(c, t.tg[e], t.tc[e]), "set_arguments: term %u: tuple column (%u, %u) is not a code or data column", i, t.tg[e], t.tc[e]);
    }
    for (uint32_t col = 0; col < k; col++) ZKH_REQUIRE(per_col[col] >= 1, "set_arguments: accum column %u has no terms", col);
    if (a.version >= 3) ZKH_TRY(check_sorted(a));
    if (a.version >= 2) ZKH_TRY(check_derived(a));
    ZKH_TRY(open_rule(c, a));
    if (a.after_pages != NONE) {
        ZKH_REQUIRE(!a.second_pages, "set_arguments: record %u: a second PAGES record (record %u is one: a blob pages one memory)", a.after_pages, a.pages[0].index);
        return make_err("set_arguments: record %u: a record after the PAGES record %u (the PAGES record comes last)", a.after_pages, a.pages[0].index);
    }
    ZKH_REQUIRE(a.late_record == NONE, "set_arguments: record %u: a LIMBS / ORDER record after the LINK record %u (LINK records come last)", a.late_record,
                a.late_after);
    const std::vector<Owned> all = owned(a);
    ZKH_TRY(check_owned(c, a, all, 0));
    ZKH_TRY(check_owned(c, a, all, 1));
    return check_owned(c, a, all, 2);
}

}  // namespace

const char* zkh::trace_rows(const char* who, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, const zkh_buf* data,
                            const zkh_buf* accum, size_t* n, uint32_t* A) {
    ZKH_REQUIRE(po2 >= 1 && po2 <= 24, "%s: po2 %zu out of range", who, po2);
    *n = (size_t)1 << po2;
    ZKH_REQUIRE(zk_cycles < *n, "%s: zk_cycles %zu leaves no active row at po2 %zu", who, zk_cycles, po2);
    *A = (uint32_t)(*n - zk_cycles);
    ZKH_REQUIRE((!code || code->len == (size_t)c->group_size[GROUP_CODE] * *n) && data->len == (size_t)c->group_size[GROUP_DATA] * *n &&
                (!accum || accum->len == (size_t)c->group_size[GROUP_ACCUM] * *n), "%s: buffer shape mismatch", who);
    return nullptr;
}

extern "C" const char* zkh_circuit_set_arguments(zkh_circuit* c, const uint32_t* blob, size_t words) {
    ZKH_REQUIRE(c && (blob || !words), "set_arguments: null argument");
    if (!words) { c->args.reset(); return nullptr; }
    auto a = std::make_shared<Arguments>();
    ZKH_TRY(decode_arguments(blob, words, a.get()));
    ZKH_TRY(check_arguments(c, *a));
    c->args = std::move(a);
    return nullptr;
}

extern "C" int zkh_circuit_has_arguments(const zkh_circuit* c) { return c && c->args; }

extern "C" int zkh_circuit_derives_multiplicities(const zkh_circuit* c) {
    return c && c->args && std::any_of(c->args->terms.begin(), c->args->terms.end(), [](const Term& t) { return t.derive; });
}

extern "C" int zkh_circuit_derives_sorted(const zkh_circuit* c) {
    return c && c->args && std::any_of(c->args->terms.begin(), c->args->terms.end(), [](const Term& t) { return t.sorted; });
}

extern "C" int zkh_circuit_derives_columns(const zkh_circuit* c) { return c && c->args && !c->args->records.empty(); }

extern "C" int zkh_circuit_derives_links(const zkh_circuit* c) { return c && c->args && !c->args->links.empty(); }

extern "C" int zkh_circuit_links_check_reads(const zkh_circuit* c) { return c && c->args ? (int)c->args->reads : 0; }

extern "C" int zkh_circuit_pages(const zkh_circuit* c) { return c && c->args && !c->args->pages.empty(); }

extern "C" int zkh_circuit_page_words(const zkh_circuit* c) { return c && c->args ? (int)c->args->page_words() : 0; }

extern "C" int zkh_circuit_page_flats(const zkh_circuit* c) { return c && c->args ? (int)c->args->page_flats() : 0; }

extern "C" int zkh_circuit_open_bus(const zkh_circuit* c, uint32_t where[4]) {
    if (!c || !c->args || !c->args->is_open()) return 0;
    const Open& o = c->args->open[0];
    if (where) { where[0] = o.tag; where[1] = o.alpha; where[2] = o.beta; where[3] = o.total; }
    return 1;
}

// THE DERIVE STAGES, IN THEIR ORDER (arguments.h, WHO WRITES A DATA COLUMN): the one statement of the order in code.  A LIMBS / ORDER
// record may read a sorted copy's column, and the multiplicities count the limbs that the records and the links derive.
namespace {
using Derive = const char* (*)(zkh_ctx*, const zkh_circuit*, size_t, size_t, const zkh_buf*, zkh_buf*, const PagedFrom&);
template <const char* (*F)(zkh_ctx*, const zkh_circuit*, size_t, size_t, const zkh_buf*, zkh_buf*)>
const char* no_image(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const PagedFrom&) {
    return F(ctx, c, po2, zk_cycles, code, data);
}
const struct { const char* name; int (*derives)(const zkh_circuit*); Derive derive; } STAGES[] = {
    {"sorted", zkh_circuit_derives_sorted, no_image<zkh_derive_sorted>},
    {"columns", zkh_circuit_derives_columns, no_image<zkh_derive_columns>},
    {"links", zkh_circuit_derives_links, derive_links_from},                // the one stage that reads the memory image (a PAGES record), as words or as a page table
    {"multiplicities", zkh_circuit_derives_multiplicities, no_image<zkh_derive_multiplicities>},
};
}  // namespace

// every stage the circuit's arguments have, with the arguments as given: the stage's own checks and messages are the call's.  A circuit
// whose arguments page memory is refused without an image, or a page table in its place, before any stage writes.
static const char* derive_all_from(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data, const PagedFrom& mem) {
    ZKH_REQUIRE(c, "derive_all: null circuit");
    ZKH_REQUIRE(mem.image || mem.table || !zkh_circuit_pages(c), "derive_all: the arguments page memory: an image is required (zkh_derive_all_paged)");
    for (const auto& s : STAGES)
        if (s.derives(c)) ZKH_TRY(s.derive(ctx, c, po2, zk_cycles, code, data, mem));
    return nullptr;
}

extern "C" const char* zkh_derive_all_paged(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data,
                                            const zkh_buf* image) {
    return derive_all_from(ctx, c, po2, zk_cycles, code, data, PagedFrom{image});
}

extern "C" const char* zkh_derive_all_paged_table(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data,
                                                  const zkh_buf* table, size_t table_at, size_t D, size_t image_words) {
    ZKH_REQUIRE(c, "derive_all: null circuit");
    ZKH_REQUIRE(table || !zkh_circuit_pages(c), "derive_all: the arguments page memory: a page table is required (zkh_derive_all_paged_table)");
    return derive_all_from(ctx, c, po2, zk_cycles, code, data, PagedFrom{nullptr, table, table_at, D, image_words});
}

extern "C" const char* zkh_derive_all(zkh_ctx* ctx, const zkh_circuit* c, size_t po2, size_t zk_cycles, const zkh_buf* code, zkh_buf* data) {
    return zkh_derive_all_paged(ctx, c, po2, zk_cycles, code, data, nullptr);
}

extern "C" const char* zkh_circuit_derived_data_columns(const zkh_circuit* c, uint32_t* cols, size_t cap, size_t* n) {
    ZKH_REQUIRE(c && n && (cols || !cap), "derived_data_columns: null argument");
    std::vector<uint32_t> out;
    if (c->args) {
        for (const Term& t : c->args->terms) {
            if (t.derive) out.push_back(t.mc);
            if (t.sorted) out.insert(out.end(), t.tc, t.tc + t.w);
        }
        for (const Owned& v : owned(*c->args)) out.insert(out.end(), v.dst, v.dst + v.n_dst);
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    *n = out.size();
    ZKH_REQUIRE(out.size() <= cap, "derived_data_columns: %zu columns, room for %zu", out.size(), cap);
    std::copy(out.begin(), out.end(), cols);
    return nullptr;
}
