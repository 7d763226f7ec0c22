// sort.h — the stable sort of selected trace rows by packed keys that sort.hip owns (its kernels live there and nowhere else), for
// its two callers: zkh_derive_sorted (sort.hip) and zkh_derive_links (links.hip), and the counter scan inside it, which every compaction
// launches as well after its heads stage (scan.h scan_heads): the page scan of links.hip, the lists and the proof of image.hip.
#pragma once
#include <vector>

#include "arguments.h"

namespace zkh {

struct SortPair {                                       // one sort as the kernels read it (zkh_derive_sorted: a pair (D, S))
    uint32_t d_term, w, nkeys, sel;                     // D's blob index; tuple width; key fields; selector code column or NONE
    uint32_t kg[MAX_SORT_KEYS], kc[MAX_SORT_KEYS];      // the key columns, most significant first
    uint32_t sg[MAX_TUPLE], sc[MAX_TUPLE];              // S's tuple
    uint32_t dc[MAX_TUPLE];                             // D's tuple (data columns)
};
// status words: [0, 2) the first bad selector (pair << 32 | row), then per pair ST_WORDS: OR[3], AND[3], m = selected rows, unused
constexpr uint32_t ST_HEAD = 2, ST_WORDS = 8, ST_OR = 0, ST_AND = 3, ST_M = 6;

// What sort_rows leaves on the device, pair p at items [p cap, p cap + m_p) (cap = A unless runs are given): the packed keys (the live bits of the key fields: two rows have
// equal keys exactly when their packed keys are equal) in ascending order, equal keys in row order, and the source row of each.
struct SortedRows {
    Tmp pairs, status, selbase;                         // the SortPair table; the status words; per 64-row group the rank of its first selected row
    Tmp klo[2], khi[2], idx[2], hist, totals;
    Tmp runs;                                           // sort_rows with runs: the Memory table on the device
    uint32_t cap = 0;                                   // the items a pair (a run) can hold: pair p's items start at p * cap; A without runs
    int cur = 0;                                        // which of the two item buffers holds the result
    bool wide = false;                                  // keys of more than 64 live bits: khi holds bits 64..95
    uint32_t groups = 0;
    std::vector<uint32_t> st;                           // the status words as read back after the key pass
    bool bad_selector = false;                          // a selector other than 0 / 1: the lowest (pair, row); nothing was sorted
    uint32_t bad_pair = 0, bad_row = 0;
    const SortPair* d_pairs() const { return (const SortPair*)pairs->ptr(); }
    const unsigned long long* keys() const { return (const unsigned long long*)klo[cur]->ptr(); }
    const uint32_t* rows() const { return idx[cur]->ptr(); }
};
// the passes (a) .. (c) of sort.hip over `pairs`, all pairs in the same launches.
// runs (links.hip, the ports of ZKA1 version 9): run r is ONE sort over the accesses of the pairs [runs[r].first, runs[r].first + runs[r].k), which
// tile the pairs.  Its items are ordered by (row, port) before the first radix pass, so the stable passes end in (key, row, port) order; the
// item's source id is the virtual row v = row * k + port; the live-bit masks are the run's, not a pair's; status words, `cap` and the item
// buffers are per run (run r at items [r cap, r cap + m_r), cap = A * the most ports of a run).  A bad selector still names (pair, row).
const char* sort_rows(zkh_ctx* ctx, const zkh_buf* code, const zkh_buf* data, size_t n, uint32_t A, const std::vector<SortPair>& pairs, SortedRows* out,
                      const std::vector<Memory>* runs = nullptr);

// the exclusive scan, in place, of `segments` runs of `len` counters each at v (k_sort_scan: one workgroup per run, none waits for another);
// with `total`, the sum of run s goes to total[s * total_stride].  A plain launch on the context's stream.
void scan_counters(zkh_ctx* ctx, uint32_t* v, uint32_t segments, uint32_t len, uint32_t* total, uint32_t total_stride);

}  // namespace zkh
