// claims.h — the claim rules of the recursion tree and of the P2-JOIN tree, as plain C++ (no HIP, no library, no threads).
//
// What a lift / lift2 / join / join3 / union / resolve node PUBLISHES, what it READS as witness, and the shape in which nodes
// fold: the host side of zeth_amd/circuits/rec_verify.py, once.  session.hip's prover (run_node), its verifiers
// (zkh_succinct_verify*, zkh_session_verify) and zkh_session_set_recursion all take these rules from here; the independent twin
// is zeth_amd/recursion.py (fold_leaf_claims, union_claims, resolved_claim, allowed_tree, membership_words), which
// tests/cpp/claims_test.cpp is compared with word for word, and the fold shape is checked there against scheduler.h's plan.
//   * claim' = hash_pair(core, (pre, post, 0, 0, 0, 0, 0, 0)): what every recursion receipt publishes (rec_verify.py _wrap) — its
//     core claim bound to the state range [pre, post] it covers.  A join opens both children's claim' in-circuit and asserts
//     post(left) = pre(right); the opening (core, pre, post) travels next to a receipt as witness for its parent, never trusted.
//   * fold: the first level pairs, every level above takes three at a time (a group of three is join(join(a, b), c)), a remainder
//     of two is a join, of one moves up (recursion.py fold_plan; scheduler.h build_fold_plan).
//   * union(l, r): wrap(hash_pair(lo, hi), 0, 0) with (lo, hi) the two claim' sorted by their CANONICAL words, lexicographically
//     (recursion.py union_node; ProverServer::union, risc0-zkvm 3.0.3: the UnionClaim keeps left <= right); the union tree takes
//     neighbours pairwise, level by level, an odd one moves up at the end of its level.
//   * resolve(cond, assum): the conditional's state range over hash_pair(claim'_cond, claim'_assum).
//   * the allowed-programs tree: 16 leaves (control roots, zero padded), a membership path = per level the direction bit as an
//     element, then the sibling (rec_verify.py ALLOWED_DEPTH, Verifier.allowed_member).
//   * the P2-JOIN tree (pair_fold): neighbours pairwise, an odd one moves up at the end of its level.
// The pair hash is a parameter: digests are Montgomery words and the header needs neither the Poseidon2 tables nor the library.
// Errors are strings, "" = ok (as scheduler.h's build_fold_plan returns them).
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "fp.h"

namespace zkh {
namespace claims {

using Digest = std::array<uint32_t, 8>;
using Levels = std::vector<std::vector<Digest>>;                          // allowed-programs tree: [leaves, ..., [root]]
using PairHash = std::function<std::string(const uint32_t* a, const uint32_t* b, uint32_t out[8])>;
constexpr size_t ALLOWED = 16, ALLOWED_DEPTH = 4;                         // zeth_amd/circuits/rec_verify.py ALLOWED_DEPTH

#define ZKH_CLAIMS_TRY(expr) do { const std::string _e = (expr); if (!_e.empty()) return _e; } while (0)

struct NodeClaim { uint32_t core[8] = {0}; uint32_t pre = 0, post = 0; };

inline std::string wrap(const PairHash& h, const NodeClaim& c, uint32_t out[8]) {
    const uint32_t st[8] = {c.pre, c.post, 0, 0, 0, 0, 0, 0};
    return h(c.core, st, out);
}
// parent of two nodes: core = hash_pair(claim'_l, claim'_r), state range = [pre_l, post_r]; the children must chain
inline std::string parent(const PairHash& h, const NodeClaim& l, const NodeClaim& r, NodeClaim* out) {
    if (l.post != r.pre) return "claim tree: two neighbouring nodes do not chain (post(l) != pre(r)): no join has a witness for them";
    uint32_t cl[8], cr[8];
    ZKH_CLAIMS_TRY(wrap(h, l, cl)); ZKH_CLAIMS_TRY(wrap(h, r, cr));
    NodeClaim nd;
    ZKH_CLAIMS_TRY(h(cl, cr, nd.core));
    nd.pre = l.pre; nd.post = r.post;
    *out = nd;
    return "";
}
// the fold plan's shape over claim nodes: pairs first, then three at a time, a remainder of two is a join, of one moves up
inline std::string fold_nodes(const PairHash& h, std::vector<NodeClaim> nodes, NodeClaim* root) {
    if (nodes.empty()) return "claim tree: no leaves";
    for (size_t group = 2; nodes.size() > 1; group = 3) {
        std::vector<NodeClaim> up;
        size_t k = 0;
        for (; k + group <= nodes.size(); k += group) {
            NodeClaim nd;
            ZKH_CLAIMS_TRY(parent(h, nodes[k], nodes[k + 1], &nd));
            if (group == 3) ZKH_CLAIMS_TRY(parent(h, nd, nodes[k + 2], &nd));
            up.push_back(nd);
        }
        if (nodes.size() - k == 2) { NodeClaim nd; ZKH_CLAIMS_TRY(parent(h, nodes[k], nodes[k + 1], &nd)); up.push_back(nd); }
        else if (nodes.size() - k == 1) up.push_back(nodes[k]);
        nodes.swap(up);
    }
    *root = nodes[0];
    return "";
}

// union: does (l, r) swap?  By canonical residues, the first differing word decides; equal claims stay
inline bool union_order(const uint32_t* l, const uint32_t* r) {
    for (int i = 0; i < 8; i++) {
        const uint32_t a = fp_decode(Fp::raw(l[i])), b = fp_decode(Fp::raw(r[i]));
        if (a != b) return b < a;
    }
    return false;
}
// the node union(l, r) of two claim': (hash_pair(lo, hi), 0, 0)
inline std::string union_node(const PairHash& h, const uint32_t* l, const uint32_t* r, NodeClaim* out, bool* swapped = nullptr) {
    const bool swap = union_order(l, r);
    if (swapped) *swapped = swap;
    *out = NodeClaim();
    return h(swap ? r : l, swap ? l : r, out->core);
}
inline std::string union_claim(const PairHash& h, const uint32_t* l, const uint32_t* r, uint32_t out[8]) {
    NodeClaim nd;
    ZKH_CLAIMS_TRY(union_node(h, l, r, &nd));
    return wrap(h, nd, out);
}
// the union tree over assumption claim': neighbours pairwise, level by level, an odd one moves up
inline std::string union_tree(const PairHash& h, std::vector<Digest> level, uint32_t out[8]) {
    if (level.empty()) return "union tree: no assumption claims";
    while (level.size() > 1) {
        std::vector<Digest> up;
        for (size_t k = 0; k + 1 < level.size(); k += 2) {
            Digest u;
            ZKH_CLAIMS_TRY(union_claim(h, level[k].data(), level[k + 1].data(), u.data()));
            up.push_back(u);
        }
        if (level.size() % 2) up.push_back(level.back());
        level.swap(up);
    }
    memcpy(out, level[0].data(), 32);
    return "";
}
// the node resolve(cond, assum): (hash_pair(claim'_cond, claim'_assum), pre, post of cond)
inline std::string resolved(const PairHash& h, const NodeClaim& cond, const uint32_t* assum_claim, NodeClaim* out) {
    uint32_t cc[8];
    ZKH_CLAIMS_TRY(wrap(h, cond, cc));
    NodeClaim nd;
    ZKH_CLAIMS_TRY(h(cc, assum_claim, nd.core));
    nd.pre = cond.pre; nd.post = cond.post;
    *out = nd;
    return "";
}

// The P2-JOIN tree's shape: per level, join_level fills up[k] from level[2 k], level[2 k + 1] (up.size() == level.size() / 2; the
// prover proves them, a verifier hashes them: hashed_level), an odd claim moves up at the END of its level.  Stops once `stop`
// claims are left: 1 = the root, 2 = the root's two children (what a verifier compares the root seal's public inputs with).
using JoinLevel = std::function<std::string(const std::vector<Digest>& level, std::vector<Digest>& up)>;
inline std::string pair_fold(std::vector<Digest> level, size_t stop, const JoinLevel& join_level, std::vector<Digest>* out) {
    if (level.empty() || !stop) return "pair fold: no claims";
    while (level.size() > stop) {
        std::vector<Digest> up(level.size() / 2);
        ZKH_CLAIMS_TRY(join_level(level, up));
        if (level.size() % 2) up.push_back(level.back());
        level.swap(up);
    }
    out->swap(level);
    return "";
}
inline JoinLevel hashed_level(const PairHash& h) {
    return [h](const std::vector<Digest>& level, std::vector<Digest>& up) -> std::string {
        for (size_t k = 0; k < up.size(); k++) ZKH_CLAIMS_TRY(h(level[2 * k].data(), level[2 * k + 1].data(), up[k].data()));
        return "";
    };
}

// levels of the allowed-programs tree over n <= 16 control roots (8 words each), zero padded to 16 leaves
inline std::string allowed_levels(const PairHash& h, const uint32_t* roots, size_t n, Levels* out) {
    if (n > ALLOWED) return "allowed-programs tree: more than 16 programs";
    std::vector<Digest> level(ALLOWED, Digest{});
    for (size_t i = 0; i < n; i++) memcpy(level[i].data(), roots + 8 * i, 32);
    out->assign(1, level);
    const JoinLevel up_level = hashed_level(h);
    while (level.size() > 1) {
        std::vector<Digest> up(level.size() / 2);
        ZKH_CLAIMS_TRY(up_level(level, up));
        out->push_back(up);
        level.swap(up);
    }
    return "";
}
// appends, per level: the direction bit as an element, then the sibling
inline void membership_path(const Levels& levels, size_t index, std::vector<uint32_t>& out) {
    for (size_t l = 0; l + 1 < levels.size(); l++) {
        out.push_back(fp_encode((uint32_t)(index & 1)).v);
        out.insert(out.end(), levels[l][index ^ 1].begin(), levels[l][index ^ 1].end());
        index >>= 1;
    }
}

// claim' of a session's root receipt: `ranks` contiguous equal ranges of the leaves folded on their own, their tops folded
// again; the union tree over the LIFTED assumption claims (a lifted receipt publishes wrap(receipt claim, 0, 0)); the resolve of
// the two — or the union root alone when there are no leaves
inline std::string session_root_claim(const PairHash& h, std::vector<NodeClaim> leaves, size_t ranks, const std::vector<Digest>& lifted_assumptions,
                                      uint32_t out[8]) {
    if (leaves.empty() && lifted_assumptions.empty()) return "claim tree: neither leaves nor assumptions";
    if (!ranks || leaves.size() % ranks) return "claim tree: the leaves do not split into equal ranges";
    uint32_t assumed[8];
    if (!lifted_assumptions.empty()) ZKH_CLAIMS_TRY(union_tree(h, lifted_assumptions, assumed));
    if (leaves.empty()) { memcpy(out, assumed, 32); return ""; }
    if (ranks > 1) {
        const size_t per = leaves.size() / ranks;
        std::vector<NodeClaim> tops(ranks);
        for (size_t r = 0; r < ranks; r++)
            ZKH_CLAIMS_TRY(fold_nodes(h, std::vector<NodeClaim>(leaves.begin() + r * per, leaves.begin() + (r + 1) * per), &tops[r]));
        leaves.swap(tops);
    }
    NodeClaim top;
    ZKH_CLAIMS_TRY(fold_nodes(h, leaves, &top));
    if (!lifted_assumptions.empty()) ZKH_CLAIMS_TRY(resolved(h, top, assumed, &top));
    return wrap(h, top, out);
}

// What a fold node reads (`in`, the words zkh_rec_prove takes) and what it publishes (`claim`), from its children.  A child is a
// receipt: its seal, the index of the program that proved it (its place in the allowed set) and its node claim.  By kind
// (scheduler.h PlanNode):
//   0 lift(a), 2 lift2(a, b) — the children are SEGMENT seals (claim: receipt claim + state words; program unused):
//     seal(s), then the allowed-programs root; claim = a's, or parent(a, b);
//   1 join(a, b), 3 join3(a, b, c) — per child: seal, membership path, the opening of its claim' (core, pre, post);
//     claim = parent(a, b), or parent(parent(a, b), c);
//   4 union(a, b) — per child: seal, membership path; then the swap bit as an element; claim = union_node(claim'_a, claim'_b);
//   5 resolve(a = the conditional, b = the assumptions' union root) — a: seal, path, opening; b: seal, path; claim = resolved.
struct Child { const uint32_t* seal = nullptr; size_t words = 0; uint32_t program = 0; NodeClaim claim; };
inline std::string node_witness(const PairHash& h, uint32_t kind, const Child* ch, size_t n_children, const Levels& allowed,
                                std::vector<uint32_t>& in, NodeClaim* claim) {
    const size_t want = kind == 0 ? 1 : kind == 3 ? 3 : 2;
    if (kind > 5 || n_children != want || allowed.size() != ALLOWED_DEPTH + 1) return "claim tree: a fold node of kind " + std::to_string(kind) + " with " + std::to_string(n_children) + " children";
    in.clear();
    auto seal = [&](const Child& c) { in.insert(in.end(), c.seal, c.seal + c.words); };
    auto path = [&](const Child& c) { membership_path(allowed, c.program, in); };
    auto opening = [&](const Child& c) { in.insert(in.end(), c.claim.core, c.claim.core + 8); in.push_back(c.claim.pre); in.push_back(c.claim.post); };
    if (kind == 0 || kind == 2) {
        for (size_t k = 0; k < n_children; k++) seal(ch[k]);
        in.insert(in.end(), allowed.back()[0].begin(), allowed.back()[0].end());
        if (kind == 0) { *claim = ch[0].claim; return ""; }
        return parent(h, ch[0].claim, ch[1].claim, claim);
    }
    if (kind == 1 || kind == 3) {
        for (size_t k = 0; k < n_children; k++) { seal(ch[k]); path(ch[k]); opening(ch[k]); }
        ZKH_CLAIMS_TRY(parent(h, ch[0].claim, ch[1].claim, claim));
        return kind == 3 ? parent(h, *claim, ch[2].claim, claim) : "";
    }
    uint32_t ca[8], cb[8];
    ZKH_CLAIMS_TRY(wrap(h, ch[1].claim, cb));
    if (kind == 4) {
        ZKH_CLAIMS_TRY(wrap(h, ch[0].claim, ca));
        bool swap = false;
        ZKH_CLAIMS_TRY(union_node(h, ca, cb, claim, &swap));
        for (size_t k = 0; k < 2; k++) { seal(ch[k]); path(ch[k]); }
        in.push_back(fp_encode(swap ? 1u : 0u).v);
        return "";
    }
    seal(ch[0]); path(ch[0]); opening(ch[0]);
    seal(ch[1]); path(ch[1]);
    return resolved(h, ch[0].claim, cb, claim);
}

#undef ZKH_CLAIMS_TRY

}  // namespace claims
}  // namespace zkh
