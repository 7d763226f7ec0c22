// The claim rules (zeth_amd/csrc/claims.h) as a unit: plain C++, no GPU, no library.
// Part A — structure, with a toy pair hash that logs its calls: the fold shape against scheduler.h's plan (the sequence of `parent`
//   applications IS the plan's lift2 / join / join3 nodes in dependency order), the union order, parent's refusal and range, the
//   P2-JOIN pair fold, membership paths against the allowed tree's top, the layout of every kind of node witness.
// Part B — values, with the real Poseidon2 hash_pair (header-only: poseidon2.h and the shipped constants): the program prints claims
//   for fixed inputs ("key = words" lines) and tests/test_session_claim_rules.py compares them word for word with
//   zeth_amd/recursion.py (fold_leaf_claims, union_claims, resolved_claim, allowed_tree, membership_words).
// Build: g++ -O1 -std=c++17 -Wall -Werror -Wno-unknown-pragmas -I zeth_amd/csrc tests/cpp/claims_test.cpp -o <out>;  "claims ok" + exit code 0 = all hold.
#include "claims.h"
#include "scheduler.h"
#include "poseidon2.h"          // kernel code too: its `#pragma unroll` is hipcc's, hence -Wno-unknown-pragmas
#include "../../include/zkh_poseidon2_consts.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

using namespace zkh;
using namespace zkh::claims;

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// ---- the toy hash: depends on both inputs and their order; every call is logged ----
struct Call { Digest a, b, out; };
static std::vector<Call> calls;
static std::string toy(const uint32_t* a, const uint32_t* b, uint32_t out[8]) {
    uint64_t acc = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 8; i++) acc = (acc ^ a[i]) * 0xBF58476D1CE4E5B9ull + 1;
    for (int i = 0; i < 8; i++) acc = (acc ^ b[i]) * 0x94D049BB133111EBull + 3;
    Call c;
    for (int i = 0; i < 8; i++) { acc ^= acc >> 29; acc *= 0xD1B54A32D192ED03ull; out[i] = (uint32_t)((acc >> 16) % P); c.a[i] = a[i]; c.b[i] = b[i]; c.out[i] = out[i]; }
    calls.push_back(c);
    return "";
}
static const PairHash TOY = toy;

static uint64_t rng_state = 0x1234567ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((rng_state >> 33) % P); }
static Digest rnd_digest() { Digest d; for (auto& w : d) w = rnd(); return d; }
static NodeClaim leaf(uint32_t pre, uint32_t post) { NodeClaim c; for (auto& w : c.core) w = rnd(); c.pre = pre; c.post = post; return c; }
static bool same(const NodeClaim& x, const NodeClaim& y) { return memcmp(x.core, y.core, 32) == 0 && x.pre == y.pre && x.post == y.post; }

// ---- fold shape: fold_nodes against sched::build_fold_plan ----
using Range = std::pair<uint32_t, uint32_t>;
using Application = std::pair<Range, Range>;            // parent(l, r), by the leaf ranges [pre, post] of l and r (leaf i covers [i, i + 1])
static void fold_shape(size_t n, bool fused) {
    sched::FoldPlan plan;
    const std::string perr = sched::build_fold_plan(std::vector<uint32_t>(n, 12),
        [&](uint32_t kind, uint32_t, uint32_t) { return (kind == 2 || kind == 3) && !fused ? -1 : 0; }, [](uint32_t) { return 12u; }, &plan);
    CHECK(perr.empty(), "plan n=%zu: %s", n, perr.c_str());
    std::vector<Application> want;
    std::vector<Range> range(plan.nodes.size());
    for (size_t k = 0; k < plan.nodes.size(); k++) {          // index order = dependency order: children come before their parent
        const sched::PlanNode& nd = plan.nodes[k];
        if (nd.kind == 0) { range[k] = {(uint32_t)nd.a, (uint32_t)nd.a + 1}; continue; }
        const Range l = nd.kind == 2 ? Range{(uint32_t)nd.a, (uint32_t)nd.a + 1} : range[nd.a], r = nd.kind == 2 ? Range{(uint32_t)nd.b, (uint32_t)nd.b + 1} : range[nd.b];
        CHECK(nd.kind == 2 || (nd.a < k && nd.b < k && (nd.kind != 3 || nd.c < k)), "plan n=%zu: node %zu before a child", n, k);
        want.push_back({l, r});
        range[k] = {l.first, r.second};
        if (nd.kind == 3) { want.push_back({range[k], range[nd.c]}); range[k].second = range[nd.c].second; }      // join3 = join(join(a, b), c)
    }
    std::vector<NodeClaim> leaves;
    for (size_t i = 0; i < n; i++) leaves.push_back(leaf((uint32_t)i, (uint32_t)i + 1));
    calls.clear();
    NodeClaim root;
    CHECK(fold_nodes(TOY, leaves, &root).empty(), "fold_nodes n=%zu", n);
    // a parent application is three calls: wrap(l), wrap(r) — whose second operand is (pre, post, 0 ..) — then the pair of the two
    CHECK(calls.size() == 3 * want.size(), "n=%zu fused=%d: %zu hash calls, the plan has %zu parent applications", n, (int)fused, calls.size(), want.size());
    for (size_t k = 0; k < want.size(); k++) {
        const Call &wl = calls[3 * k], &wr = calls[3 * k + 1], &pr = calls[3 * k + 2];
        for (int i = 2; i < 8; i++) CHECK(wl.b[i] == 0 && wr.b[i] == 0, "n=%zu application %zu: not a wrap", n, k);
        CHECK(pr.a == wl.out && pr.b == wr.out, "n=%zu application %zu: the pair is not (claim'_l, claim'_r)", n, k);
        const Application got{{wl.b[0], wl.b[1]}, {wr.b[0], wr.b[1]}};
        CHECK(got == want[k], "n=%zu fused=%d application %zu: fold_nodes joins [%u, %u] + [%u, %u], the plan [%u, %u] + [%u, %u]", n, (int)fused, k,
              got.first.first, got.first.second, got.second.first, got.second.second, want[k].first.first, want[k].first.second, want[k].second.first, want[k].second.second);
    }
    CHECK(root.pre == 0 && root.post == n, "n=%zu: root range", n);
    if (!want.empty()) CHECK(memcmp(root.core, calls.back().out.data(), 32) == 0, "n=%zu: the root is not the last application", n);
}

static void union_rules() {
    // a pair whose Montgomery words and canonical residues sort opposite ways
    uint32_t x = 0, y = 0;
    for (int t = 0; t < 100000 && !x; t++) {
        const uint32_t a = rnd(), b = rnd();
        if ((a < b) != (fp_decode(Fp::raw(a)) < fp_decode(Fp::raw(b))) && a != b) { x = a; y = b; }
    }
    CHECK(x, "no pair with opposite orders found");
    Digest l = rnd_digest(), r = l;
    l[0] = x; r[0] = y;
    const bool canon_swap = fp_decode(Fp::raw(y)) < fp_decode(Fp::raw(x));
    CHECK(canon_swap == (x < y), "search");
    CHECK(union_order(l.data(), r.data()) == canon_swap && union_order(r.data(), l.data()) == !canon_swap, "union order is not by canonical residues");
    // the FIRST differing word decides: word 3 says one thing, word 5 the opposite
    Digest p = rnd_digest(), q = p;
    p[3] = fp_encode(5).v; q[3] = fp_encode(9).v; p[5] = fp_encode(9).v; q[5] = fp_encode(5).v;
    CHECK(!union_order(p.data(), q.data()) && union_order(q.data(), p.data()), "union order: first differing word first");
    CHECK(!union_order(p.data(), p.data()), "equal claims swap");
    // union_claim is symmetric, = wrap(hash(lo, hi), 0, 0); the tree pairs neighbours, an odd one moves up
    uint32_t u1[8], u2[8], w[8];
    CHECK(union_claim(TOY, l.data(), r.data(), u1).empty() && union_claim(TOY, r.data(), l.data(), u2).empty() && memcmp(u1, u2, 32) == 0, "union(a, b) != union(b, a)");
    NodeClaim nd;
    const Digest &lo = canon_swap ? r : l, &hi = canon_swap ? l : r;
    toy(lo.data(), hi.data(), nd.core);
    CHECK(wrap(TOY, nd, w).empty() && memcmp(w, u1, 32) == 0, "union claim");
    const std::vector<Digest> five{rnd_digest(), rnd_digest(), rnd_digest(), rnd_digest(), rnd_digest()};
    uint32_t t5[8], ab[8], cd[8], abcd[8], all[8];
    CHECK(union_tree(TOY, five, t5).empty(), "union tree");
    union_claim(TOY, five[0].data(), five[1].data(), ab); union_claim(TOY, five[2].data(), five[3].data(), cd);
    union_claim(TOY, ab, cd, abcd); union_claim(TOY, abcd, five[4].data(), all);
    CHECK(memcmp(t5, all, 32) == 0, "union tree of five: ((ab)(cd))e");
    CHECK(!union_tree(TOY, {}, t5).empty(), "an empty union tree is refused");
}

static void parent_rules() {
    const NodeClaim l = leaf(7, 11), r = leaf(11, 13), bad = leaf(12, 13);
    NodeClaim p;
    CHECK(parent(TOY, l, r, &p).empty() && p.pre == 7 && p.post == 13, "parent range");
    uint32_t cl[8], cr[8], core[8];
    wrap(TOY, l, cl); wrap(TOY, r, cr); toy(cl, cr, core);
    CHECK(memcmp(core, p.core, 32) == 0, "parent core");
    CHECK(parent(TOY, l, bad, &p) == "claim tree: two neighbouring nodes do not chain (post(l) != pre(r)): no join has a witness for them", "parent's refusal");
    NodeClaim res;
    CHECK(resolved(TOY, l, cr, &res).empty() && res.pre == 7 && res.post == 11, "resolved range");
    toy(cl, cr, core);
    CHECK(memcmp(core, res.core, 32) == 0, "resolved core");
}

static void pair_fold_shape() {
    for (size_t n = 1; n <= 9; n++) {
        // labels instead of hashes: digest = (node id, first leaf, end leaf); every level must be the contiguous 2^L blocks, the odd one last
        size_t level_no = 0;
        const JoinLevel label = [&](const std::vector<Digest>& level, std::vector<Digest>& up) -> std::string {
            level_no++;
            for (size_t k = 0; k < level.size(); k++) {
                const size_t lo = k << (level_no - 1), hi = std::min(n, (k + 1) << (level_no - 1));
                CHECK(level[k][1] == lo && level[k][2] == hi, "pair_fold n=%zu level %zu node %zu covers [%u, %u)", n, level_no, k, level[k][1], level[k][2]);
            }
            CHECK(up.size() == level.size() / 2, "pair_fold: up size");
            for (size_t k = 0; k < up.size(); k++) { up[k] = Digest{}; up[k][1] = level[2 * k][1]; up[k][2] = level[2 * k + 1][2]; }
            return "";
        };
        std::vector<Digest> leaves(n, Digest{}), top;
        for (size_t i = 0; i < n; i++) { leaves[i][1] = (uint32_t)i; leaves[i][2] = (uint32_t)i + 1; }
        CHECK(pair_fold(leaves, 1, label, &top).empty() && top.size() == 1 && top[0][1] == 0 && top[0][2] == n, "pair_fold n=%zu root", n);
        // the two-claim stop gives the root's children
        for (auto& d : leaves) d = rnd_digest();
        std::vector<Digest> root, kids;
        CHECK(pair_fold(leaves, 1, hashed_level(TOY), &root).empty() && pair_fold(leaves, 2, hashed_level(TOY), &kids).empty(), "pair_fold hashed");
        CHECK(kids.size() == std::min<size_t>(n, 2), "pair_fold n=%zu stop 2 leaves %zu claims", n, kids.size());
        if (n >= 2) { Digest r; toy(kids[0].data(), kids[1].data(), r.data()); CHECK(r == root[0], "pair_fold n=%zu: stop 2 is not the root's children", n); }
        else CHECK(kids[0] == leaves[0] && root[0] == leaves[0], "pair_fold n=1");
    }
}

static Levels toy_allowed(size_t k, std::vector<uint32_t>* flat = nullptr) {
    std::vector<uint32_t> roots;
    for (size_t i = 0; i < 8 * k; i++) roots.push_back(rnd());
    Levels levels;
    CHECK(allowed_levels(TOY, roots.data(), k, &levels).empty(), "allowed_levels");
    if (flat) *flat = roots;
    return levels;
}
static void membership() {
    for (size_t k : {1, 7, 16}) {
        std::vector<uint32_t> roots;
        const Levels levels = toy_allowed(k, &roots);
        CHECK(levels.size() == ALLOWED_DEPTH + 1 && levels[0].size() == ALLOWED && levels.back().size() == 1, "allowed tree shape");
        for (size_t i = 0; i < ALLOWED; i++)
            for (int w = 0; w < 8; w++) CHECK(levels[0][i][w] == (i < k ? roots[8 * i + w] : 0u), "allowed leaves: roots, zero padded");
        for (size_t index = 0; index < ALLOWED; index++) {
            std::vector<uint32_t> path{0xAAAAu};                     // appends
            membership_path(levels, index, path);
            CHECK(path.size() == 1 + 9 * ALLOWED_DEPTH && path[0] == 0xAAAAu, "path length");
            Digest cur = levels[0][index];
            for (size_t l = 0; l < ALLOWED_DEPTH; l++) {
                const uint32_t bit = path[1 + 9 * l];
                CHECK(bit == fp_encode((uint32_t)((index >> l) & 1)).v && (bit == fp_encode(0).v || bit == fp_encode(1).v), "direction word");
                Digest nxt;
                if (bit == fp_encode(1).v) toy(&path[2 + 9 * l], cur.data(), nxt.data()); else toy(cur.data(), &path[2 + 9 * l], nxt.data());
                cur = nxt;
            }
            CHECK(cur == levels.back()[0], "k=%zu index %zu: the path does not lead to the top", k, index);
        }
    }
    Levels none;
    CHECK(!allowed_levels(TOY, nullptr, 17, &none).empty(), "17 programs are refused");
}

// ---- node witnesses: word counts and where everything sits ----
static size_t expect_words(const std::vector<uint32_t>& in, size_t at, const uint32_t* want, size_t n, const char* what) {
    CHECK(at + n <= in.size() && (n == 0 || memcmp(&in[at], want, 4 * n) == 0), "node witness: %s at word %zu", what, at);
    return at + n;
}
static void node_witnesses() {
    const Levels allowed = toy_allowed(11);
    const Digest& A = allowed.back()[0];
    std::vector<std::vector<uint32_t>> seals;
    Child ch[3];
    for (size_t k = 0; k < 3; k++) {
        seals.emplace_back(40 + 7 * k);
        for (auto& w : seals.back()) w = rnd();
    }
    for (size_t k = 0; k < 3; k++) { ch[k].seal = seals[k].data(); ch[k].words = seals[k].size(); ch[k].program = (uint32_t)(3 + 4 * k); ch[k].claim = leaf(20 + (uint32_t)k, 21 + (uint32_t)k); }
    auto at_child = [&](const std::vector<uint32_t>& in, size_t at, const Child& c, bool path, bool opening) {
        at = expect_words(in, at, c.seal, c.words, "seal");
        if (path) { std::vector<uint32_t> p; membership_path(allowed, c.program, p); at = expect_words(in, at, p.data(), p.size(), "path"); }
        if (opening) { at = expect_words(in, at, c.claim.core, 8, "opening (core)"); const uint32_t st[2] = {c.claim.pre, c.claim.post}; at = expect_words(in, at, st, 2, "opening (pre, post)"); }
        return at;
    };
    std::vector<uint32_t> in{1, 2, 3};                               // cleared by every call
    NodeClaim got, want, ab;
    size_t at;
    // 0: lift (either family): seal, A; the child's claim
    CHECK(node_witness(TOY, 0, ch, 1, allowed, in, &got).empty(), "lift");
    at = at_child(in, 0, ch[0], false, false); at = expect_words(in, at, A.data(), 8, "allowed root");
    CHECK(at == in.size() && in.size() == 40 + 8 && same(got, ch[0].claim), "lift: %zu words", in.size());
    // 2: lift2: seal, seal, A; parent
    CHECK(node_witness(TOY, 2, ch, 2, allowed, in, &got).empty() && parent(TOY, ch[0].claim, ch[1].claim, &want).empty(), "lift2");
    at = at_child(in, 0, ch[0], false, false); at = at_child(in, at, ch[1], false, false); at = expect_words(in, at, A.data(), 8, "allowed root");
    CHECK(at == in.size() && in.size() == 40 + 47 + 8 && same(got, want), "lift2: %zu words", in.size());
    // 1: join, 3: join3: per child seal, path, opening
    CHECK(node_witness(TOY, 1, ch, 2, allowed, in, &got).empty(), "join");
    at = at_child(in, 0, ch[0], true, true); at = at_child(in, at, ch[1], true, true);
    CHECK(at == in.size() && in.size() == 40 + 47 + 2 * (36 + 10) && same(got, want), "join: %zu words", in.size());
    ab = want;
    CHECK(node_witness(TOY, 3, ch, 3, allowed, in, &got).empty() && parent(TOY, ab, ch[2].claim, &want).empty(), "join3");
    at = at_child(in, 0, ch[0], true, true); at = at_child(in, at, ch[1], true, true); at = at_child(in, at, ch[2], true, true);
    CHECK(at == in.size() && in.size() == 40 + 47 + 54 + 3 * (36 + 10) && same(got, want), "join3: %zu words", in.size());
    // 4: union, both orders: per child seal, path; the swap bit last
    for (int flip = 0; flip < 2; flip++) {
        const Child two[2] = {ch[flip], ch[1 - flip]};
        uint32_t ca[8], cb[8];
        wrap(TOY, two[0].claim, ca); wrap(TOY, two[1].claim, cb);
        bool swap = false;
        CHECK(node_witness(TOY, 4, two, 2, allowed, in, &got).empty() && union_node(TOY, ca, cb, &want, &swap).empty(), "union");
        at = at_child(in, 0, two[0], true, false); at = at_child(in, at, two[1], true, false);
        CHECK(at + 1 == in.size() && in.size() == 40 + 47 + 2 * 36 + 1 && in[at] == fp_encode(swap ? 1u : 0u).v && swap == union_order(ca, cb) && same(got, want) && got.pre == 0 && got.post == 0,
              "union: %zu words, swap %d", in.size(), (int)swap);
        if (flip) { NodeClaim first; const Child back[2] = {ch[0], ch[1]}; std::vector<uint32_t> in2; node_witness(TOY, 4, back, 2, allowed, in2, &first);
                    CHECK(same(first, got) && in2.back() != in.back(), "union: the two orders give one claim and opposite swap bits"); }
    }
    // 5: resolve: the conditional with its opening, the assumption without
    uint32_t cb[8];
    wrap(TOY, ch[1].claim, cb);
    CHECK(node_witness(TOY, 5, ch, 2, allowed, in, &got).empty() && resolved(TOY, ch[0].claim, cb, &want).empty(), "resolve");
    at = at_child(in, 0, ch[0], true, true); at = at_child(in, at, ch[1], true, false);
    CHECK(at == in.size() && in.size() == 40 + 47 + 2 * 36 + 10 && same(got, want) && got.pre == ch[0].claim.pre && got.post == ch[0].claim.post, "resolve: %zu words", in.size());
    // a wrong number of children is refused
    CHECK(!node_witness(TOY, 1, ch, 3, allowed, in, &got).empty() && !node_witness(TOY, 3, ch, 2, allowed, in, &got).empty() && !node_witness(TOY, 6, ch, 2, allowed, in, &got).empty(), "child counts");
}

// ---- Part B: the real hash_pair, header-only (the library's zkh_poseidon2_mix_host is the same permutation over the same tables) ----
static std::vector<uint32_t> p2_rcs, p2_tab;
static std::string real_hash(const uint32_t* a, const uint32_t* b, uint32_t out[8]) {
    uint32_t s[CELLS] = {0};
    memcpy(s, a, 32); memcpy(s + 8, b, 32);
    poseidon2_mix(s, p2_rcs.data(), p2_tab.data());
    memcpy(out, s, 32);
    return "";
}
// the input stream both sides generate (tests/test_session_claim_rules.py stream): Montgomery words are any residues
struct Stream { uint64_t x; uint32_t next() { x = (x * 1103515245ull + 12345ull) & 0x7fffffffull; return (uint32_t)(x % P); } };
static void print_words(const char* key, const uint32_t* w, size_t n) {
    printf("%s =", key);
    for (size_t i = 0; i < n; i++) printf(" %u", w[i]);
    printf("\n");
}
static void part_b() {
    p2_rcs.resize(ROUNDS_TOTAL * CELLS); p2_tab.resize(P2_TAB_WORDS);
    for (int i = 0; i < ROUNDS_TOTAL * CELLS; i++) p2_rcs[i] = fp_encode(ZKH_P2_ROUND_CONSTANTS[i]).v - P;
    CHECK(poseidon2_partial_table(p2_tab.data(), ZKH_P2_ROUND_CONSTANTS, ZKH_P2_M_INT_DIAG), "poseidon2 tables");
    const PairHash H = real_hash;
    char key[96];
    const size_t ms[] = {0, 1, 2, 3, 5};
    std::vector<std::vector<Digest>> assumed;
    for (size_t m : ms) {
        Stream st{200 + m};
        std::vector<Digest> a(m);
        for (auto& d : a) for (auto& w : d) w = st.next();
        assumed.push_back(a);
        if (!m) continue;
        uint32_t u[8];
        CHECK(union_tree(H, a, u).empty(), "union tree");
        snprintf(key, sizeof key, "union m=%zu", m); print_words(key, u, 8);
    }
    for (size_t n : {1, 2, 3, 5, 7, 10}) {
        Stream st{100 + n};
        std::vector<NodeClaim> leaves(n);
        uint32_t state = st.next();
        for (auto& l : leaves) { for (auto& w : l.core) w = st.next(); l.pre = state; state = st.next(); l.post = state; }
        for (size_t ranks = 1; ranks <= (n == 10 ? 2u : 1u); ranks++)
            for (size_t mi = 0; mi < 5; mi++) {
                uint32_t c[8];
                CHECK(session_root_claim(H, leaves, ranks, assumed[mi], c).empty(), "session_root_claim");
                snprintf(key, sizeof key, "root n=%zu ranks=%zu m=%zu", n, ranks, ms[mi]); print_words(key, c, 8);
            }
        // the resolve alone: this tree's first leaf as the conditional, the second assumption set's first claim as the assumption
        NodeClaim res;
        uint32_t c[8];
        CHECK(resolved(H, leaves[0], assumed[1][0].data(), &res).empty() && wrap(H, res, c).empty(), "resolved");
        snprintf(key, sizeof key, "resolved n=%zu", n); print_words(key, c, 8);
    }
    for (size_t m : ms) {                  // no leaves: the union root alone
        if (!m) continue;
        uint32_t c[8];
        CHECK(session_root_claim(H, {}, 1, assumed[m == 5 ? 4 : m], c).empty(), "session_root_claim without leaves");
        snprintf(key, sizeof key, "root n=0 ranks=1 m=%zu", m); print_words(key, c, 8);
    }
    for (size_t k : {1, 7, 16}) {
        Stream st{300 + k};
        std::vector<uint32_t> roots(8 * k);
        for (auto& w : roots) w = st.next();
        Levels levels;
        CHECK(allowed_levels(H, roots.data(), k, &levels).empty(), "allowed_levels");
        for (size_t l = 0; l < levels.size(); l++) {
            std::vector<uint32_t> flat;
            for (auto& d : levels[l]) flat.insert(flat.end(), d.begin(), d.end());
            snprintf(key, sizeof key, "allowed k=%zu level=%zu", k, l); print_words(key, flat.data(), flat.size());
        }
        for (size_t index = 0; index < ALLOWED; index++) {
            std::vector<uint32_t> path;
            membership_path(levels, index, path);
            snprintf(key, sizeof key, "path k=%zu index=%zu", k, index); print_words(key, path.data(), path.size());
        }
    }
}

int main() {
    for (size_t n : {1, 2, 3, 4, 5, 6, 7, 9, 10, 27, 64}) { fold_shape(n, true); fold_shape(n, false); }
    NodeClaim none;
    CHECK(!fold_nodes(TOY, {}, &none).empty(), "an empty fold is refused");
    union_rules();
    parent_rules();
    pair_fold_shape();
    membership();
    node_witnesses();
    part_b();
    printf("claims ok\n");
    return 0;
}
