// session.hip — the session executor: every segment of a session sealed on G devices x K lanes, receipts in index order,
// optionally folded through the P2-JOIN tree to one root receipt, and the verification of what comes out.
//
// Stands in for risc0-zkvm 3.0.3 `ProverServer::prove_session` / `ProverImpl::{prove_segment, lift, join}` (un-vendored:
// /root/reference/Cargo.lock:5418) — what `default_prover().prove(env, elf)` (/root/reference/crates/host/src/lib.rs:137) runs
// after the executor has cut the guest's execution into segments — and for `receipt.verify(image_id)`
// (/root/reference/crates/host/src/bin/cli.rs:103).  Upstream proves the segments of a session in a plain loop on one
// device; segments are independent, so here segment i goes to whichever lane is free next (one shared work
// index over all lanes of all devices: round-robin with work stealing for the short tail), with NO exchange between devices.
// Host code only (threads + the C ABI of this library); one lane = one zkh_ctx (device + stream) + circuit + prover.
//
// Three parts, two of them plain C++ that is unit-tested without a GPU:
//   * scheduler.h — the fold plan and the scheduling state machine (WHAT a lane does next);
//   * claims.h    — the claim rules (what a lift / join / union / resolve node reads and publishes, the fold shapes, the
//                   allowed-programs tree): the prover and the verifiers below take them from there, with hash_pair_host;
//   * this file   — the GPU work and the threads.  zkh_session_prove is a ProveRun taken through its stages in order:
//                   chain_public_inputs, plan_fold, start_scheduler, prepare_preflight, run_lanes (worker / producer threads; a
//                   worker's steps are seal_step and node_step, a node is run_node), write_statistics, join_tree (P2-JOIN).
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include <sys/random.h>

#include "circuit.h"
#include "claims.h"
#include "scheduler.h"

using namespace zkh;
using claims::NodeClaim;

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct Lane {
    int device = 0;
    zkh_ctx* ctx = nullptr;
    zkh_circuit *circuit = nullptr, *join_circuit = nullptr, *rec_circuit = nullptr;
    zkh_prover *prover = nullptr, *join_prover = nullptr;
    std::vector<zkh_rec_program*> programs;
    std::vector<uint32_t> resident_po2;       // sizes whose committed code group this lane's prover keeps in HBM
    // witness source 1 (host preflight): pinned record slots of this lane (zkh_host_alloc), 4 x 2^po2 words each, recycled
    std::vector<uint32_t*> record_slots;
    size_t record_slot_words = 0;
    void close() {
        for (auto p : record_slots) if (ctx) zkh_host_free(ctx, p);
        record_slots.clear(); record_slot_words = 0;
        for (auto p : programs) zkh_rec_program_destroy(p);
        programs.clear();
        if (rec_circuit) zkh_circuit_destroy(rec_circuit);
        rec_circuit = nullptr;
        if (join_prover) zkh_prover_destroy(join_prover);
        if (prover) zkh_prover_destroy(prover);
        if (join_circuit) zkh_circuit_destroy(join_circuit);
        if (circuit) zkh_circuit_destroy(circuit);
        if (ctx) zkh_ctx_destroy(ctx);
        join_prover = prover = nullptr; join_circuit = circuit = nullptr; ctx = nullptr;
    }
};

struct ErrorSlot {
    std::mutex lock;
    std::string first;
    bool set(const char* err, const char* what) {          // takes ownership of err; returns true if there was an error
        if (!err) return false;
        {
            std::lock_guard<std::mutex> lk(lock);
            if (first.empty()) first = std::string(what) + ": " + err;
        }
        zkh_free_error(err);
        return true;
    }
    bool any() { std::lock_guard<std::mutex> lk(lock); return !first.empty(); }
    std::string get() { std::lock_guard<std::mutex> lk(lock); return first; }
};

struct SealFree { void operator()(uint32_t* p) const { zkh_free_seal(p); } };
using SealPtr = std::unique_ptr<uint32_t, SealFree>;                   // a malloc'd seal and its owner
struct CircuitFree { void operator()(zkh_circuit* c) const { zkh_circuit_destroy(c); } };
using CircuitPtr = std::unique_ptr<zkh_circuit, CircuitFree>;
const char* load_host_circuit(const std::vector<uint32_t>& desc, CircuitPtr* out) {     // host-only (no context): verification, claims
    zkh_circuit* c = nullptr;
    ZKH_TRY(zkh_circuit_load(nullptr, desc.data(), desc.size(), &c));
    out->reset(c);
    return nullptr;
}

}  // namespace

struct RecKind { uint32_t join, a, b; };
struct zkh_session {
    std::vector<uint32_t> desc, join_desc, rec_desc;
    std::vector<RecKind> rec_kinds;
    std::vector<std::vector<uint32_t>> rec_roots;                 // control root of program i
    claims::Levels allowed;                                       // levels of the allowed-programs tree (claims.h allowed_levels)
    std::vector<Lane> lanes;
    std::vector<Lane> fold_lanes;        // extra contexts that only lift / join (zkh_session_set_recursion): the fold packs the GPU with more lanes than the seals need
    std::vector<Lane*> rec_lanes;        // lanes + fold_lanes
    size_t lanes_per_device = 0;
    zkh_accumulate_fn accumulate = nullptr;
    void* accumulate_user = nullptr;
    bool resident_code = true;           // built-in circuits: the committed code group of each size stays in HBM per lane
    bool streamed_fold = true;           // join_tree 2: lift2 / join a node the moment its children exist, concurrently with the sealing lanes
    bool chained = false;                // SYN-C sessions: segment i's pre-state = initial + contributions of segments 0 .. i-1 (continuity)
    uint32_t initial_state = 0;          // ... as a canonical residue
    bool has_journal = false;            // SYN-S: the bytes the guest commits (zkh_session_set_journal); unset: the final state word
    std::vector<uint8_t> journal;
    const uint8_t* journal_ptr() const {     // non-NULL also for an EMPTY journal (NULL means "the final state word" downstream)
        static const uint8_t none = 0;
        return !has_journal ? nullptr : journal.empty() ? &none : journal.data();
    }
    int witness_source = 0;              // 0: closed-form generators on the device; 1: sequential host preflight -> compact records -> row fill
    size_t producers_per_lane = 2;       // ... host threads per sealing lane that run the preflight ahead of the seals
    // assumption receipts of the session (zkh_session_set_assumptions): seals of ANOTHER circuit (keccak batches) proven beforehand;
    // join_tree 2 lifts them (family 1), unites them pairwise and resolves the session's root against the union root
    std::vector<uint32_t> assum_desc;
    std::vector<std::vector<uint32_t>> assum_seals;
    std::vector<uint32_t> assum_po2;
    std::vector<std::vector<uint32_t>> assum_roots;    // the assumption circuit's control root at assum_po2[i]
    std::vector<uint32_t> assum_claims;                // 8 words each: the receipts' claim digests (zkh_receipt_claim), in the caller's order
    // the digest a chained SYN-S session's last seal binds beside its journal: Assumptions([Assumption{claim, control root}, ..]) of the
    // receipts above, NULL when the session assumes nothing (verifier.hip assumptions_digest)
    const uint32_t* assumptions_digest(uint32_t out[8]) const {
        if (assum_seals.empty()) return nullptr;
        std::vector<uint32_t> roots;
        for (const auto& r : assum_roots) roots.insert(roots.end(), r.begin(), r.end());
        zkh::assumptions_digest(assum_claims.data(), roots.data(), assum_seals.size(), out);
        return out;
    }
    ~zkh_session() { for (auto& l : fold_lanes) l.close(); for (auto& l : lanes) l.close(); }
};

extern "C" const char* zkh_session_create(const int* devices, size_t n_devices, size_t lanes_per_device, const uint32_t* desc, size_t desc_words,
                                          const uint32_t* join_desc, size_t join_desc_words, zkh_session** out) {
    ZKH_REQUIRE(devices && n_devices && lanes_per_device && desc && desc_words >= 16 && out, "session_create: bad argument");
    ZKH_REQUIRE(!join_desc || (join_desc_words >= 16 && join_desc[13] == 3), "session_create: the join circuit must be a P2-JOIN description (kind 3)");
    std::unique_ptr<zkh_session> s(new zkh_session());
    s->desc.assign(desc, desc + desc_words);
    if (join_desc) s->join_desc.assign(join_desc, join_desc + join_desc_words);
    s->lanes.resize(n_devices * lanes_per_device);
    s->lanes_per_device = lanes_per_device;
    for (size_t i = 0; i < s->lanes.size(); i++) {
        Lane& l = s->lanes[i];
        l.device = devices[i / lanes_per_device];
        ZKH_TRY(zkh_ctx_create(l.device, "poseidon2", &l.ctx));
        ZKH_TRY(zkh_circuit_load(l.ctx, s->desc.data(), s->desc.size(), &l.circuit));
        ZKH_TRY(zkh_prover_create(l.ctx, l.circuit, &l.prover));
        if (join_desc) {
            ZKH_TRY(zkh_circuit_load(l.ctx, s->join_desc.data(), s->join_desc.size(), &l.join_circuit));
            ZKH_TRY(zkh_prover_create(l.ctx, l.join_circuit, &l.join_prover));
        }
    }
    *out = s.release();
    return nullptr;
}
extern "C" void zkh_session_destroy(zkh_session* s) { delete s; }
extern "C" size_t zkh_session_lanes(const zkh_session* s) { return s ? s->lanes.size() : 0; }
extern "C" zkh_circuit* zkh_session_circuit(zkh_session* s, size_t lane, int join) {
    if (!s || lane >= s->lanes.size()) return nullptr;
    return join ? s->lanes[lane].join_circuit : s->lanes[lane].circuit;
}
extern "C" void zkh_session_set_resident_code(zkh_session* s, int on) {
    if (!s) return;
    s->resident_code = on != 0;
    if (!on) for (auto& l : s->lanes) { if (l.prover) zkh_prover_drop_code_cache(l.prover); l.resident_po2.clear(); }
}
extern "C" void zkh_session_set_accumulate(zkh_session* s, zkh_accumulate_fn fn, void* user) {
    if (s) { s->accumulate = fn; s->accumulate_user = user; }
}

// ---- the claim rules live in claims.h; what this file adds is the pair hash (the library's host permutation), the library's
// error convention, and the claims of SEGMENT seals (which need the circuit) ----
static std::string hash_pair_host(const uint32_t* a, const uint32_t* b, uint32_t out[8]) {
    uint32_t st[24] = {0};
    memcpy(st, a, 32); memcpy(st + 8, b, 32);
    if (const char* e = zkh_poseidon2_mix_host(nullptr, nullptr, st, 1)) { const std::string msg(e); zkh_free_error(e); return msg; }
    memcpy(out, st, 32);
    return "";
}
static const claims::PairHash HASH_PAIR = hash_pair_host;
constexpr size_t REC_ALLOWED = claims::ALLOWED;
static const char* claim_err(const std::string& e) { return e.empty() ? nullptr : make_err("%s", e.c_str()); }      // claims.h "" / message -> NULL / heap string

// (receipt claim, pre, post) of a segment seal: SYN-C circuits (kind 1, five outputs) carry their state in out[4] / out[0]
static void leaf_state(const zkh_circuit* c, const uint32_t* seal, NodeClaim* out) {
    const bool chained = circuit_has_state(c);
    out->pre = chained ? seal[4] : 0; out->post = chained ? seal[0] : 0;
}
static const char* leaf_claim(const zkh_circuit* c, const uint32_t* seal, size_t words, const uint32_t* control_root, NodeClaim* out) {
    ZKH_TRY(zkh_receipt_claim(c, seal, words, control_root, nullptr, nullptr, out->core));
    leaf_state(c, seal, out);
    return nullptr;
}
// a lifted assumption receipt publishes wrap(receipt claim, 0, 0)
static const char* lifted_claim(const uint32_t* receipt_claim, claims::Digest* out) {
    NodeClaim nd;
    memcpy(nd.core, receipt_claim, 32);
    return claim_err(claims::wrap(HASH_PAIR, nd, out->data()));
}
// verify one seal under one control root; a refusal is prefixed with whose seal it was
static const char* verify_under(const zkh_circuit* c, const uint32_t* seal, size_t words, const uint32_t* control_root, const std::string& what) {
    const char* e = zkh_verify_segment(c, seal, words, control_root, nullptr, nullptr);
    if (!e) return nullptr;
    const char* out = make_err("%s: %s", what.c_str(), e);
    zkh_free_error(e);
    return out;
}

// `receipt.verify` for a SUCCINCT receipt, on the host alone (no GPU, no session): what zeth_amd/recursion.py RecReceipt.verify does.
static const char* succinct_verify_impl(const uint32_t* root_seal, size_t root_words, const uint32_t* allowed_roots, size_t n_allowed,
                                        size_t root_program, const uint32_t* leaves, size_t n_leaves, size_t ranks,
                                        const uint32_t* assumptions, size_t n_assumptions) {
    ZKH_REQUIRE(root_seal && allowed_roots && (leaves || !n_leaves) && (assumptions || !n_assumptions), "succinct_verify: null argument");
    ZKH_REQUIRE(n_allowed >= 1 && n_allowed <= claims::ALLOWED && root_program < n_allowed, "succinct_verify: the receipt's program is not in the allowed set");
    ZKH_REQUIRE(n_leaves + n_assumptions >= 1, "succinct_verify: neither leaves nor assumptions");
    ZKH_REQUIRE(ranks >= 1 && n_leaves % ranks == 0 && (n_leaves || ranks == 1), "succinct_verify: %zu leaves do not split into %zu equal ranges", n_leaves, ranks);
    ZKH_REQUIRE(root_words > 16, "succinct_verify: not a recursion seal");
    // 1) ONE seal, under the control root of an allowed program
    const uint32_t* rdesc = nullptr;
    size_t rdesc_words = 0;
    ZKH_TRY(zkh_shipped_circuit_desc("recursion", &rdesc, &rdesc_words));
    CircuitPtr rc;
    ZKH_TRY(load_host_circuit(std::vector<uint32_t>(rdesc, rdesc + rdesc_words), &rc));
    ZKH_TRY(verify_under(rc.get(), root_seal, root_words, allowed_roots + 8 * root_program, "succinct_verify: root receipt"));
    // 2) the allowed-programs root the receipt carries is the root of THIS set (16 leaves, zero padded)
    claims::Levels allowed;
    ZKH_TRY(claim_err(claims::allowed_levels(HASH_PAIR, allowed_roots, n_allowed, &allowed)));
    ZKH_REQUIRE(memcmp(root_seal + 8, allowed.back()[0].data(), 32) == 0, "succinct_verify: the receipt was produced under another allowed-programs root");
    // 3) its claim is the root of the leaves' claim tree (`ranks` contiguous equal ranges folded on their own, their roots folded
    //    again), resolved against the assumptions' union tree when there are any
    std::vector<NodeClaim> nodes(n_leaves);
    for (size_t i = 0; i < n_leaves; i++) { memcpy(nodes[i].core, leaves + 10 * i, 32); nodes[i].pre = leaves[10 * i + 8]; nodes[i].post = leaves[10 * i + 9]; }
    std::vector<claims::Digest> lifted(n_assumptions);
    for (size_t i = 0; i < n_assumptions; i++) ZKH_TRY(lifted_claim(assumptions + 8 * i, &lifted[i]));
    uint32_t want[8];
    ZKH_TRY(claim_err(claims::session_root_claim(HASH_PAIR, nodes, ranks, lifted, want)));
    ZKH_REQUIRE(memcmp(root_seal, want, 32) == 0, n_assumptions ? "succinct_verify: the receipt's claim is not the resolved root of the leaves' claim tree and the assumptions' union tree"
                                                                : "succinct_verify: the receipt's claim is not the root of the leaves' claim tree");
    return nullptr;
}
extern "C" const char* zkh_succinct_verify(const uint32_t* root_seal, size_t root_words, const uint32_t* allowed_roots, size_t n_allowed,
                                           size_t root_program, const uint32_t* leaves, size_t n_leaves, size_t ranks) {
    ZKH_REQUIRE(leaves && n_leaves >= 1, "succinct_verify: null argument");
    return succinct_verify_impl(root_seal, root_words, allowed_roots, n_allowed, root_program, leaves, n_leaves, ranks, nullptr, 0);
}
extern "C" const char* zkh_succinct_verify_resolved(const uint32_t* root_seal, size_t root_words, const uint32_t* allowed_roots, size_t n_allowed,
                                                    size_t root_program, const uint32_t* leaves, size_t n_leaves, size_t ranks,
                                                    const uint32_t* assumption_claims, size_t n_assumptions) {
    ZKH_REQUIRE(n_assumptions >= 1, "succinct_verify_resolved: no assumption claims (zkh_succinct_verify checks a receipt without assumptions)");
    return succinct_verify_impl(root_seal, root_words, allowed_roots, n_allowed, root_program, leaves, n_leaves, ranks, assumption_claims, n_assumptions);
}

extern "C" const char* zkh_session_set_recursion(zkh_session* s, const uint32_t* rec_desc, size_t rec_desc_words, const uint32_t* const* blobs,
                                                 const size_t* words, const uint32_t* kinds, size_t n_programs) {
    ZKH_REQUIRE(s && rec_desc && rec_desc_words >= 16 && blobs && words && kinds && n_programs && n_programs <= REC_ALLOWED, "session_set_recursion: bad argument");
    ZKH_REQUIRE(s->rec_kinds.empty() && s->rec_lanes.empty() && s->fold_lanes.empty(), "session_set_recursion: the session already has its programs");
    // Everything is built in locals and committed to the session only when every context, circuit and program has loaded: a
    // failure half way leaves the session exactly as it was (no lane holds a program, no fold lane exists, a retry starts clean).
    std::vector<Lane> fold_lanes;
    struct Loaded { zkh_circuit* circuit = nullptr; std::vector<zkh_rec_program*> programs; };
    std::vector<Loaded> loaded;
    auto undo = [&] {
        for (auto& ld : loaded) { for (auto p : ld.programs) zkh_rec_program_destroy(p); if (ld.circuit) zkh_circuit_destroy(ld.circuit); }
        for (auto& l : fold_lanes) l.close();
    };
#define REC_TRY(expr) do { const char* _e = (expr); if (_e) { undo(); return _e; } } while (0)
    // a lift's / join's witness schedule is a chain of ~300 dependency levels (latency): the fold runs on ZKH_FOLD_LANES lanes
    // per device (default 6: the measured knee, profiles/r03_recursion_fold_lanes.txt), the sealing lanes plus extra contexts
    const char* env = getenv("ZKH_FOLD_LANES");
    const size_t want = env ? (size_t)strtoul(env, nullptr, 10) : 6;
    const size_t n_devices = s->lanes.size() / s->lanes_per_device;
    if (want > s->lanes_per_device) {
        fold_lanes.resize(n_devices * (want - s->lanes_per_device));
        for (size_t i = 0; i < fold_lanes.size(); i++) {
            Lane& l = fold_lanes[i];
            l.device = s->lanes[(i / (want - s->lanes_per_device)) * s->lanes_per_device].device;
            REC_TRY(zkh_ctx_create(l.device, "poseidon2", &l.ctx));
        }
    }
    std::vector<Lane*> rec_lanes;
    for (auto& l : s->lanes) rec_lanes.push_back(&l);
    for (auto& l : fold_lanes) rec_lanes.push_back(&l);
    loaded.resize(rec_lanes.size());
    for (size_t k = 0; k < rec_lanes.size(); k++) {
        REC_TRY(zkh_circuit_load(rec_lanes[k]->ctx, rec_desc, rec_desc_words, &loaded[k].circuit));
        for (size_t i = 0; i < n_programs; i++) {
            zkh_rec_program* p = nullptr;
            REC_TRY(zkh_rec_program_load(rec_lanes[k]->ctx, loaded[k].circuit, blobs[i], words[i], &p));
            loaded[k].programs.push_back(p);
        }
    }
    std::vector<RecKind> rec_kinds;
    std::vector<std::vector<uint32_t>> rec_roots;
    for (size_t i = 0; i < n_programs; i++) {
        rec_kinds.push_back(RecKind{kinds[3 * i], kinds[3 * i + 1], kinds[3 * i + 2]});
        std::vector<uint32_t> root(8);
        REC_TRY(zkh_rec_program_info(loaded[0].programs[i], root.data(), nullptr));
        rec_roots.push_back(root);
    }
    std::vector<uint32_t> flat_roots;
    for (const auto& r : rec_roots) flat_roots.insert(flat_roots.end(), r.begin(), r.end());
    claims::Levels allowed;
    REC_TRY(claim_err(claims::allowed_levels(HASH_PAIR, flat_roots.data(), rec_roots.size(), &allowed)));
#undef REC_TRY
    // ---- commit (nothing below can fail) ----
    s->rec_desc.assign(rec_desc, rec_desc + rec_desc_words);
    s->fold_lanes = std::move(fold_lanes);
    s->rec_lanes.clear();
    for (auto& l : s->lanes) s->rec_lanes.push_back(&l);
    for (auto& l : s->fold_lanes) s->rec_lanes.push_back(&l);
    for (size_t k = 0; k < s->rec_lanes.size(); k++) { s->rec_lanes[k]->rec_circuit = loaded[k].circuit; s->rec_lanes[k]->programs = std::move(loaded[k].programs); }
    s->rec_kinds = std::move(rec_kinds);
    s->rec_roots = std::move(rec_roots);
    s->allowed = std::move(allowed);
    return nullptr;
}
extern "C" const char* zkh_session_set_assumptions(zkh_session* s, const uint32_t* desc, size_t desc_words, const uint32_t* const* seals,
                                                   const size_t* seal_words, const uint32_t* po2s, const uint32_t* control_roots, size_t n) {
    ZKH_REQUIRE(s, "session_set_assumptions: null session");
    if (!n) { s->assum_desc.clear(); s->assum_seals.clear(); s->assum_po2.clear(); s->assum_roots.clear(); s->assum_claims.clear(); return nullptr; }
    ZKH_REQUIRE(desc && desc_words >= 16 && seals && seal_words && po2s && control_roots, "session_set_assumptions: null argument");
    // every receipt is verified HERE, on the host, against the control root it is handed with: what the lifts then prove in-circuit
    CircuitPtr hold;
    ZKH_TRY(load_host_circuit(std::vector<uint32_t>(desc, desc + desc_words), &hold));
    const zkh_circuit* hc = hold.get();
    ZKH_REQUIRE(!circuit_has_state(hc), "session_set_assumptions: an assumption circuit has no state words (its claim' is wrap(claim, 0, 0))");
    std::vector<uint32_t> claims(8 * n);
    for (size_t i = 0; i < n; i++) {
        ZKH_REQUIRE(seals[i] && po2s[i] >= 4 && po2s[i] <= 24, "session_set_assumptions: assumption %zu: bad seal / po2", i);
        ZKH_TRY(verify_under(hc, seals[i], seal_words[i], control_roots + 8 * i, "session_set_assumptions: assumption receipt " + std::to_string(i)));
        ZKH_TRY(zkh_receipt_claim(hc, seals[i], seal_words[i], control_roots + 8 * i, nullptr, nullptr, &claims[8 * i]));
    }
    s->assum_claims = std::move(claims);
    s->assum_desc.assign(desc, desc + desc_words);
    s->assum_seals.clear(); s->assum_po2.assign(po2s, po2s + n); s->assum_roots.clear();
    for (size_t i = 0; i < n; i++) {
        s->assum_seals.emplace_back(seals[i], seals[i] + seal_words[i]);
        s->assum_roots.emplace_back(control_roots + 8 * i, control_roots + 8 * i + 8);
    }
    return nullptr;
}
extern "C" void zkh_session_set_streamed_fold(zkh_session* s, int on) { if (s) s->streamed_fold = on != 0; }
extern "C" const char* zkh_session_set_chained(zkh_session* s, int on, uint32_t initial_state) {
    ZKH_REQUIRE(s, "session_set_chained: null session");
    ZKH_REQUIRE(!on || circuit_has_state(s->lanes[0].circuit),
                "session_set_chained: continuity needs a SYN-C or SYN-S circuit (kind 1 whose first public input is the pre-state)");
    ZKH_REQUIRE(initial_state < P, "session_set_chained: the initial state is not a reduced element");
    s->chained = on != 0; s->initial_state = initial_state;
    return nullptr;
}
extern "C" const char* zkh_session_set_journal(zkh_session* s, const uint8_t* journal, size_t journal_len) {
    ZKH_REQUIRE(s, "session_set_journal: null session");
    ZKH_REQUIRE(!journal || circuit_is_session(s->lanes[0].circuit), "session_set_journal: only a SYN-S circuit binds an output digest");
    ZKH_REQUIRE(journal || !journal_len, "session_set_journal: a length without bytes");
    s->has_journal = journal != nullptr;
    s->journal.assign(journal, journal + (journal ? journal_len : 0));
    return nullptr;
}
extern "C" const char* zkh_session_set_witness_source(zkh_session* s, int source, size_t producers_per_lane) {
    ZKH_REQUIRE(s && (source == 0 || source == 1), "session_set_witness_source: source must be 0 (closed form on the device) or 1 (host preflight)");
    ZKH_REQUIRE(source == 0 || (s->lanes[0].circuit->kind == 1 && s->lanes[0].circuit->global_size[GLOBAL_OUT] == 4),
                "session_set_witness_source: the host preflight drives SYN-AIR circuits (kind 1) without public inputs only");
    s->witness_source = source;
    s->producers_per_lane = producers_per_lane ? producers_per_lane : 2;
    return nullptr;
}

extern "C" void zkh_prove_info_free(zkh_prove_info* info) {
    if (!info) return;
    for (size_t i = 0; i < info->n_segments; i++) if (info->seals) zkh_free_seal(info->seals[i]);
    free(info->seals); free(info->seal_words);
    zkh_free_seal(info->root_seal);
    memset(info, 0, sizeof *info);
}

// control root of the leaf circuit at one segment's size: generated for the built-in circuits, committed from the caller's
// code trace otherwise (a deployment ships these per (circuit, po2): upstream's control IDs)
static const char* leaf_control_root(zkh_session* s, const zkh_segment& seg, uint32_t root[8]) {
    Lane& l = s->lanes[0];
    if (l.circuit->kind >= 1 && l.circuit->kind <= 3) return zkh_syn_control_root(l.prover, seg.po2, ZKH_ZK_CYCLES, root);
    ZKH_REQUIRE(seg.host_code, "session: circuit kind %u has no built-in code generator and the segment carries no code trace", l.circuit->kind);
    Tmp code;
    ZKH_TRY(zkh_copy_from(l.ctx, "code", seg.host_code, (size_t)l.circuit->group_size[GROUP_CODE] << seg.po2, code.out()));
    return zkh_code_root(l.prover, code, seg.po2, root);
}

// The program set of a block whose segments have the sizes `po2s` (largest first), built HERE (rec_builder.hip: no Python, no
// files) and loaded on every lane: a lift per size, a lift2 per pair (a >= b), joins for every pair of program sizes until the set
// closes, the join3 of the largest size if three such children fit that size again (with_join3) — the set and the ORDER of
// zeth_amd/recursion.py build_programs, hence the same allowed-programs root.  Built-in circuits (kinds 1..3): the control roots
// come from their own code generators.
extern "C" const char* zkh_session_build_recursion(zkh_session* s, const uint32_t* po2s, size_t n_po2s, int with_join3) {
    ZKH_REQUIRE(s && po2s && n_po2s >= 1 && n_po2s <= 4, "session_build_recursion: 1..4 segment sizes");
    ZKH_REQUIRE(s->lanes[0].circuit->kind >= 1 && s->lanes[0].circuit->kind <= 3, "session_build_recursion: the segment circuit has no built-in code generator "
                "(build the programs with zkh_rec_build_program from its control roots and use zkh_session_set_recursion)");
    for (size_t k = 1; k < n_po2s; k++) ZKH_REQUIRE(po2s[k] < po2s[k - 1], "session_build_recursion: sizes go largest first, each once");
    std::vector<std::vector<uint32_t>> roots(n_po2s, std::vector<uint32_t>(8));
    for (size_t k = 0; k < n_po2s; k++) {
        zkh_segment seg;
        memset(&seg, 0, sizeof seg);
        seg.po2 = po2s[k];
        ZKH_TRY(leaf_control_root(s, seg, roots[k].data()));
    }
    const uint32_t* rdesc = nullptr;
    size_t rdesc_words = 0;
    ZKH_TRY(zkh_shipped_circuit_desc("recursion", &rdesc, &rdesc_words));
    struct Built { uint32_t kind, a, b; uint32_t* blob; size_t words; };
    std::vector<Built> built;
    struct Free { std::vector<Built>& b; ~Free() { for (auto& x : b) zkh_free_seal(x.blob); } } free_blobs{built};
    std::vector<uint32_t> sizes;
    auto add = [&](uint32_t kind, const uint32_t* d, size_t dw, std::vector<uint32_t> ps, const uint32_t* rts, uint32_t ka, uint32_t kb, uint32_t only_po2 = 0) -> const char* {
        ps.resize(3, 0);
        uint32_t* blob = nullptr;
        size_t words = 0;
        ZKH_TRY(zkh_rec_build_program(kind, d, dw, ps.data(), rts, ZKH_ZK_CYCLES, &blob, &words));
        if (only_po2 && blob[2] != only_po2) { zkh_free_seal(blob); return nullptr; }
        built.push_back({kind, ka, kb, blob, words});
        if (std::find(sizes.begin(), sizes.end(), blob[2]) == sizes.end()) sizes.push_back(blob[2]);
        return nullptr;
    };
    const std::vector<uint32_t>& desc = s->desc;
    for (size_t k = 0; k < n_po2s; k++) ZKH_TRY(add(0, desc.data(), desc.size(), {po2s[k]}, roots[k].data(), po2s[k], 0));
    // the session's assumption receipts (zkh_session_set_assumptions before this call): a lift per size of THEIR circuit (family 1),
    // kept out of the join closure: they meet the session's tree in one resolve
    std::vector<uint32_t> leaf_sizes;                           // program sizes of the assumption lifts
    {
        std::vector<std::pair<uint32_t, const uint32_t*>> asz;  // distinct assumption po2s, largest first, with their control root
        for (size_t i = 0; i < s->assum_po2.size(); i++) {
            bool have = false;
            for (auto& a : asz) {
                if (a.first != s->assum_po2[i]) continue;
                have = true;
                ZKH_REQUIRE(memcmp(a.second, s->assum_roots[i].data(), 32) == 0, "session_build_recursion: two assumption receipts of po2 %u under different control roots", a.first);
            }
            if (!have) asz.emplace_back(s->assum_po2[i], s->assum_roots[i].data());
        }
        std::sort(asz.begin(), asz.end(), [](auto& x, auto& y) { return x.first > y.first; });
        const std::vector<uint32_t> session_sizes(sizes);
        for (auto& a : asz) {
            ZKH_TRY(add(0, s->assum_desc.data(), s->assum_desc.size(), {a.first}, a.second, a.first, 1));
            leaf_sizes.push_back(built.back().blob[2]);
        }
        sizes = session_sizes;                                  // (add() recorded the assumption lifts' sizes: not part of the join closure)
    }
    for (size_t i = 0; i < n_po2s; i++)
        for (size_t j = i; j < n_po2s; j++) {
            std::vector<uint32_t> two(roots[i]);
            two.insert(two.end(), roots[j].begin(), roots[j].end());
            ZKH_TRY(add(2, desc.data(), desc.size(), {po2s[i], po2s[j]}, two.data(), po2s[i], po2s[j]));
        }
    std::vector<std::pair<uint32_t, uint32_t>> done;
    for (bool more = true; more;) {
        more = false;
        std::vector<uint32_t> cur(sizes);
        std::sort(cur.begin(), cur.end());
        for (uint32_t a : cur)
            for (uint32_t b : cur) {
                if (std::find(done.begin(), done.end(), std::make_pair(a, b)) != done.end()) continue;
                done.push_back({a, b});
                ZKH_TRY(add(1, rdesc, rdesc_words, {a, b}, nullptr, a, b));
                more = true;
            }
    }
    if (with_join3 && built.size() < REC_ALLOWED) {
        const uint32_t m = *std::max_element(sizes.begin(), sizes.end());
        ZKH_TRY(add(3, rdesc, rdesc_words, {m, m, m}, nullptr, m, m, m));
    }
    if (!leaf_sizes.empty()) {
        // unions for the pairs the union tree can meet — two leaves, or a union result on the LEFT of anything (an odd node moves up at
        // the END of its level) — until the sizes close; then resolves, the largest session sizes first, as far as the set has room
        const std::vector<uint32_t> session_sizes(sizes);
        std::sort(leaf_sizes.begin(), leaf_sizes.end());
        leaf_sizes.erase(std::unique(leaf_sizes.begin(), leaf_sizes.end()), leaf_sizes.end());
        std::vector<uint32_t> usizes;
        std::vector<std::pair<uint32_t, uint32_t>> udone;
        auto in = [](const std::vector<uint32_t>& v, uint32_t x) { return std::find(v.begin(), v.end(), x) != v.end(); };
        for (bool more = true; more;) {
            more = false;
            std::vector<uint32_t> all(leaf_sizes);
            for (uint32_t u : usizes) if (!in(all, u)) all.push_back(u);
            std::sort(all.begin(), all.end());
            std::vector<std::pair<uint32_t, uint32_t>> todo;      // (decided on the sizes known when the round starts: build_programs' order)
            for (uint32_t a : all)
                for (uint32_t b : all)
                    if (std::find(udone.begin(), udone.end(), std::make_pair(a, b)) == udone.end() && (in(usizes, a) || (in(leaf_sizes, a) && in(leaf_sizes, b))))
                        todo.push_back({a, b});
            for (auto& ab : todo) {
                udone.push_back(ab);
                ZKH_TRY(add(4, rdesc, rdesc_words, {ab.first, ab.second}, nullptr, ab.first, ab.second));
                if (!in(usizes, built.back().blob[2])) usizes.push_back(built.back().blob[2]);
                more = true;
            }
        }
        std::vector<uint32_t> all(leaf_sizes);
        for (uint32_t u : usizes) if (!in(all, u)) all.push_back(u);
        std::sort(all.begin(), all.end());
        std::vector<uint32_t> ss(session_sizes);
        std::sort(ss.begin(), ss.end(), std::greater<uint32_t>());
        for (uint32_t a : ss)
            for (uint32_t b : all) {
                if (built.size() < REC_ALLOWED) ZKH_TRY(add(5, rdesc, rdesc_words, {a, b}, nullptr, a, b));
                else ZKH_REQUIRE(a != ss[0], "session_build_recursion: the allowed set (%zu programs) has no room for resolve(%u, %u): this circuit's lift / lift2 / join "
                                 "programs come in %zu sizes (their join closure alone is %zu programs)%s", REC_ALLOWED, a, b, ss.size(), ss.size() * ss.size(),
                                 with_join3 ? "; pass with_join3 = 0" : ": a circuit this narrow cannot resolve assumptions within one allowed set (the BASELINE widths give two sizes)");
            }
    }
    ZKH_REQUIRE(built.size() <= REC_ALLOWED, "session_build_recursion: %zu programs do not fit the allowed set", built.size());
    std::vector<const uint32_t*> ptrs;
    std::vector<size_t> words;
    std::vector<uint32_t> kinds;
    for (auto& b : built) { ptrs.push_back(b.blob); words.push_back(b.words); kinds.insert(kinds.end(), {b.kind, b.a, b.b}); }
    return zkh_session_set_recursion(s, rdesc, rdesc_words, ptrs.data(), words.data(), kinds.data(), built.size());
}

// control root of the leaf circuit per segment size (po2 -> root): filled through leaf_control_root (lane 0's GPU for the built-in
// circuits) on ONE thread, read without a lock once threads run
struct ControlRoots {
    std::vector<std::pair<uint32_t, claims::Digest>> roots;
    const uint32_t* find(uint32_t po2) const {
        for (const auto& r : roots) if (r.first == po2) return r.second.data();
        return nullptr;
    }
    const char* add(zkh_session* s, const zkh_segment& seg) {          // a size already known costs nothing
        if (find(seg.po2)) return nullptr;
        claims::Digest cr;
        ZKH_TRY(leaf_control_root(s, seg, cr.data()));
        roots.emplace_back(seg.po2, cr);
        return nullptr;
    }
};

// ---- one segment on one lane: the caller's traces through prove_begin / accumulate / prove_finish, or a built-in witness
// generator through zkh_prove_segment.  seal_one allocates what both need. ----
struct SegmentTraces { NoiseKey nk; Tmp code, data; std::vector<uint32_t> out_global; double t0 = 0; };
struct Prepared { const uint32_t* records = nullptr; const uint32_t* ram = nullptr; };   // a producer's preflight output in pinned memory (witness source 1)
struct SealCost { double witgen_s = 0, preflight_cpu_s = 0, trace_bytes = 0; };

static const char* seal_host_traces(zkh_session* s, Lane& l, const zkh_segment& seg, SegmentTraces& t, uint32_t** seal, size_t* words, SealCost* cost) {
    const zkh_circuit* cir = l.circuit;
    ZKH_REQUIRE(seg.host_code && seg.host_data && seg.out_global, "session: a segment with host traces needs host_code, host_data and out_global");
    ZKH_TRY(zkh_write(l.ctx, t.code, seg.host_code, 0, t.code->len));
    ZKH_TRY(zkh_upload_data_trace(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, t.data, seg.host_data, 0));     // without what is derived below
    // what the library derives belongs to the data group: filled before it is committed, callback or not
    ZKH_TRY(zkh_derive_all(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, t.code, t.data));
    // a caller's raw words >= P (and the derives' copies of them) end here: the seal takes reduced words
    ZKH_TRY(zkh_reduce_elem(l.ctx, t.code));
    ZKH_TRY(zkh_reduce_elem(l.ctx, t.data));
    t.out_global.assign(seg.out_global, seg.out_global + t.out_global.size());
    cost->witgen_s = now_s() - t.t0;
    zkh_seal_job* job = nullptr;
    std::vector<uint32_t> mix(cir->global_size[GLOBAL_MIX] ? cir->global_size[GLOBAL_MIX] : 1);
    ZKH_TRY(zkh_prove_begin(l.prover, seg.po2, t.code, t.data, t.out_global.data(), &job, mix.data()));
    Tmp accum;
    const char* err = zkh_alloc(l.ctx, "accum", (size_t)cir->group_size[GROUP_ACCUM] << seg.po2, 0, accum.out());
    if (!err) {
        if (s->accumulate) err = s->accumulate(s->accumulate_user, l.ctx, cir, seg.po2, t.data, mix.data(), accum);
        else if (cir->kind >= 1 && cir->kind <= 3) err = zkh_syn_accum(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, t.nk.k, t.data, mix.data(), accum);
        else if (zkh_circuit_has_arguments(cir)) err = zkh_accumulate(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, t.nk.k, t.code, t.data, mix.data(), accum);
        else err = make_err("session: circuit kind %u has no built-in accum witness generator, no arguments and no accumulate callback was set", cir->kind);
    }
    if (err) { zkh_prove_abort(job); return err; }
    return zkh_prove_finish(job, accum, seal, words);
}

// pre: this segment's preflight output (witness source 1), or empty: run the preflight here (a retry)
static const char* seal_generated(zkh_session* s, Lane& l, const zkh_segment& seg, const Prepared& pre, SegmentTraces& t, uint32_t** seal, size_t* words,
                                  SealCost* cost) {
    const zkh_circuit* cir = l.circuit;
    ZKH_REQUIRE(cir->kind >= 1 && cir->kind <= 3, "session: circuit kind %u has no built-in witness generator: supply host traces", cir->kind);
    // The code (control) group of a built-in circuit is a function of (circuit, po2) alone: commit it once per lane and size and
    // keep the committed form in HBM (seals are byte-identical to the recomputing prover's).  Upstream's
    // SegmentProver re-commits it per segment; zkh_session_set_resident_code(s, 0) does the same.
    if (s->resident_code && cir->kind <= 2) {
        if (std::find(l.resident_po2.begin(), l.resident_po2.end(), seg.po2) == l.resident_po2.end()) {
            ZKH_TRY(zkh_syn_code(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, t.code));
            ZKH_TRY(zkh_prover_cache_code(l.prover, seg.po2, t.code));
            l.resident_po2.push_back(seg.po2);
        }
        t.code.out();                                                // the trace itself is not needed again
    }
    zkh_buf* code_arg = t.code ? (zkh_buf*)t.code : nullptr;
    const uint32_t* noise = t.nk.k;
    if (s->witness_source == 1 && cir->kind == 1) {
        // trace-driven: the compact per-cycle records (16 bytes per cycle) go up from pinned memory, the row fill expands them
        const size_t A = ((size_t)1 << seg.po2) - ZKH_ZK_CYCLES;
        std::vector<uint32_t> inline_records, inline_ram;
        if (!pre.records) {                                           // no producer ran ahead for this one (a retry): preflight here
            inline_records.resize(4 * A); inline_ram.resize(zkh_syn_preflight_ram_words());
            double cpu = 0;
            ZKH_TRY(zkh_syn_preflight(seg.seed, seg.po2, ZKH_ZK_CYCLES, inline_records.data(), inline_ram.data(), &cpu));
            cost->preflight_cpu_s += cpu;
        }
        Tmp recs;
        ZKH_TRY(zkh_alloc(l.ctx, "records", 4 * A, 0, recs.out()));
        if (pre.records) ZKH_TRY(zkh_write_async(l.ctx, recs, pre.records, 0, 4 * A));
        else ZKH_TRY(zkh_write(l.ctx, recs, inline_records.data(), 0, 4 * A));
        cost->trace_bytes += 16.0 * A + 4.0 * zkh_syn_preflight_ram_words() + 4.0 * t.out_global.size();
        ZKH_TRY(zkh_syn_witgen_trace(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, noise, recs, pre.records ? pre.ram : inline_ram.data(), code_arg, t.data, t.out_global.data()));
    } else {
        ZKH_TRY(zkh_syn_witgen(l.ctx, cir, seg.po2, ZKH_ZK_CYCLES, seg.seed, noise, seg.n_pub ? seg.pub : nullptr, code_arg, t.data, t.out_global.data()));
    }
    cost->witgen_s = now_s() - t.t0;
    return zkh_prove_segment(l.prover, seg.po2, ZKH_ZK_CYCLES, noise, code_arg, t.data, t.out_global.data(), seal, words);
}

static const char* seal_one(zkh_session* s, Lane& l, const zkh_segment& seg, const Prepared& pre, uint32_t** seal, size_t* words, SealCost* cost) {
    const zkh_circuit* cir = l.circuit;
    const size_t n = (size_t)1 << seg.po2;
    SegmentTraces t;
    ZKH_TRY(resolve_noise_key(seg.noise_key, &t.nk));     // this segment's blinding key: the caller's, or (all-zero) 256 fresh bits from the OS
    ZKH_TRY(zkh_alloc(l.ctx, "code", (size_t)cir->group_size[GROUP_CODE] * n, 0, t.code.out()));
    ZKH_TRY(zkh_alloc(l.ctx, "data", (size_t)cir->group_size[GROUP_DATA] * n, 0, t.data.out()));
    t.out_global.resize(cir->global_size[GLOBAL_OUT]);
    t.t0 = now_s();
    if (seg.host_code || seg.host_data) return seal_host_traces(s, l, seg, t, seal, words, cost);
    return seal_generated(s, l, seg, pre, t, seal, words, cost);
}

namespace {

// Fault injection (tests of the retry path): ZKH_FAULT_SEGMENT=<i> fails the FIRST attempt at segment i, ZKH_FAULT_SEGMENT_ALWAYS=<i>
// every attempt.  Armed only by a value that parses STRICTLY as a decimal index (an empty or stray variable arms nothing: atol("")
// was 0 = segment 0) and only together with ZKH_TEST_HOOKS=1, which no deployment sets.
long fault_index(const char* name) {
    const char* v = getenv(name);
    const char* armed = getenv("ZKH_TEST_HOOKS");
    if (!v || !*v || !armed || strcmp(armed, "1") != 0) return -1;
    char* end = nullptr;
    const long k = strtol(v, &end, 10);
    return (end && *end == 0 && k >= 0) ? k : -1;
}

const char* node_name(const sched::PlanNode& nd) {
    const uint32_t k = nd.kind;
    return k == 1 ? "join" : k == 3 ? "join3" : k == 2 ? "lift2" : k == 4 ? "union (of two assumption receipts)" : k == 5 ? "resolve (the session's root against its assumptions)"
           : nd.family == 1 ? "lift (of an assumption receipt)" : "lift";
}

// frees the caller's zkh_prove_info on every exit of zkh_session_prove but the successful one
struct InfoGuard {
    zkh_prove_info* info;
    ~InfoGuard() { if (info) zkh_prove_info_free(info); }
    void keep() { info = nullptr; }
};

struct NodeData { SealPtr seal; size_t words = 0; NodeClaim claim; };     // what a proven node leaves for its parent
struct Ready { size_t seg; uint32_t* slot; };
struct LaneQ { std::deque<Ready> ready; std::vector<uint32_t*> free_slots; size_t producers_active = 0; bool accepting = true; };
struct Busy { double wit = 0, seal = 0, fold = 0; };                      // one worker's seconds, added to the run's sums when it leaves

// One call of zkh_session_prove: the state its threads share, and its stages in the order the call takes them.
// Lock discipline: every Scheduler method, every LaneQ and every sum below is touched with m held; GPU work runs with it released.
struct ProveRun {
    zkh_session* const s;
    const zkh_segment* segs;             // the segments as proven (a chained session: with their public inputs)
    const size_t n;
    zkh_prove_info* const info;
    const uint32_t* const join_noise_key;
    const bool fold, streamed, use_pre;
    std::vector<zkh_segment> chained_segs;
    std::vector<uint32_t> pre_states;
    sched::FoldPlan fplan;
    std::vector<NodeData> ndata;
    ControlRoots leaf_roots;             // (the lifts' claims are computed against them)
    ErrorSlot errs;
    std::mutex m;
    std::condition_variable cv;
    std::optional<sched::Scheduler> sc;
    long fault_seg = -1, fault_always = -1;
    std::vector<LaneQ> laneq;
    double t0 = 0, t_end = 0;
    double wit_sum = 0, seal_sum = 0, fold_busy = 0, pre_cpu_sum = 0, trace_bytes_sum = 0;

    ProveRun(zkh_session* s_, const zkh_segment* segs_, size_t n_, int join_tree, const uint32_t* key, zkh_prove_info* info_)
        : s(s_), segs(segs_), n(n_), info(info_), join_noise_key(key), fold(join_tree == 2), streamed(fold && s_->streamed_fold),
          use_pre(s_->witness_source == 1 && s_->lanes[0].circuit->kind == 1), laneq(s_->lanes.size()) {}

    // ---- chained session: the executor's pass.  Every segment's pre-state is fixed BEFORE any segment is proven (one launch over
    // all segments), so the provers stay independent; the pre-state becomes the segment's public input ----
    const char* chain_public_inputs() {
        if (!s->chained) return nullptr;
        std::vector<uint64_t> seeds(n);
        std::vector<uint32_t> po2s(n), contrib(n);
        for (size_t i = 0; i < n; i++) {
            ZKH_REQUIRE(!segs[i].host_code && !segs[i].host_data, "session_prove: a chained session takes segments described by their seed");
            seeds[i] = segs[i].seed; po2s[i] = segs[i].po2;
        }
        ZKH_TRY(zkh_syn_chain_contributions(s->lanes[0].ctx, s->lanes[0].circuit, seeds.data(), po2s.data(), n, ZKH_ZK_CYCLES, contrib.data()));
        // SYN-C: one public word per segment (the pre-state).  SYN-S: 19 — pre-state, the exit code pair (SystemSplit (2, 0) for
        // every segment but the last, Halted(0) (0, 0) for the last) and the 16 limbs of SHA-256(journal), zero except in the last
        // segment; the journal of a session is its final state word (canonical residue, 4 bytes little-endian).
        const bool sess = circuit_is_session(s->lanes[0].circuit);
        const size_t pw = sess ? SESSION_OUT_WORDS - 4 : 1;
        pre_states.assign(n * pw, 0);
        uint32_t state = fp_encode(s->initial_state).v;
        for (size_t i = 0; i < n; i++) { pre_states[i * pw] = state; state = add_mod(state, contrib[i]); }
        if (sess) {
            // ... and WHICH receipts the session assumes: the last seal binds Output{journal, assumptions} (zkh_session_set_assumptions first)
            uint32_t limbs[SESSION_JOURNAL_LIMBS], ad[8];
            if (s->has_journal) session_output_limbs(s->journal_ptr(), s->journal.size(), s->assumptions_digest(ad), limbs);
            else session_journal_limbs(state, s->assumptions_digest(ad), limbs);
            for (size_t i = 0; i < n; i++) {
                const bool is_last = i + 1 == n;
                pre_states[i * pw + 1] = fp_encode(is_last ? EXIT_SYS_HALTED : EXIT_SYS_SPLIT).v;
                if (is_last) memcpy(&pre_states[i * pw + 3], limbs, sizeof limbs);
            }
        }
        chained_segs.assign(segs, segs + n);
        for (size_t i = 0; i < n; i++) { chained_segs[i].pub = &pre_states[i * pw]; chained_segs[i].n_pub = pw; }
        segs = chained_segs.data();
        return nullptr;
    }

    // ---- the fold plan (join_tree 2), fixed before anything runs: the bottom level turns segment receipts into recursion
    // receipts — a pair of segments is ONE proof where the program set has lift2(po2_l, po2_r) for EVERY pair (lift + lift + join
    // fused), else every segment is lifted on its own and the first level above pairs the lifts — and every level above THAT takes
    // three nodes at a time (zeth_amd/recursion.py fold_plan: one join3 where the program set has it for their sizes, else
    // join(join(a, b), c), the same node either way), a remainder of two is a join, of one moves up unchanged.  A node's program
    // follows from its children's sizes, so a missing program is reported here, not after the leaves are sealed.
    // (the plan itself and the scheduling state machine: scheduler.h — plain C++, unit-tested without a GPU) ----
    const char* plan_fold() {
        if (!fold) return nullptr;
        std::vector<uint32_t> seg_po2(n);
        for (size_t i = 0; i < n; i++) seg_po2[i] = segs[i].po2;
        const std::string perr = sched::build_fold_plan(
            seg_po2,
            [&](uint32_t join, uint32_t a, uint32_t b) -> int {
                for (size_t i = 0; i < s->rec_kinds.size(); i++)
                    if (s->rec_kinds[i].join == join && s->rec_kinds[i].a == a && s->rec_kinds[i].b == b) return (int)i;     // lifts: b = circuit family, 0 = the session's
                return -1;
            },
            [&](uint32_t program) { uint32_t inf[8] = {0}; (void)zkh_rec_program_info(s->lanes[0].programs[program], nullptr, inf); return inf[0]; },
            &fplan, s->assum_po2);
        ZKH_REQUIRE(perr.empty(), "session_prove: %s", perr.c_str());
        ndata.resize(fplan.nodes.size());
        // control root of the leaf circuit per segment size: before any thread starts
        for (size_t i = 0; i < n; i++) ZKH_TRY(leaf_roots.add(s, segs[i]));
        return nullptr;
    }

    // ---- one scheduler for the whole call.  Sealing lanes pull segments from one index (round-robin with work stealing over all
    // lanes of all devices; a segment whose seal fails is handed to ANOTHER lane before the session gives up: ZKH_SEGMENT_RETRIES,
    // default 1).  With join_tree 2 a fold node becomes ready the moment its children exist and is proven by whichever lane is
    // free — the fold-only lanes while segments are still being sealed (the witness schedule of a lift / join is a 300-level
    // latency chain that fills the gaps the VALU-bound seals leave), every lane once the segments are done: upstream's
    // join-as-you-go.  zkh_session_set_streamed_fold(s, 0) holds the fold back until the last segment is sealed (two phases). ----
    void start_scheduler() {
        const char* renv = getenv("ZKH_SEGMENT_RETRIES");
        sc.emplace(n, s->lanes.size(), fold ? &fplan : nullptr, streamed, renv ? atoi(renv) : 1);
        fault_seg = fault_index("ZKH_FAULT_SEGMENT"); fault_always = fault_index("ZKH_FAULT_SEGMENT_ALWAYS");
        t0 = now_s();
    }
    bool finished() { return errs.any() || sc->finished(); }                                  // call with m held

    // ---- witness source 1: the sequential host preflight runs AHEAD of the seals.  Every sealing lane has its own producer threads
    // (zkh_session_set_witness_source: default 2 — one preflight of a po2-20 segment is ~70 ms of one core, a lane seals one every
    // ~70 ms) and a pool of pinned record slots (producers + 1): a producer takes the next segment index, replays its cycles into a
    // free slot, and queues (segment, slot) for its lane, which uploads the 16 bytes per cycle and row-fills on the GPU.  The
    // producers are what pull the work index; a lane seals what its producers hand it. ----
    const char* prepare_preflight() {
        if (!use_pre) return nullptr;
        uint32_t max_po2 = 0;
        for (size_t i = 0; i < n; i++) {
            ZKH_REQUIRE(!segs[i].host_code && !segs[i].host_data && !segs[i].n_pub, "session_prove: witness source 1 takes segments described by their seed only");
            max_po2 = std::max(max_po2, segs[i].po2);
        }
        const size_t slot_words = ((size_t)4 << max_po2) + zkh_syn_preflight_ram_words();          // records, then the RAM image
        for (size_t k = 0; k < s->lanes.size(); k++) {
            Lane& l = s->lanes[k];
            if (l.record_slot_words < slot_words) {                             // (main thread: nobody else touches the contexts yet)
                for (auto p : l.record_slots) zkh_host_free(l.ctx, p);
                l.record_slots.clear(); l.record_slot_words = 0;
            }
            while (l.record_slots.size() < s->producers_per_lane + 1) {
                uint32_t* p = nullptr;
                ZKH_TRY(zkh_host_alloc(l.ctx, slot_words, &p));
                l.record_slots.push_back(p);
            }
            l.record_slot_words = slot_words;
            laneq[k].free_slots = l.record_slots;
            laneq[k].producers_active = s->producers_per_lane;
        }
        return nullptr;
    }
    void producer(size_t lane_idx) {
        LaneQ& q = laneq[lane_idx];
        const Lane& l = s->lanes[lane_idx];
        { const char* e = zkh_bind_thread_to_device(l.device, 0, 1, nullptr, nullptr); if (e) zkh_free_error(e); }      // (ZKH_AFFINITY=off: a no-op)
        std::unique_lock<std::mutex> lk(m);
        for (;;) {
            cv.wait(lk, [&] { return errs.any() || !q.accepting || !sc->indices_left() || !q.free_slots.empty(); });
            if (errs.any() || !q.accepting || !sc->indices_left()) break;
            const size_t i = sc->claim_index();
            uint32_t* slot = q.free_slots.back();
            q.free_slots.pop_back();
            lk.unlock();
            double cpu = 0;
            const char* err = zkh_syn_preflight(segs[i].seed, segs[i].po2, ZKH_ZK_CYCLES, slot, slot + ((size_t)4 << segs[i].po2), &cpu);
            lk.lock();
            pre_cpu_sum += cpu;
            if (err) { errs.set(err, "preflight"); q.free_slots.push_back(slot); break; }
            if (q.accepting) q.ready.push_back(Ready{i, slot});
            else { q.free_slots.push_back(slot); sc->requeue(i); }     // the lane stopped sealing meanwhile: anyone may take it
            cv.notify_all();
        }
        q.producers_active--;
        lk.unlock();
        cv.notify_all();
    }

    // A fold node: look up the children, take the witness words and the node's claim from claims.h, prove, release the children's seals
    const char* run_node(Lane* l, size_t id, std::vector<uint32_t>& in) {
        const sched::PlanNode& nd = fplan.nodes[id];
        NodeData& me = ndata[id];
        const size_t ids[3] = {nd.a, nd.b, nd.c}, n_ch = nd.kind == 0 ? 1 : nd.kind == 3 ? 3 : 2;
        const bool of_nodes = nd.kind == 1 || nd.kind >= 3;                // else a lift / lift2: the children are seals of another circuit
        claims::Child ch[3];
        for (size_t k = 0; k < n_ch; k++) {
            const size_t c = ids[k];
            if (of_nodes) {
                ch[k].seal = ndata[c].seal.get(); ch[k].words = ndata[c].words; ch[k].program = fplan.nodes[c].program; ch[k].claim = ndata[c].claim;
            } else if (nd.family == 1) {                                   // an assumption receipt: its receipt claim, no state
                ch[k].seal = s->assum_seals[c].data(); ch[k].words = s->assum_seals[c].size();
                memcpy(ch[k].claim.core, &s->assum_claims[8 * c], 32);
            } else {
                ch[k].seal = info->seals[c]; ch[k].words = info->seal_words[c];
                ZKH_TRY(leaf_claim(s->lanes[0].circuit, info->seals[c], info->seal_words[c], leaf_roots.find(segs[c].po2), &ch[k].claim));
            }
        }
        ZKH_TRY(claim_err(claims::node_witness(HASH_PAIR, nd.kind, ch, n_ch, s->allowed, in, &me.claim)));
        uint32_t* seal = nullptr;
        const char* err = zkh_rec_prove(l->programs[nd.program], in.data(), in.size(), join_noise_key, nullptr, &seal, &me.words);    // NULL: a fresh OS key per proof
        me.seal.reset(seal);
        if (!err && of_nodes) for (size_t k = 0; k < n_ch; k++) ndata[ids[k]].seal.reset();     // children are not kept: the verifier needs the root only
        return err;
    }

    // One segment on this lane.  m is held on entry and on return and released around the GPU work; false: the run has failed.
    bool seal_step(Lane* l, size_t lane_idx, size_t seg, uint32_t* slot, bool* can_seal, Busy* busy, std::unique_lock<std::mutex>& lk) {
        lk.unlock();
        SealCost cost;
        const double ts = now_s();
        const char* err = nullptr;
        if ((long)seg == fault_always || ((long)seg == fault_seg && sc->attempts(seg) == 0)) err = make_err("injected fault (ZKH_FAULT_SEGMENT)");
        else err = seal_one(s, *l, segs[seg], Prepared{slot, slot ? slot + ((size_t)4 << segs[seg].po2) : nullptr}, &info->seals[seg], &info->seal_words[seg], &cost);
        const double te = now_s();
        lk.lock();
        pre_cpu_sum += cost.preflight_cpu_s; trace_bytes_sum += cost.trace_bytes;
        if (slot) {
            // a successful seal ended with a host sync, so the upload from this pinned slot is done; a FAILED one may have returned
            // with the async H2D still in flight: drain the lane's stream before a producer may overwrite the slot
            if (err) { lk.unlock(); if (const char* se = zkh_sync(l->ctx)) zkh_free_error(se); lk.lock(); }
            laneq[lane_idx].free_slots.push_back(slot); cv.notify_all();
        }
        if (!err) {
            busy->wit += cost.witgen_s; busy->seal += te - ts - cost.witgen_s;
            sc->on_seal_done(seg, lane_idx, now_s());
            cv.notify_all();
            return true;
        }
        const sched::Scheduler::Failure f = sc->on_seal_failed(seg, lane_idx, now_s());      // hand it to another lane / device, or give up
        if (f == sched::Scheduler::Failure::Fatal) {
            char what[64];
            snprintf(what, sizeof what, "segment %zu (after %d attempt(s))", seg, sc->attempts(seg));
            errs.set(err, what);
            cv.notify_all();
            return false;
        }
        zkh_free_error(err);
        zkh_free_seal(info->seals[seg]); info->seals[seg] = nullptr; info->seal_words[seg] = 0;
        if (f == sched::Scheduler::Failure::RetryAndRetireLane) {        // two failures in a row: this lane stops taking segments
            *can_seal = false;
            if (use_pre) {                            // what its producers already prepared goes to the other lanes
                LaneQ& q = laneq[lane_idx];
                q.accepting = false;
                for (auto& r : q.ready) { q.free_slots.push_back(r.slot); sc->requeue(r.seg); }
                q.ready.clear();
            }
        }
        cv.notify_all();
        return true;
    }
    // One fold node on this lane, under the same lock contract
    bool node_step(Lane* l, size_t id, std::vector<uint32_t>& in, Busy* busy, std::unique_lock<std::mutex>& lk) {
        lk.unlock();
        const double ts = now_s();
        const char* err = run_node(l, id, in);
        const double te = now_s();
        lk.lock();
        busy->fold += te - ts;
        if (err) errs.set(err, node_name(fplan.nodes[id]));
        else sc->on_node_done(id, now_s());
        cv.notify_all();
        return !err;
    }
    void worker(Lane* l, bool can_seal) {
        const size_t lane_idx = can_seal ? (size_t)(l - s->lanes.data()) : sched::NONE;
        { const char* e = zkh_bind_thread_to_device(l->device, 0, 1, nullptr, nullptr); if (e) zkh_free_error(e); }
        std::vector<uint32_t> in;
        Busy busy;
        std::unique_lock<std::mutex> lk(m);
        while (!finished()) {
            // 1) a segment (scheduler.h take_segment: retries first, then the next index — or, with the host-preflight pipeline, what
            //    this lane's producers have prepared)
            size_t seg = sched::NONE;
            uint32_t* slot = nullptr;
            if (can_seal) {
                seg = sc->take_segment(lane_idx, now_s(), !use_pre).index;
                if (seg == sched::NONE && use_pre) {
                    LaneQ& q = laneq[lane_idx];
                    if (!q.ready.empty()) { seg = q.ready.front().seg; slot = q.ready.front().slot; q.ready.pop_front(); }
                }
            }
            if (seg != sched::NONE) {
                if (!seal_step(l, lane_idx, seg, slot, &can_seal, &busy, lk)) break;
                continue;
            }
            // 2) a fold node (streamed: any time; two phases: once every segment is sealed)
            const sched::Scheduler::Work nw = sc->take_node();
            if (nw.kind == sched::Scheduler::Kind::Node) {
                if (!node_step(l, nw.index, in, &busy, lk)) break;
                continue;
            }
            // 3) nothing to do right now (a retry entry held back for another lane wakes us after 20 ms; producers, finished seals and
            //    finished fold nodes notify)
            if (can_seal && sc->retries_waiting()) cv.wait_for(lk, std::chrono::milliseconds(20));
            else cv.wait(lk);
        }
        sc->lane_leaves(can_seal);
        wit_sum += busy.wit; seal_sum += busy.seal; fold_busy += busy.fold;
        lk.unlock();
        cv.notify_all();
        (void)zkh_sync(l->ctx);
    }
    // one worker per sealing lane, one per fold lane when folding, producers_per_lane producers per lane with witness source 1
    void run_lanes() {
        std::vector<std::thread> th;
        for (auto& lane : s->lanes) th.emplace_back([this, l = &lane] { worker(l, true); });
        if (fold) for (auto& lane : s->fold_lanes) th.emplace_back([this, l = &lane] { worker(l, false); });
        if (use_pre) for (size_t k = 0; k < s->lanes.size(); k++) for (size_t p = 0; p < s->producers_per_lane; p++) th.emplace_back([this, k] { producer(k); });
        for (auto& t : th) t.join();
        t_end = now_s();
    }

    void write_statistics() {
        info->witgen_s_sum = wit_sum; info->seal_s_sum = seal_sum; info->fold_busy_s_sum = fold_busy; info->n_retries = sc->n_retries;
        info->preflight_cpu_s_sum = pre_cpu_sum; info->trace_bytes = trace_bytes_sum;
        info->leaves_s = (sc->t_leaves_done ? sc->t_leaves_done : t_end) - t0;
        if (!fold) return;
        // bottom level = lifts (or lift2 per pair); with the streamed fold these overlap the leaf phase: lift_s / join_s are what the
        // fold still took AFTER the last segment was sealed (bottom level, then joins); two phases: the two phases' durations
        const double tb = std::max(sc->t_bottom_done ? sc->t_bottom_done : t_end, t0 + info->leaves_s);
        info->n_lifts = fplan.n_bottom + fplan.n_assumptions;          // the bottom level + a lift per assumption receipt
        info->n_joins = fplan.nodes.size() - info->n_lifts;            // joins / join3s, unions, the resolve
        info->lift_s = tb - (t0 + info->leaves_s);
        info->join_s = t_end - tb;
        info->fold_tail_s = t_end - (t0 + info->leaves_s);
    }
    void move_root_into_info() {            // every other node seal goes with the run
        NodeData& r = ndata[fplan.root];
        info->root_seal = r.seal.release(); info->root_seal_words = r.words; info->root_program = fplan.nodes[fplan.root].program;
        memcpy(info->root_core, r.claim.core, 32); info->root_pre = r.claim.pre; info->root_post = r.claim.post;
    }

    // ---- the P2-JOIN tree (join_tree 1), after the lanes: claims.h pair_fold gives the shape, a level's joins are proven on one
    // thread per lane; joins below the root are not kept (the verifier does not need them) ----
    std::string join_level(size_t join_po2, const std::vector<claims::Digest>& level, std::vector<claims::Digest>& up) {
        const size_t pairs = up.size();
        std::vector<SealPtr> seals(pairs);
        std::vector<size_t> words(pairs, 0);
        std::atomic<size_t> idx{0};
        std::vector<std::thread> th;
        for (auto& lane : s->lanes)
            th.emplace_back([&, l = &lane] {
                const zkh_circuit* jc = l->join_circuit;
                const size_t jn = (size_t)1 << join_po2;
                Tmp code, data;
                if (errs.set(zkh_alloc(l->ctx, "code", (size_t)jc->group_size[GROUP_CODE] * jn, 0, code.out()), "join alloc") ||
                    errs.set(zkh_alloc(l->ctx, "data", (size_t)jc->group_size[GROUP_DATA] * jn, 0, data.out()), "join alloc")) return;
                uint32_t pub[16], outg[24];
                for (;;) {
                    const size_t k = idx.fetch_add(1);
                    if (k >= pairs || errs.any()) break;
                    memcpy(pub, level[2 * k].data(), 32);
                    memcpy(pub + 8, level[2 * k + 1].data(), 32);
                    NoiseKey jk;
                    if (errs.set(resolve_noise_key(join_noise_key, &jk), "join noise")) break;
                    uint32_t* seal = nullptr;
                    const bool failed = errs.set(zkh_syn_witgen(l->ctx, jc, join_po2, ZKH_ZK_CYCLES, 0, jk.k, pub, code, data, outg), "join witgen") ||
                                        errs.set(zkh_prove_segment(l->join_prover, join_po2, ZKH_ZK_CYCLES, jk.k, code, data, outg, &seal, &words[k]), "join seal");
                    seals[k].reset(seal);
                    if (failed) break;
                    memcpy(up[k].data(), seal, 32);
                }
                (void)zkh_sync(l->ctx);
            });
        for (auto& t : th) t.join();
        if (errs.any()) return errs.get();
        info->n_joins += pairs;
        if (level.size() == 2) { info->root_seal = seals[0].release(); info->root_seal_words = words[0]; }
        return "";
    }
    void join_tree(size_t join_po2) {
        const double tj = now_s();
        std::vector<claims::Digest> leaf_claims(n), root;
        ControlRoots roots;
        for (size_t i = 0; i < n && !errs.any(); i++) {
            if (errs.set(roots.add(s, segs[i]), "control root")) break;
            errs.set(zkh_receipt_claim(s->lanes[0].circuit, info->seals[i], info->seal_words[i], roots.find(segs[i].po2), nullptr, nullptr, leaf_claims[i].data()), "receipt_claim");
        }
        if (!errs.any())          // (a failed level is in errs: the string only stops the fold)
            (void)claims::pair_fold(leaf_claims, 1, [&](const std::vector<claims::Digest>& level, std::vector<claims::Digest>& up) { return join_level(join_po2, level, up); }, &root);
        info->join_s = now_s() - tj;
    }
};

}  // namespace

extern "C" const char* zkh_session_prove(zkh_session* s, const zkh_segment* segs, size_t n, int join_tree, size_t join_po2, const uint32_t* join_noise_key,
                                         zkh_prove_info* info) {
    ZKH_REQUIRE(s && segs && n && info, "session_prove: bad argument");
    ZKH_REQUIRE(join_tree != 1 || !s->join_desc.empty(), "session_prove: the session was created without a join circuit");
    ZKH_REQUIRE(join_tree != 2 || !s->rec_kinds.empty(), "session_prove: join_tree 2 needs zkh_session_set_recursion");
    memset(info, 0, sizeof *info);
    InfoGuard guard{info};                   // from here on every return but the last leaves *info zeroed and owning nothing
    info->n_segments = n;
    info->seals = (uint32_t**)calloc(n, sizeof(uint32_t*));
    info->seal_words = (size_t*)calloc(n, sizeof(size_t));
    ZKH_REQUIRE(info->seals && info->seal_words, "session_prove: out of host memory for %zu receipts", n);
    ZKH_REQUIRE(join_tree != 1 || s->assum_po2.empty(), "session_prove: the session has assumption receipts: they are united and resolved by the RECURSION programs (join_tree 2), the P2-JOIN tree has no such node");
    ProveRun run(s, segs, n, join_tree, join_noise_key, info);
    info->streamed = run.streamed;
    ZKH_TRY(run.chain_public_inputs());
    ZKH_TRY(run.plan_fold());
    run.start_scheduler();
    ZKH_TRY(run.prepare_preflight());
    run.run_lanes();
    run.write_statistics();
    if (run.fold && !run.errs.any()) run.move_root_into_info();
    if (join_tree == 1 && n > 1 && !run.errs.any()) run.join_tree(join_po2);
    info->wall_s = now_s() - run.t0;
    if (run.errs.any()) return make_err("session_prove: %s", run.errs.first.c_str());
    guard.keep();
    return nullptr;
}

// receipt.verify for what zkh_session_prove returned: every leaf seal against the control root of its size, and — when a root
// receipt is present — the root seal against the join circuit's control root plus the claim tree recomputed on the host
// (claims.h).  Host arithmetic only, except that the control roots of the built-in circuits are computed on lane 0 (a deployment
// ships them).
// the segment seals are independent and the verifier is pure host arithmetic on read-only data: spread them over host
// threads (upstream verifies them in a loop; 1024 seals x 7 ms is 7 s on one core)
static const char* verify_leaves(const zkh_circuit* hc, const zkh_segment* segs, const zkh_prove_info* info, const ControlRoots& roots,
                                 std::vector<claims::Digest>& leaf_claims) {
    ErrorSlot verrs;
    std::atomic<size_t> next{0};
    const size_t n_threads = std::max<size_t>(1, std::min<size_t>({(size_t)std::thread::hardware_concurrency(), (size_t)16, info->n_segments}));
    std::vector<std::thread> th;
    for (size_t t = 0; t < n_threads; t++)
        th.emplace_back([&] {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= info->n_segments || verrs.any()) return;
                const uint32_t* root = roots.find(segs[i].po2);
                char what[48];
                snprintf(what, sizeof what, "segment %zu", i);
                if (verrs.set(zkh_verify_segment(hc, info->seals[i], info->seal_words[i], root, nullptr, nullptr), what)) return;
                if (verrs.set(zkh_receipt_claim(hc, info->seals[i], info->seal_words[i], root, nullptr, nullptr, leaf_claims[i].data()), what)) return;
            }
        });
    for (auto& t : th) t.join();
    ZKH_REQUIRE(!verrs.any(), "session_verify: %s", verrs.first.c_str());
    return nullptr;
}
// continuity (CompositeReceipt::verify_integrity): pre == prev.post, read from the verified seals' `out` words
static const char* verify_continuity(zkh_session* s, const zkh_prove_info* info) {
    uint32_t prev = fp_encode(s->initial_state).v;
    for (size_t i = 0; i < info->n_segments; i++) {
        ZKH_REQUIRE(info->seal_words[i] > 5 && info->seals[i][4] == prev, "session_verify: the session is not continuous: segment %zu does not start from its predecessor's post-state", i);
        prev = info->seals[i][0];
    }
    // SYN-S: the session TERMINATES here — every segment but the last says SystemSplit, the last Halted(0) and carries the digest
    // of the journal (= the final state word): a receipt with trailing segments cut off ends in a SystemSplit and is refused
    if (!circuit_is_session(s->lanes[0].circuit)) return nullptr;
    std::vector<const uint32_t*> seals(info->n_segments);
    for (size_t i = 0; i < info->n_segments; i++) {
        ZKH_REQUIRE(info->seal_words[i] > SESSION_OUT_WORDS, "session_verify: segment %zu: seal too short", i);
        seals[i] = info->seals[i];
    }
    uint32_t ad[8];
    return check_session_termination(seals.data(), info->n_segments, s->journal_ptr(), s->journal.size(), s->assumptions_digest(ad));
}
// a RECURSION root: ONE seal under a program of the allowed set, out = claim tree root ‖ allowed-programs root
static const char* verify_recursion_root(zkh_session* s, const zkh_circuit* hc, const zkh_prove_info* info, const std::vector<claims::Digest>& leaf_claims) {
    ZKH_REQUIRE(!s->rec_kinds.empty() && info->root_program < s->rec_roots.size(), "session_verify: a recursion root without the session's programs");
    CircuitPtr rc;
    ZKH_TRY(load_host_circuit(s->rec_desc, &rc));
    ZKH_TRY(verify_under(rc.get(), info->root_seal, info->root_seal_words, s->rec_roots[info->root_program].data(), "session_verify: root receipt"));
    // the claim tree over the leaves (receipt claim + state words of every VERIFIED segment seal), as the lift2 / join programs
    // build it in-circuit, in the shape of the fold plan; a session with assumption receipts (verified when they were handed over)
    // was RESOLVED against the union tree over their lifted claims
    std::vector<NodeClaim> nodes(info->n_segments);
    for (size_t i = 0; i < info->n_segments; i++) { memcpy(nodes[i].core, leaf_claims[i].data(), 32); leaf_state(hc, info->seals[i], &nodes[i]); }
    std::vector<claims::Digest> lifted(s->assum_seals.size());
    for (size_t i = 0; i < lifted.size(); i++) ZKH_TRY(lifted_claim(&s->assum_claims[8 * i], &lifted[i]));
    uint32_t want[8];
    ZKH_TRY(claim_err(claims::session_root_claim(HASH_PAIR, nodes, 1, lifted, want)));
    ZKH_REQUIRE(info->root_seal_words > 16 && memcmp(info->root_seal, want, 32) == 0,
                s->assum_seals.empty() ? "session_verify: the root receipt does not commit to the claim tree of these segments"
                                       : "session_verify: the root receipt does not commit to the claim tree of these segments resolved against the session's assumption receipts");
    ZKH_REQUIRE(memcmp(info->root_seal + 8, s->allowed.back()[0].data(), 32) == 0, "session_verify: the root receipt was produced under another allowed-programs root");
    return nullptr;
}
// a P2-JOIN root: its public inputs are the two children of the root of the pairwise claim tree
static const char* verify_join_root(zkh_session* s, const zkh_prove_info* info, size_t join_po2, const std::vector<claims::Digest>& leaf_claims) {
    ZKH_REQUIRE(!s->join_desc.empty() && info->n_segments > 1, "session_verify: a root receipt without a join circuit");
    CircuitPtr jc;
    ZKH_TRY(load_host_circuit(s->join_desc, &jc));
    uint32_t jroot[8];
    ZKH_TRY(zkh_syn_control_root(s->lanes[0].join_prover, join_po2, ZKH_ZK_CYCLES, jroot));
    ZKH_TRY(verify_under(jc.get(), info->root_seal, info->root_seal_words, jroot, "session_verify: root receipt"));
    std::vector<claims::Digest> top;
    ZKH_TRY(claim_err(claims::pair_fold(leaf_claims, 2, claims::hashed_level(HASH_PAIR), &top)));
    ZKH_REQUIRE(info->root_seal_words > 24 && memcmp(info->root_seal + 8, top[0].data(), 32) == 0 && memcmp(info->root_seal + 16, top[1].data(), 32) == 0,
                "session_verify: the root receipt does not commit to the claim tree of these segments");
    return nullptr;
}

extern "C" const char* zkh_session_verify(zkh_session* s, const zkh_segment* segs, const zkh_prove_info* info, size_t join_po2) {
    ZKH_REQUIRE(s && segs && info && info->n_segments, "session_verify: bad argument");
    CircuitPtr hc;
    ZKH_TRY(load_host_circuit(s->desc, &hc));
    ControlRoots roots;                                       // the control root of every segment size first (lane 0's GPU for built-in circuits)
    for (size_t i = 0; i < info->n_segments; i++) ZKH_TRY(roots.add(s, segs[i]));
    std::vector<claims::Digest> leaf_claims(info->n_segments);
    ZKH_TRY(verify_leaves(hc.get(), segs, info, roots, leaf_claims));
    if (s->chained) ZKH_TRY(verify_continuity(s, info));
    if (!info->root_seal) return nullptr;
    if (info->n_lifts) return verify_recursion_root(s, hc.get(), info, leaf_claims);
    return verify_join_root(s, info, join_po2, leaf_claims);
}
