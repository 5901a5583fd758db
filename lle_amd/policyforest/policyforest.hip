// policyforest.hip -- liblle_policyforest.so: one steps-to-go table per map for many equally shaped maps, built in the same launches,
// and a lookup that answers a whole batch of several maps in one launch (C ABI: include/lle_policyforest.h; INTEGRATION.md section
// 24; DESIGN.md "Forest of steps-to-go tables").
//
// The library touches a batch only through include/lle_hip.h.  For the build it owns ONE lle_batch of n_maps * E environments made
// with lle_batch_create_multi, in which map m owns the environments [m * E, (m + 1) * E), exactly as forest.hip does; a lookup reads
// the caller's batch.  Per map a segment of everything policy.hip keeps: `cap` pool records, depth (u16) and value (u32) per state, a
// table segment, eight u64 counters; after the exploration the level starts of every map and a few words of facts per map.
//   phase A, explore   pf_expand, lle_batch_step, pf_insert, pf_commit per piece: the forest's lock-step level loop (../forest/
//                      forest_core.hpp: the batch, the buffers, roots, seed, the insert over sl::PlainKind) in which a map does not stop
//                      at a goal; pf_commit writes depth and the first value as policy_commit does
//   phase B, relax     pf_expand, lle_batch_step, pf_relax per piece, levels from the deepest to the shallowest, all maps that have not
//                      converged in the same launches; lane k finds its map's level in the level-start array (policyforest_logic.hpp:
//                      relax_work), its successor in the map's table segment, and takes the 32-bit atomicMin of policy_relax
//   lookup             pf_lookup, a lane per environment of the caller's batch: its map's facts, record, hash, find, exactness rule
// A workgroup may straddle maps (E and the caller's environments per map are any numbers): per-map facts are read from memory, a few
// cache lines per map that every lane of the map shares; there is no LDS and no barrier, an idle lane returns at once.
//
// depth and value have the shapes of the forest core's `action` (u16 [n_maps][cap]) and `parent` (u32 [n_maps][cap]), which a table
// without plans has no use for: they ARE those buffers.  The core's seed writes parent 0xFFFFFFFF and action 0 for record 0 -- NO_PLAN
// at depth 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lle_policyforest.h"
#include "../forest/forest_core.hpp"
#include "../forest/forest_logic.hpp"
#include "../policy/policy_logic.hpp"
#include "policyforest_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace fl = lle_forest_logic;
namespace fc = lle_forest_core;
namespace pl = lle_policy_logic;
namespace pfl = lle_policyforest_logic;
using sd::fail;

namespace lle {

struct PfParams : fc::Params {
    uint32_t* value;              // [n_maps][cap]: the core's `parent`
    uint16_t* depth;              // [n_maps][cap]: the core's `action`
    const pfl::MapFacts* facts;   // [n_maps]: phase B
    pfl::MapPass* pass;           // [n_maps]: phase B
    const uint32_t* level_start;  // [n_maps][ls_stride]: phase B
    int64_t ls_stride;
    uint32_t level;               // depth of the states being expanded (all maps walk in lock-step)
    uint32_t relax;               // 0: phase A, the lanes' work comes from `desc`; 1: phase B, from `level_start`
};

struct PfLookupParams {
    sl::KeyView env;        // the caller's batch
    int64_t n_envs, envs_per_map, map_index;
    const uint32_t* pool;
    const uint16_t* depth;
    const uint32_t* value;
    const uint32_t* table;
    const pfl::MapFacts* facts;
    sl::RecordLayout lay;
    uint64_t cap;
    uint32_t table_mask;
    int32_t horizon;
    int32_t* steps_out;     // [n_envs] or nullptr
    uint8_t* actions_out;   // [n_envs][action_stride] or nullptr
    int64_t action_stride;
};

using sd::relaxed_load;

__global__ __launch_bounds__(fc::THREADS) void pf_roots(PfParams p) { fc::roots(p); }

// Record 0 of every map is its reset state at depth 0; a reset state that is a goal starts at (0 << 16) | all-STAY.
__global__ __launch_bounds__(fc::THREADS) void pf_seed(PfParams p) {
    fc::seed<sl::PlainKind>(p, nullptr);
    const int64_t m = fc::lane();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const sl::RecordLayout& r = p.lay;
    const uint32_t* root = p.roots + m * r.n_words;
    if (!sl::anybody_dead(root[r.w_bits], r.A) && sl::is_goal(root[r.w_bits], root[r.w_gems], r, p.collect_gems != 0u, p.G))
        p.value[fl::state_index(m, p.cap, 0)] = pl::pack_value(0u, pl::stay_code(r.A));
}

// Lane k scatters the record of its state into environment k and writes its joint action; phase A counts the available ones.
__global__ __launch_bounds__(fc::THREADS) void pf_expand(PfParams p) {
    const int64_t k = fc::lane();
    if (k >= p.n_lanes) return;
    int64_t map;
    uint64_t item;
    uint32_t first_state;
    bool idle;
    if (p.relax) {
        const pfl::RelaxWork w = pfl::relax_work(k, p.piece, p.E, p.level, p.n_joint, p.facts, p.pass, p.level_start, p.ls_stride);
        map = w.map, item = w.item, first_state = w.first_state, idle = w.idle;
    } else {
        const fl::LaneWork w = fl::lane_work(k, p.piece, p.E, p.desc);
        map = w.map, item = w.item, idle = w.idle;
        first_state = idle ? 0u : p.desc[map].first_state;
    }
    if (idle) {
        p.valid[k] = 0;
        return;
    }
    const uint32_t s = first_state + (uint32_t)(item / p.n_joint);  // < the level's end <= cap
    // (an invalid item leaves environment k as it is: whatever the step makes of it, the kernels behind drop the item)
    const bool valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{fc::pool_segment(p, map), p.cap, s}, k, (uint32_t)(item % p.n_joint));
    p.valid[k] = valid ? 1 : 0;
    if (valid && !p.relax) atomicAdd(&p.counters[fl::counter_index(map, fl::CNT_EXPANDED)], 1ull);
}

// The forest's insert over the plain kind: refused and deadly successors dropped, the rest hashed and probed in the map's segment.
__global__ __launch_bounds__(fc::THREADS) void pf_insert(PfParams p) {
    const int64_t k = fc::lane();
    if (fc::insert_front(p, k)) fc::insert_back(p, sl::PlainKind{}, nullptr, nullptr, k);
}

// Every winner takes a pool index of its map, copies its record, writes its depth and first value, and puts the index where its tag was.
__global__ __launch_bounds__(fc::THREADS) void pf_commit(PfParams p) {
    const int64_t k = fc::lane();
    if (!fc::is_winner(p, k)) return;
    const uint32_t slot = p.win_slot[k];
    const int64_t map = k / p.E;
    unsigned long long* counters = p.counters + fl::counter_index(map, 0);
    const unsigned long long idx = atomicAdd(&counters[fl::CNT_STATES], 1ull);
    if (idx >= (unsigned long long)p.cap) {  // this map's pool is full: no table (the tag stays; later launches return at once)
        atomicMax(&counters[fl::CNT_OVERFLOW], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord rec{p.b, r, k};
    sl::copy_record(p.b, r, k, fc::pool_segment(p, map), p.cap, idx);
    const bool goal = sl::is_goal(rec(r.w_bits), rec(r.w_gems), r, p.collect_gems != 0u, p.G);
    p.depth[fl::state_index(map, p.cap, idx)] = (uint16_t)(p.level + 1u);
    p.value[fl::state_index(map, p.cap, idx)] = goal ? pl::pack_value(0u, pl::stay_code(r.A)) : pl::NO_PLAN;
    p.table[fl::table_base(map, p.slots) + slot] = (uint32_t)idx;
}

// Phase B: lane k finds the successor that lies in environment k in its map's table and offers its value, one step longer, to the
// state it came from.
__global__ __launch_bounds__(fc::THREADS) void pf_relax(PfParams p) {
    const int64_t k = fc::lane();
    if (k >= p.n_lanes || !p.valid[k] || p.b.err[k] != 0) return;  // (an idle lane has valid = 0; refusals were counted by the exploration)
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    if (sl::anybody_dead(me(r.w_bits), r.A)) return;
    const pfl::RelaxWork w = pfl::relax_work(k, p.piece, p.E, p.level, p.n_joint, p.facts, p.pass, p.level_start, p.ls_stride);
    const pfl::MapFacts& f = p.facts[w.map];
    const uint64_t h = sl::hash_record(me, r.n_key);
    auto load = [](const uint32_t* slot) { return *slot; };  // (the table is immutable now)
    const sl::Occupants who{p.b.key(), 0, 0u, p.pool + f.pool_offset, p.cap, p.cap};
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, me); };
    const int64_t succ = pl::table_find(p.table + f.table_offset, (uint32_t)(p.slots - 1), h, load, same_as);
    if (succ == pl::FIND_MISSING) return;
    const uint32_t s = w.first_state + (uint32_t)(w.item / p.n_joint);
    const uint32_t code = (uint32_t)(w.item % p.n_joint);
    uint32_t* value = p.value + f.state_offset;
    bool saturated = false;
    const uint32_t offer = pl::relaxed_value(relaxed_load(&value[(uint32_t)succ]), code, &saturated);
    if (saturated) atomicMax(&p.pass[w.map].saturated, 1u);
    if (offer == pl::NO_PLAN) return;
    if (relaxed_load(&value[s]) <= offer) return;  // (a stale larger value only costs the atomic below)
    if (atomicMin(&value[s], offer) > offer) atomicMax(&p.pass[w.map].changed, 1u);
}

// The hot path: a lane per environment of the caller's batch, inside the segments of the environment's map.
__global__ __launch_bounds__(fc::THREADS) void pf_lookup(PfLookupParams q) {
    const int64_t e = fc::lane();
    if (e >= q.n_envs) return;
    const sl::RecordLayout& r = q.lay;
    auto key = [&](int w) { return sl::env_word(q.env, r, e, w); };  // (read again for the comparison: n_key <= w_gems + 1 words, in cache)
    int32_t answer = pl::ANSWER_DEAD_END;
    uint32_t code = pl::stay_code(r.A);
    // (the map's facts depend on e alone: asked for beside the record's words, not behind them)
    const pfl::MapFacts f = q.facts[pfl::lookup_map(e, q.n_envs, q.envs_per_map, q.map_index)];
    if (!sl::anybody_dead(key(r.w_bits), r.A)) {
        answer = pl::ANSWER_UNKNOWN;
        if (pfl::has_table(f)) {
            const uint64_t h = sl::hash_record(key, r.n_key);
            auto load = [](const uint32_t* slot) { return *slot; };
            const sl::Occupants who{q.env, 0, 0u, q.pool + f.pool_offset, q.cap, f.n_states};
            auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, key); };
            const int64_t s = pl::table_find(q.table + f.table_offset, q.table_mask, h, load, same_as);
            if (s != pl::FIND_MISSING) {
                const uint32_t v = q.value[f.state_offset + (uint32_t)s];
                answer = pfl::map_answer(f, true, v, q.depth[f.state_offset + (uint32_t)s], q.horizon);
                if (answer >= 0) code = pl::value_code(v);
            }
        }
    }
    if (q.steps_out) q.steps_out[e] = answer;
    if (q.actions_out)
        for (int a = 0; a < r.A; a++) {
            q.actions_out[e * q.action_stride + a] = (uint8_t)(code % 5u);
            code /= 5u;
        }
}

}  // namespace lle

// ================================================================================================ host side
using lle::PfLookupParams;
using lle::PfParams;

namespace {

std::atomic<uint32_t> g_launched{0};
enum { K_ROOTS = 0, K_SEED, K_EXPAND, K_INSERT, K_COMMIT, K_RELAX, K_LOOKUP, K_COUNT };
const char* const KERNEL_NAMES[K_COUNT] = {"pf_roots", "pf_seed", "pf_expand", "pf_insert", "pf_commit", "pf_relax", "pf_lookup"};
const fc::Library LIBRARY = {"pf", "lle_policyforest_options", "the policy forest", "state", sl::PlainKind::EXTRA, LLE_POLICY_CAPACITY, 0, 0};

static_assert(LLE_POLICY_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_policy.h and search_logic.hpp disagree");
static_assert(LLE_POLICY_MAX_HORIZON == pl::MAX_HORIZON && LLE_POLICY_UNKNOWN == pl::ANSWER_UNKNOWN && LLE_POLICY_DEAD_END == pl::ANSWER_DEAD_END,
              "include/lle_policy.h and policy_logic.hpp disagree");

// What a lookup keeps about a caller's batch.
struct BatchEntry {
    const lle_batch* batch = nullptr;
    lle_buffer_desc pos{}, beams{};  // as queried: compared at every call
    sl::KeyView view{};
    int64_t n_envs = 0;
    int n_maps = 0;
};

bool same_desc(const lle_buffer_desc& a, const lle_buffer_desc& b) {
    return a.ptr == b.ptr && a.bytes == b.bytes && a.elem_bytes == b.elem_bytes && a.ndim == b.ndim && a.shape[0] == b.shape[0] && a.shape[1] == b.shape[1] &&
           a.stride[0] == b.stride[0] && a.stride[1] == b.stride[1];
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct lle_policyforest : fc::Handle {
    PfParams p{};
    std::vector<uint64_t> fingerprints;  // lle_policy_map_fingerprint of every map
    pfl::MapFacts* d_facts = nullptr;
    pfl::MapPass* d_pass = nullptr;
    uint32_t* d_level_start = nullptr;
    size_t level_start_words = 0;
    pfl::MapPass* h_pass = nullptr;   // pinned: down and up once per pass
    uint32_t* h_root_value = nullptr;  // pinned: the reset states' values, once per build
    // the last build
    bool built = false;
    sl::RecordLayout lay{};
    int32_t horizon = 0;
    std::vector<pfl::MapFacts> facts;    // the source of d_facts
    std::vector<uint32_t> level_start;   // the source of d_level_start
    std::vector<BatchEntry> batches;
};

namespace {

int launch_relax_piece(lle_policyforest* f, const PfParams& p) {
    const dim3 grid = fc::grid_for(p.n_lanes), block(fc::THREADS);
    hipLaunchKernelGGL(lle::pf_expand, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "pf_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(f->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, f->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    hipLaunchKernelGGL(lle::pf_relax, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "pf_relax launch failed");
    g_launched.fetch_or(1u << K_EXPAND | 1u << K_RELAX);
    return LLE_OK;
}

void report(const lle_policyforest* f, const std::vector<int32_t>& complete, const std::vector<int32_t>& passes, const std::vector<int32_t>& root_steps,
            lle_policyforest_result* per_map) {
    for (size_t m = 0; m < (size_t)f->n_maps; m++) {
        const fl::MapProgress& pr = f->maps[m].progress;
        per_map[m].status = pr.status;
        per_map[m].depth_reached = pr.depth_reached;
        per_map[m].n_states = pr.n_states;
        per_map[m].complete = pr.status == 0 ? complete[m] : 0;
        per_map[m].root_steps = root_steps[m];
        per_map[m].passes = passes[m];
        per_map[m].pad = 0;
    }
}

}  // namespace

extern "C" {

const char* lle_policyforest_last_error(void) { return sd::g_error.c_str(); }

void lle_policyforest_free(lle_policyforest* f) {
    if (!f) return;
    fc::close(f);  // (synchronises the stream first)
    {
        sd::DeviceGuard g(f->device);
        (void)hipFree(f->d_facts);
        (void)hipFree(f->d_pass);
        (void)hipFree(f->d_level_start);
        if (f->h_pass) (void)hipHostFree(f->h_pass);
        if (f->h_root_value) (void)hipHostFree(f->h_root_value);
    }
    delete f;
}

lle_policyforest* lle_policyforest_create(const lle_map* const* maps, int n_maps, const lle_policyforest_options* opt) {
    fc::Options o;
    if (!fc::read_options(maps, n_maps, opt, LIBRARY, &o)) return nullptr;
    std::vector<uint64_t> fingerprints((size_t)n_maps);
    for (int m = 0; m < n_maps; m++)
        if (!(fingerprints[(size_t)m] = lle_policy_map_fingerprint(maps[m])))
            return fail(LLE_ERR_ARG, std::string("lle_policy_map_fingerprint: ") + lle_policy_last_error() + " (map " + std::to_string(m) + ")"), nullptr;
    auto* f = new lle_policyforest();
    f->fingerprints = fingerprints;
    const fc::Table tables[2] = {{nullptr, 0}, {nullptr, 0}};
    if (fc::open(f, maps, n_maps, o, LIBRARY, tables, &f->p, lle::pf_roots) != LLE_OK) {
        delete f;
        return nullptr;
    }
    g_launched.fetch_or(1u << K_ROOTS);
    const size_t M = (size_t)n_maps;
    sd::DeviceGuard g(f->device);
    if (hipMalloc(&f->d_facts, M * sizeof(pfl::MapFacts)) != hipSuccess || hipMalloc(&f->d_pass, M * sizeof(pfl::MapPass)) != hipSuccess ||
        hipHostMalloc(&f->h_pass, M * sizeof(pfl::MapPass)) != hipSuccess || hipHostMalloc(&f->h_root_value, M * 4) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating the per-map facts failed");
        lle_policyforest_free(f);
        return nullptr;
    }
    PfParams& p = f->p;
    p.value = f->d_parent;
    p.depth = f->d_action;
    p.facts = f->d_facts;
    p.pass = f->d_pass;
    p.level_start = nullptr;
    p.ls_stride = 0;
    p.level = 0;
    p.relax = 0;
    sd::g_error.clear();
    return f;
}

int lle_policyforest_build(lle_policyforest* f, const lle_policy_args* args, lle_policyforest_result* per_map, lle_policyforest_summary* summary) {
    if (!args || !per_map) return fail(LLE_ERR_NULL, "NULL arguments or results");
    // (the arguments are judged before the handle is looked at: what they refuse they refuse on a machine without a device too)
    if (args->struct_bytes != sizeof(lle_policy_args)) return fail(LLE_ERR_ARG, "lle_policy_args.struct_bytes is not sizeof(lle_policy_args)");
    if (summary && summary->struct_bytes != sizeof(lle_policyforest_summary))
        return fail(LLE_ERR_ARG, "lle_policyforest_summary.struct_bytes is not sizeof(lle_policyforest_summary)");
    if (args->horizon < 0 || args->horizon > LLE_POLICY_MAX_HORIZON) return fail(LLE_ERR_ARG, "horizon must be 0 .. 32767");
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    sd::DeviceGuard g(f->device);
    const bool collect = args->collect_gems != 0;
    PfParams p = f->p;
    fc::begin_run(f, &p, collect);
    const sl::RecordLayout& r = p.lay;
    const size_t M = (size_t)f->n_maps;
    f->built = false;  // (until the end: a failed build leaves no table)
    f->batches.clear();
    std::vector<int32_t> complete(M, 0), passes(M, 0), root_steps(M, LLE_POLICY_UNKNOWN);
    std::vector<std::vector<uint32_t>> starts(M, std::vector<uint32_t>{0u, 1u});  // starts[m][d]: local pool index of map m's first state of depth d
    lle_policyforest_summary sum{};
    sum.struct_bytes = sizeof(lle_policyforest_summary);
    auto leave = [&](int rc) {
        report(f, complete, passes, root_steps, per_map);
        if (summary) *summary = sum;
        return rc;
    };
    const auto t_explore = std::chrono::steady_clock::now();

    // ---- tables, counters and record 0 of every map: the reset state at depth 0, whatever it is (lle_policy_build expands it too)
    for (size_t m = 0; m < M; m++) {
        uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
        std::fill(c, c + fl::N_COUNTERS, 0ull);
        c[fl::CNT_STATES] = 1;
        c[fl::CNT_GOAL] = fl::NO_GOAL;  // (never written: a map does not stop at a goal)
        f->maps[m].progress = fl::fresh_progress(true);
        f->h_desc[m] = fl::level_descriptor(f->maps[m].progress, p.n_joint);
    }
    bool ok = hipMemsetAsync(p.table, 0xFF, M * (size_t)p.slots * 4, f->stream) == hipSuccess &&
              hipMemcpyAsync(p.counters, f->h_counters, M * fl::N_COUNTERS * 8, hipMemcpyHostToDevice, f->stream) == hipSuccess && fc::upload_descriptors(f);
    if (ok) {
        hipLaunchKernelGGL(lle::pf_seed, fc::grid_for(f->n_maps), dim3(fc::THREADS), 0, f->stream, p);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(f->stream) != hipSuccess) return leave(fc::hip_failed(f, "preparing the pools failed"));
    g_launched.fetch_or(1u << K_SEED);

    // ---- phase A: level by level, all maps in lock-step, until every frontier is empty or `horizon` levels are expanded
    const fc::Launch<PfParams> launch = {lle::pf_seed, lle::pf_expand, lle::pf_insert, lle::pf_commit, nullptr, 1u << K_SEED,
                                         1u << K_EXPAND | 1u << K_INSERT | 1u << K_COMMIT, 0u};
    int depth = 0;
    bool any_active = true;
    p.relax = 0u;
    while (depth < args->horizon && any_active) {
        if (depth > 0) {
            for (size_t m = 0; m < M; m++) f->h_desc[m] = fl::level_descriptor(f->maps[m].progress, p.n_joint);
            if (!fc::upload_descriptors(f)) return leave(fc::hip_failed(f, "writing the level's descriptors failed"));
        }
        const uint64_t pieces = fl::piece_count(f->h_desc, f->n_maps, f->E);
        sum.explore_items += (int64_t)fl::level_items(f->h_desc, f->n_maps);
        sum.explore_lanes += (int64_t)pieces * p.n_lanes;
        p.level = (uint32_t)depth;
        for (uint64_t q = 0; q < pieces; q++) {
            p.piece = q;
            if (const int rc = fc::launch_piece(f, p, launch, LIBRARY, g_launched)) {
                (void)hipStreamSynchronize(f->stream);
                return leave(rc);
            }
        }
        if (hipMemcpyAsync(f->h_counters, p.counters, M * fl::N_COUNTERS * 8, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
            hipStreamSynchronize(f->stream) != hipSuccess)
            return leave(fc::hip_failed(f, "reading the level's counters failed"));
        depth++;
        any_active = false;
        for (size_t m = 0; m < M; m++) {
            fc::MapRun& mr = f->maps[m];
            if (!mr.progress.active) continue;
            const uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
            int64_t frontier_new = 0, expanded_new = 0;
            const int fate = fl::advance(mr.progress, c, p.cap, depth, LLE_POLICY_CAPACITY, 0, &frontier_new, &expanded_new);
            if (fate == fl::FATE_STEP_ERROR) {
                sum.step_errors = (int64_t)c[fl::CNT_STEP_ERRORS];
                return leave(fail(LLE_ERR_HIP, "the step refused " + std::to_string(c[fl::CNT_STEP_ERRORS]) + " joint actions their availability masks allow (map " +
                                                   std::to_string(m) + ")"));
            }
            if (fate == fl::FATE_CAPACITY) {  // this map alone has no table
                mr.frontier.assign(1, 1);
                mr.expanded.clear();
                continue;
            }
            mr.frontier.push_back(frontier_new);
            mr.expanded.push_back(expanded_new);
            starts[m].push_back((uint32_t)mr.progress.n_states);
            complete[m] = fate == fl::FATE_EMPTY ? 1 : 0;
            any_active = any_active || mr.progress.active;
        }
    }
    sum.explore_ms = ms_since(t_explore);

    // ---- the facts and level starts of every map, once
    const auto t_relax = std::chrono::steady_clock::now();
    uint32_t deepest = 0;
    f->facts.resize(M);
    for (size_t m = 0; m < M; m++) {
        const fl::MapProgress& pr = f->maps[m].progress;
        f->facts[m] = pfl::make_facts((int64_t)m, p.seg_words, p.cap, p.slots, (uint32_t)pr.n_states, complete[m] != 0, pr.status, (uint32_t)pr.depth_reached);
        deepest = std::max(deepest, f->facts[m].depth_reached);
        f->h_pass[m] = pfl::MapPass{pfl::has_table(f->facts[m]) && f->facts[m].depth_reached > 0u ? 1u : 0u, 0u, 0u, 0u};
    }
    const size_t stride = (size_t)deepest + 2;  // (<= horizon + 2)
    f->level_start.assign(M * stride, 0u);
    for (size_t m = 0; m < M; m++)
        for (size_t d = 0; d < stride; d++)  // (past the map's last level: its state count again, so that such a level is empty)
            f->level_start[m * stride + d] = !pfl::has_table(f->facts[m]) ? 0u : d < starts[m].size() ? starts[m][d] : f->facts[m].n_states;
    if (M * stride > f->level_start_words) {
        (void)hipFree(f->d_level_start);
        f->d_level_start = nullptr;
        f->level_start_words = 0;
        if (hipMalloc(&f->d_level_start, M * stride * 4) != hipSuccess) return leave(fc::hip_failed(f, "allocating the level starts failed"));
        f->level_start_words = M * stride;
    }
    p.level_start = f->d_level_start;
    p.ls_stride = (int64_t)stride;
    if (hipMemcpyAsync(f->d_facts, f->facts.data(), M * sizeof(pfl::MapFacts), hipMemcpyHostToDevice, f->stream) != hipSuccess ||
        hipMemcpyAsync(f->d_level_start, f->level_start.data(), M * stride * 4, hipMemcpyHostToDevice, f->stream) != hipSuccess ||
        hipMemcpyAsync(f->d_pass, f->h_pass, M * sizeof(pfl::MapPass), hipMemcpyHostToDevice, f->stream) != hipSuccess)
        return leave(fc::hip_failed(f, "writing the level starts failed"));

    // ---- phase B: passes over every expanded level, the deepest first, until no map's values move
    p.relax = 1u;
    for (uint32_t top = pfl::relax_depth(f->facts.data(), f->h_pass, f->n_maps); top > 0u; top = pfl::relax_depth(f->facts.data(), f->h_pass, f->n_maps)) {
        for (uint32_t d = top; d-- > 0u;) {
            uint64_t items = 0;
            const uint64_t pieces = pfl::relax_piece_count(f->facts.data(), f->h_pass, f->level_start.data(), (int64_t)stride, f->n_maps, f->E, d, p.n_joint, &items);
            sum.relax_items += (int64_t)items;
            sum.relax_lanes += (int64_t)pieces * p.n_lanes;
            p.level = d;
            for (uint64_t q = 0; q < pieces; q++) {
                p.piece = q;
                if (const int rc = launch_relax_piece(f, p)) {
                    (void)hipStreamSynchronize(f->stream);
                    return leave(rc);
                }
            }
        }
        // (h_pass is read by the levels above on the host only; the device's copy went up before them, in stream order)
        if (hipMemcpyAsync(f->h_pass, f->d_pass, M * sizeof(pfl::MapPass), hipMemcpyDeviceToHost, f->stream) != hipSuccess || hipStreamSynchronize(f->stream) != hipSuccess)
            return leave(fc::hip_failed(f, "reading the pass flags failed"));
        for (size_t m = 0; m < M; m++) {
            pfl::MapPass& mp = f->h_pass[m];
            if (!mp.relaxing) continue;
            passes[m]++;
            if (mp.saturated) return leave(fail(LLE_ERR_UNSUPPORTED, "a shortest plan of more than 65 534 steps: a value does not hold it (map " + std::to_string(m) + ")"));
            pfl::next_pass(mp);
        }
        if (hipMemcpyAsync(f->d_pass, f->h_pass, M * sizeof(pfl::MapPass), hipMemcpyHostToDevice, f->stream) != hipSuccess)
            return leave(fc::hip_failed(f, "writing the pass flags failed"));
    }

    // ---- what a lookup gives for every reset state: value[0] of every map in one strided copy
    if (hipMemcpy2DAsync(f->h_root_value, 4, p.value, (size_t)p.cap * 4, 4, M, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess)
        return leave(fc::hip_failed(f, "reading the reset states' values failed"));
    for (size_t m = 0; m < M; m++) {
        const uint32_t* root = f->roots.data() + m * (size_t)r.n_words;
        root_steps[m] = sl::anybody_dead(root[(size_t)r.w_bits], r.A) ? LLE_POLICY_DEAD_END : pfl::map_answer(f->facts[m], true, f->h_root_value[m], 0u, args->horizon);
    }
    sum.relax_ms = ms_since(t_relax);
    f->valid_items = sum.explore_items + sum.relax_items;
    f->launched_lanes = sum.explore_lanes + sum.relax_lanes;
    f->lay = r;
    f->horizon = args->horizon;
    f->built = true;
    return leave(LLE_OK);
}

int lle_policyforest_stats(const lle_policyforest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) {
    return fc::stats(f, map_index, frontier, expanded, cap);
}

int lle_policyforest_fingerprints(const lle_policyforest* f, uint64_t* out, int cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    for (int m = 0; out && m < std::min<int>(cap, (int)f->n_maps); m++) out[m] = f->fingerprints[(size_t)m];
    return (int)f->n_maps;
}

int lle_policyforest_lookup(lle_policyforest* f, const lle_batch* batch, int map_index, int32_t* steps_out, uint8_t* actions_out, int64_t action_stride, void* stream) {
    if (!f || !batch) return fail(LLE_ERR_NULL, "NULL handle or batch");
    if (!steps_out && !actions_out) return fail(LLE_ERR_NULL, "NULL steps_out and actions_out: nothing to write");
    if (!f->built) return fail(LLE_ERR_ARG, "the handle holds no table: lle_policyforest_build has not run, or it failed");
    if (map_index < -1 || map_index >= f->n_maps)
        return fail(LLE_ERR_ARG, "map_index must be -1 (a batch of all " + std::to_string(f->n_maps) + " maps) or 0 .. " + std::to_string(f->n_maps - 1));
    if (actions_out && action_stride < f->lay.A) return fail(LLE_ERR_ARG, "action_stride is smaller than the number of agents");
    lle_buffer_desc pos{}, beams{};
    if (lle_batch_get_buffer(batch, LLE_BUF_POS, &pos) || lle_batch_get_buffer(batch, LLE_BUF_BEAMS, &beams)) return fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
    BatchEntry* entry = nullptr;
    for (auto& b : f->batches)
        if (b.batch == batch) entry = &b;
    if (entry && !(same_desc(entry->pos, pos) && same_desc(entry->beams, beams))) {  // the address now serves another batch
        f->batches.erase(f->batches.begin() + (entry - f->batches.data()));
        entry = nullptr;
    }
    if (!entry) {
        lle_buffer_desc bits{}, gems{};
        if (lle_batch_get_buffer(batch, LLE_BUF_BITS, &bits) || lle_batch_get_buffer(batch, LLE_BUF_GEMS, &gems)) return fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
        const int64_t n = lle_batch_n_envs(batch);
        if (pos.ndim != 3 || pos.shape[1] != f->lay.A) return fail(LLE_ERR_ARG, "the batch has " + std::to_string(pos.shape[1]) + " agents, the forest's maps " + std::to_string(f->lay.A));
        if (beams.ndim != 2 || beams.shape[1] != f->lay.Lw)
            return fail(LLE_ERR_ARG, "the batch has " + std::to_string(beams.shape[1]) + " beam words, the forest's maps " + std::to_string(f->lay.Lw));
        if (n < 1 || pos.shape[0] != n || beams.shape[0] != n || bits.shape[0] != n || gems.shape[0] != n || pos.elem_bytes != 1 || bits.elem_bytes != 8 ||
            gems.elem_bytes != 4 || beams.elem_bytes != 4 || pos.stride[0] < 2 * f->lay.A || pos.stride[1] < 2 || beams.stride[0] < f->lay.Lw)
            return fail(LLE_ERR_UNSUPPORTED, "the batch's buffers do not have the layout include/lle_hip.h describes");
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, pos.ptr) != hipSuccess) {
            (void)hipGetLastError();
            return fail(LLE_ERR_ARG, "the batch's buffers are not device memory");
        }
        if (attr.device != f->device) return fail(LLE_ERR_ARG, "the batch lives on HIP device " + std::to_string(attr.device) + ", the forest on " + std::to_string(f->device));
        BatchEntry b;
        b.batch = batch;
        b.pos = pos;
        b.beams = beams;
        b.n_envs = n;
        b.n_maps = lle_batch_n_maps(batch);
        b.view = sl::KeyView{static_cast<const uint8_t*>(pos.ptr), static_cast<const uint64_t*>(bits.ptr), static_cast<const uint32_t*>(gems.ptr),
                             static_cast<const uint32_t*>(beams.ptr), pos.stride[0], pos.stride[1], beams.stride[0]};
        if (f->batches.size() >= 64) f->batches.erase(f->batches.begin());  // (a bound, not a policy: entries are a few words)
        f->batches.push_back(b);
        entry = &f->batches.back();
    }
    const int64_t want_maps = map_index < 0 ? f->n_maps : 1;
    if (entry->n_maps != want_maps || entry->n_envs % want_maps != 0)
        return fail(LLE_ERR_ARG, "the batch holds " + std::to_string(entry->n_maps) + " maps, " +
                                     (map_index < 0 ? "the forest " + std::to_string(f->n_maps) + " (map_index = -1 asks for all of them, in the forest's order)"
                                                    : "map_index = " + std::to_string(map_index) + " asks for a batch of that map alone"));
    sd::DeviceGuard g(f->device);
    PfLookupParams q{};
    q.env = entry->view;
    q.n_envs = entry->n_envs;
    q.envs_per_map = entry->n_envs / want_maps;
    q.map_index = map_index;
    q.pool = f->d_pool;
    q.depth = f->d_action;
    q.value = f->d_parent;
    q.table = f->d_table;
    q.facts = f->d_facts;
    q.lay = f->lay;
    q.cap = f->p.cap;
    q.table_mask = (uint32_t)(f->p.slots - 1);
    q.horizon = f->horizon;
    q.steps_out = steps_out;
    q.actions_out = actions_out;
    q.action_stride = action_stride;
    hipLaunchKernelGGL(lle::pf_lookup, fc::grid_for(q.n_envs), dim3(fc::THREADS), 0, reinterpret_cast<hipStream_t>(stream), q);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "pf_lookup launch failed");
    g_launched.fetch_or(1u << K_LOOKUP);
    return LLE_OK;
}

size_t lle_policyforest_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, g_launched.load(), buf, cap); }
size_t lle_policyforest_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, (1u << K_COUNT) - 1u, buf, cap); }

}  // extern "C"
