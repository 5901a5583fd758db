// policy.hip -- liblle_policy.so: the optimal steps-to-go and an optimal joint action of every environment of a batch, from a table
// built once per map through the step kernel of liblle_hip.so (C ABI: include/lle_policy.h; DESIGN.md
// "Steps-to-go table").
//
// The library touches a batch only through include/lle_hip.h.  For the build it owns an lle_batch of `chunk` environments, exactly
// as search.hip does: frontier states are scattered into the batch's five dynamic-state buffers, the batch is stepped with
// lle_batch_step(LLE_STEP_NO_OBS) and the successors are read back out of the same buffers.  A lookup reads the caller's batch.
//
// State: the search's pool (pool[w * max_states + s] = word w of state s) and open-addressing table, and per state depth (u16) and
// value (u32, (steps << 16) | code, policy_logic.hpp).  The states of a level are a contiguous range of the pool; a work item is
// (state, joint action); a level is walked in pieces of at most `chunk` items.
//   phase A, explore   policy_expand, lle_batch_step, policy_insert, policy_commit per piece: the search's walk that does not stop at
//                      a goal; policy_commit also writes the state's depth and its first value (0 | all-STAY for a goal state)
//   phase B, relax     policy_expand, lle_batch_step, policy_relax per piece, levels from the deepest to the shallowest, passes until
//                      one changes nothing: lane k finds its successor in the table, which nobody writes any more, and takes
//                      atomicMin(value[state], (steps(successor) + 1) << 16 | code).  A value only ever falls, so a stale read of a
//                      successor's value costs a pass, never the result; the last pass changes nothing and so has read final values.
//   lookup             policy_lookup, a lane per environment of the caller's batch: record, hash, find, exactness rule, digits
// Global atomics are 32 bits wide throughout; counters that may pass 2^32 are two words with a carry (add64).
//
// The record I/O between a batch, the pool and a table slot (scatter_item, occupant_is, copy_record) is the search's, in
// ../search/search_logic.hpp; error string, device guard, batch binding and the reset state are in ../search/search_device.hpp.  This
// file's own: add64, depth and value, the relaxation, the lookup, the map fingerprint and the cache of callers' batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_policy.h"
#include "../search/search_device.hpp"
#include "policy_logic.hpp"

namespace lle {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace pl = lle_policy_logic;

constexpr int POLICY_THREADS = 256;
// counters: 32-bit words; the *_LO / *_HI pairs are 64-bit counts
enum { CNT_STATES = 0, CNT_OVERFLOW, CNT_CHANGED, CNT_SATURATED, CNT_EXPANDED_LO, CNT_EXPANDED_HI, CNT_ERRORS_LO, CNT_ERRORS_HI, CNT_COUNT };

struct PolicyParams {
    sl::BatchView b;       // the handle's batch (include/lle_hip.h buffer descriptors, read once)
    // the handle
    uint32_t* pool;        // [n_words][max_states]
    uint16_t* depth;       // [max_states]
    uint32_t* value;       // [max_states]
    uint32_t* table;       // [table_mask + 1]
    uint8_t* valid;        // [chunk]
    uint32_t* win_slot;    // [chunk]: the slot candidate k claimed, SLOT_EMPTY when it is no winner
    uint32_t* counters;    // [CNT_COUNT]
    sl::RecordLayout lay;
    uint32_t max_states, table_mask;
    int32_t G;
    uint32_t collect_gems;
    // the piece
    uint32_t first_state;  // pool index of the level's first state
    uint32_t n_joint;      // 5^A
    uint64_t item0;        // first work item of the piece, counted over the level
    uint32_t n_items;      // <= chunk
    uint32_t level;        // depth of the states being expanded
    uint32_t count_expanded;  // phase A: policy_expand counts the available joint actions
};

struct LookupParams {
    sl::KeyView env;       // the caller's batch
    int64_t n_envs;
    const uint32_t* pool;
    const uint16_t* depth;
    const uint32_t* value;
    const uint32_t* table;
    sl::RecordLayout lay;
    uint32_t max_states, table_mask, n_states;
    int32_t horizon, complete;
    int32_t* steps_out;    // [n_envs] or nullptr
    uint8_t* actions_out;  // [n_envs][action_stride] or nullptr
    int64_t action_stride;
};

// counters[lo], counters[lo + 1] += n as one 64-bit count (read only after the launch)
__device__ inline void add64(uint32_t* counters, int lo, uint32_t n) {
    if (n == 0u) return;
    const uint32_t old = atomicAdd(&counters[lo], n);
    if (old + n < old) atomicAdd(&counters[lo + 1], 1u);
}

using sd::relaxed_load;

// search_expand with a block-wide count: lane k scatters the record of its state into environment k and writes its joint action.
__global__ __launch_bounds__(POLICY_THREADS) void policy_expand(PolicyParams p) {
    const uint32_t k = blockIdx.x * POLICY_THREADS + threadIdx.x;
    bool valid = false;
    if (k < p.n_items) {
        const uint64_t item = p.item0 + k;
        const uint32_t s = p.first_state + (uint32_t)(item / p.n_joint);  // < the level's end <= max_states
        // (an invalid item leaves environment k as it is: whatever the step makes of it, the kernels behind drop the item)
        valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{p.pool, p.max_states, s}, k, (uint32_t)(item % p.n_joint));
        p.valid[k] = valid ? 1 : 0;
    }
    if (p.count_expanded) {  // (uniform over the grid: every thread of the block reaches the barrier)
        const int n = __syncthreads_count(valid ? 1 : 0);
        if (threadIdx.x == 0) add64(p.counters, CNT_EXPANDED_LO, (uint32_t)n);
    }
}

// search_insert<false>: lane k drops refused and deadly successors, hashes the rest and probes the table.
__global__ __launch_bounds__(POLICY_THREADS) void policy_insert(PolicyParams p) {
    const uint32_t k = blockIdx.x * POLICY_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    p.win_slot[k] = sl::SLOT_EMPTY;
    if (relaxed_load(&p.counters[CNT_OVERFLOW]) != 0u) return;  // (set by an earlier launch: the build has failed already)
    if (!p.valid[k]) return;
    if (p.b.err[k] != 0) {  // the step refused a joint action the mask allowed
        add64(p.counters, CNT_ERRORS_LO, 1u);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    if (sl::anybody_dead(me(r.w_bits), r.A)) return;
    const uint64_t h = sl::hash_record(me, r.n_key);
    const sl::Occupants who{p.b.key(), 0, p.n_items, p.pool, p.max_states, p.max_states};
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, me); };
    const int64_t slot = sl::table_insert(p.table, p.table_mask, h, sl::TAG_BIT | k, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) p.win_slot[k] = (uint32_t)slot;
    else if (slot == sl::INSERT_FULL) atomicMax(&p.counters[CNT_OVERFLOW], 1u);
}

// Every winner takes a pool index, copies its record, writes its depth and first value, and puts the index where its tag was.
__global__ __launch_bounds__(POLICY_THREADS) void policy_commit(PolicyParams p) {
    const uint32_t k = blockIdx.x * POLICY_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    const uint32_t slot = p.win_slot[k];
    if (slot == sl::SLOT_EMPTY) return;
    const uint32_t idx = atomicAdd(&p.counters[CNT_STATES], 1u);  // (at most max_states + chunk <= 2^31 increments: see lle_policy_build)
    if (idx >= p.max_states) {  // the pool is full: no table (the tag stays; later launches return at once)
        atomicMax(&p.counters[CNT_OVERFLOW], 1u);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    sl::copy_record(p.b, r, k, p.pool, p.max_states, idx);
    const bool goal = sl::is_goal(me(r.w_bits), me(r.w_gems), r, p.collect_gems != 0u, p.G);
    p.depth[idx] = (uint16_t)(p.level + 1u);
    p.value[idx] = goal ? pl::pack_value(0u, pl::stay_code(r.A)) : pl::NO_PLAN;
    p.table[slot] = idx;
}

// Phase B: lane k finds the successor that lies in environment k and offers its value, one step longer, to the state it came from.
__global__ __launch_bounds__(POLICY_THREADS) void policy_relax(PolicyParams p) {
    const uint32_t k = blockIdx.x * POLICY_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    if (!p.valid[k] || p.b.err[k] != 0) return;  // (refusals were counted by the exploration)
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    if (sl::anybody_dead(me(r.w_bits), r.A)) return;
    const uint64_t h = sl::hash_record(me, r.n_key);
    auto load = [](const uint32_t* slot) { return *slot; };  // (the table is immutable now)
    const sl::Occupants who{p.b.key(), 0, 0u, p.pool, p.max_states, p.max_states};
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, me); };
    const int64_t succ = pl::table_find(p.table, p.table_mask, h, load, same_as);
    if (succ == pl::FIND_MISSING) return;
    const uint64_t item = p.item0 + k;
    const uint32_t s = p.first_state + (uint32_t)(item / p.n_joint);
    const uint32_t code = (uint32_t)(item % p.n_joint);
    bool saturated = false;
    const uint32_t offer = pl::relaxed_value(relaxed_load(&p.value[(uint32_t)succ]), code, &saturated);
    if (saturated) atomicMax(&p.counters[CNT_SATURATED], 1u);
    if (offer == pl::NO_PLAN) return;
    if (relaxed_load(&p.value[s]) <= offer) return;  // (a stale larger value only costs the atomic below)
    if (atomicMin(&p.value[s], offer) > offer) atomicMax(&p.counters[CNT_CHANGED], 1u);
}

// The hot path: a lane per environment of the caller's batch.
__global__ __launch_bounds__(POLICY_THREADS) void policy_lookup(LookupParams q) {
    const int64_t e = (int64_t)blockIdx.x * POLICY_THREADS + threadIdx.x;
    if (e >= q.n_envs) return;
    const sl::RecordLayout& r = q.lay;
    auto key = [&](int w) { return sl::env_word(q.env, r, e, w); };  // (read again for the comparison: n_key <= w_gems + 1 words, in cache)
    int32_t answer = pl::ANSWER_DEAD_END;
    uint32_t code = pl::stay_code(r.A);
    if (!sl::anybody_dead(key(r.w_bits), r.A)) {
        answer = pl::ANSWER_UNKNOWN;
        const uint64_t h = sl::hash_record(key, r.n_key);
        auto load = [](const uint32_t* slot) { return *slot; };
        const sl::Occupants who{q.env, 0, 0u, q.pool, q.max_states, q.n_states};
        auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, key); };
        const int64_t s = pl::table_find(q.table, q.table_mask, h, load, same_as);
        if (s != pl::FIND_MISSING) {
            const uint32_t v = q.value[(uint32_t)s];
            answer = pl::answer_of(v, q.depth[(uint32_t)s], q.horizon, q.complete != 0);
            if (answer >= 0) code = pl::value_code(v);
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
using lle::LookupParams;
using lle::PolicyParams;
namespace sl = lle_search_logic;
namespace pl = lle_policy_logic;
namespace sd = lle_search_device;
using sd::DeviceGuard;
using sd::fail;
using sd::g_error;

namespace {

std::atomic<uint32_t> g_launched{0};
constexpr int N_KERNELS = 5;
const char* const KERNEL_NAMES[N_KERNELS] = {"policy_expand", "policy_insert", "policy_commit", "policy_relax", "policy_lookup"};
enum { K_EXPAND = 1u, K_INSERT = 2u, K_COMMIT = 4u, K_RELAX = 8u, K_LOOKUP = 16u };

static_assert(LLE_POLICY_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_policy.h and search_logic.hpp disagree");

// What a lookup keeps about a caller's batch.
struct BatchEntry {
    const lle_batch* batch = nullptr;
    lle_buffer_desc pos{}, beams{};  // as queried: compared at every call
    sl::KeyView view{};
    int64_t n_envs = 0;
};

bool same_desc(const lle_buffer_desc& a, const lle_buffer_desc& b) {
    return a.ptr == b.ptr && a.bytes == b.bytes && a.elem_bytes == b.elem_bytes && a.ndim == b.ndim && a.shape[0] == b.shape[0] && a.shape[1] == b.shape[1] &&
           a.stride[0] == b.stride[0] && a.stride[1] == b.stride[1];
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

struct lle_policy {
    int device = 0;
    hipStream_t stream = nullptr;
    lle_batch* batch = nullptr;
    lle_map_info info{};
    int64_t chunk = 0, max_states = 0;
    uint32_t* d_pool = nullptr;
    uint16_t* d_depth = nullptr;
    uint32_t* d_value = nullptr;
    uint32_t* d_table = nullptr;
    uint8_t* d_valid = nullptr;
    uint32_t* d_win = nullptr;
    uint32_t* d_counters = nullptr;
    std::vector<uint32_t> root;  // the record of the reset state, read from environment 0 right after lle_batch_create
    PolicyParams p{};
    // the last build
    bool built = false;
    sl::RecordLayout lay{};
    int32_t horizon = 0, complete = 0;
    uint32_t n_states = 0;
    std::vector<int64_t> frontier, expanded;
    std::vector<BatchEntry> batches;
};

namespace {

dim3 grid_of(uint32_t n_items) { return dim3((n_items + lle::POLICY_THREADS - 1) / lle::POLICY_THREADS); }

int expand_and_step(lle_policy* s, const PolicyParams& p) {
    hipLaunchKernelGGL(lle::policy_expand, grid_of(p.n_items), dim3(lle::POLICY_THREADS), 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "policy_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(s->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, s->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    return LLE_OK;
}

int explore_piece(lle_policy* s, const PolicyParams& p) {
    const int rc = expand_and_step(s, p);
    if (rc != LLE_OK) return rc;
    hipLaunchKernelGGL(lle::policy_insert, grid_of(p.n_items), dim3(lle::POLICY_THREADS), 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "policy_insert launch failed");
    hipLaunchKernelGGL(lle::policy_commit, grid_of(p.n_items), dim3(lle::POLICY_THREADS), 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "policy_commit launch failed");
    g_launched.fetch_or(K_EXPAND | K_INSERT | K_COMMIT);
    return LLE_OK;
}

int relax_piece(lle_policy* s, const PolicyParams& p) {
    const int rc = expand_and_step(s, p);
    if (rc != LLE_OK) return rc;
    hipLaunchKernelGGL(lle::policy_relax, grid_of(p.n_items), dim3(lle::POLICY_THREADS), 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "policy_relax launch failed");
    g_launched.fetch_or(K_EXPAND | K_RELAX);
    return LLE_OK;
}

// Every piece of the states [level_start, level_end) x every joint action through `piece`.
template <class Piece>
int walk_level(lle_policy* s, PolicyParams& p, uint64_t level_start, uint64_t level_end, uint32_t level, const Piece& piece) {
    const uint64_t total = (level_end - level_start) * (uint64_t)p.n_joint;
    for (uint64_t item0 = 0; item0 < total; item0 += (uint64_t)s->chunk) {
        p.first_state = (uint32_t)level_start;
        p.level = level;
        p.item0 = item0;
        p.n_items = (uint32_t)std::min<uint64_t>((uint64_t)s->chunk, total - item0);
        const int rc = piece(s, p);
        if (rc != LLE_OK) {
            (void)hipStreamSynchronize(s->stream);
            return rc;
        }
    }
    return LLE_OK;
}

int read_counters(lle_policy* s, uint32_t* counters) {
    if (hipMemcpyAsync(counters, s->d_counters, lle::CNT_COUNT * 4, hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "reading the counters failed");
    }
    return LLE_OK;
}

uint64_t pair64(const uint32_t* counters, int lo) { return (uint64_t)counters[lo] | (uint64_t)counters[lo + 1] << 32; }

// FNV-1a over the bytes of 64-bit values, finished with the search's mixer.
struct Fingerprint {
    uint64_t h = 0xCBF29CE484222325ull;
    void add(int64_t v) {
        for (int b = 0; b < 8; b++) {
            h ^= (uint64_t)((uint64_t)v >> (8 * b)) & 255u;
            h *= 0x100000001B3ull;
        }
    }
};

}  // namespace

extern "C" {

const char* lle_policy_last_error(void) { return g_error.c_str(); }

uint64_t lle_policy_map_fingerprint(const lle_map* map) {
    if (!map) {
        fail(LLE_ERR_NULL, "NULL map");
        return 0;
    }
    lle_map_info info{};
    if (lle_map_get_info(map, &info) != LLE_OK) {
        fail(LLE_ERR_ARG, "lle_map_get_info failed");
        return 0;
    }
    Fingerprint f;
    // (what decides a step; not the observation's pitch or the size of the device tables, which a row alignment changes)
    for (int32_t v : {info.height, info.width, info.n_agents, info.n_gems, info.n_sources, info.n_exits, info.n_walls, info.n_voids, info.n_laser_tiles,
                      info.max_beam_len, info.n_beam_words})
        f.add(v);
    for (int which : {LLE_POS_START, LLE_POS_EXIT, LLE_POS_WALL, LLE_POS_VOID, LLE_POS_GEM}) {
        std::vector<int32_t> ij((size_t)2 * std::max(0, lle_map_positions(map, which, nullptr, 0)));
        lle_map_positions(map, which, ij.data(), (int)ij.size() / 2);
        f.add((int64_t)ij.size());
        for (int32_t v : ij) f.add(v);
    }
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    f.add((int64_t)src.size());
    for (const auto& q : src)
        for (int32_t v : {q.i, q.j, q.direction, q.agent_id, q.enabled, q.length, q.laser_id}) f.add(v);
    std::vector<lle_laser_tile> tiles((size_t)std::max(0, lle_map_laser_tiles(map, nullptr, 0)));
    lle_map_laser_tiles(map, tiles.data(), (int)tiles.size());
    f.add((int64_t)tiles.size());
    for (const auto& t : tiles)
        for (int32_t v : {t.i, t.j, t.laser_id, t.offset, t.layer, t.word, t.bit}) f.add(v);
    const uint64_t h = sl::mix64(f.h);
    return h ? h : 1;  // (0 says failure)
}

void lle_policy_free(lle_policy* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    (void)hipStreamSynchronize(s->stream);
    if (s->batch) lle_batch_free(s->batch);
    (void)hipFree(s->d_pool);
    (void)hipFree(s->d_depth);
    (void)hipFree(s->d_value);
    (void)hipFree(s->d_table);
    (void)hipFree(s->d_valid);
    (void)hipFree(s->d_win);
    (void)hipFree(s->d_counters);
    delete s;
}

lle_policy* lle_policy_create(const lle_map* map, const lle_policy_options* opt) {
    if (!map) {
        fail(LLE_ERR_NULL, "NULL map");
        return nullptr;
    }
    if (opt && opt->struct_bytes != sizeof(lle_policy_options)) {
        fail(LLE_ERR_ARG, "lle_policy_options.struct_bytes is not sizeof(lle_policy_options)");
        return nullptr;
    }
    const int64_t chunk = opt && opt->chunk ? opt->chunk : 65536;
    const int64_t max_states = opt && opt->max_states ? opt->max_states : (int64_t)1 << 22;
    if (chunk < 1 || chunk > (int64_t)sl::MAX_CHUNK) {
        fail(LLE_ERR_ARG, "chunk must be 1 .. 2^30");
        return nullptr;
    }
    if (max_states < 1 || max_states > (int64_t)sl::MAX_STATES) {
        fail(LLE_ERR_ARG, "max_states must be 1 .. 2^30");
        return nullptr;
    }
    lle_map_info info{};
    if (lle_map_get_info(map, &info) != LLE_OK) {
        fail(LLE_ERR_ARG, "lle_map_get_info failed");
        return nullptr;
    }
    if (!sd::record_limits_ok(
            info, "more than 6 agents: a state has 5^A joint actions, the table serves maps of at most 6 agents (this map has "))
        return nullptr;
    int device = -1;
    if (sd::choose_device(opt ? opt->device : -1, "no HIP device: the table is built on the GPU only (there is no CPU fallback)", &device) != LLE_OK)
        return nullptr;
    auto* s = new lle_policy();
    s->device = device;
    s->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    s->info = info;
    s->chunk = chunk;
    s->max_states = max_states;
    DeviceGuard g(device);
    s->batch = lle_batch_create(map, chunk, device, nullptr, 0, s->stream);
    if (!s->batch) {
        fail(LLE_ERR_HIP, std::string("lle_batch_create: ") + lle_last_error());
        lle_policy_free(s);
        return nullptr;
    }
    if (sd::bind_batch(s->batch, info, chunk, &s->p.b) != LLE_OK) {
        lle_policy_free(s);
        return nullptr;
    }
    const sl::RecordLayout lay = sl::make_layout(info.n_agents, info.n_beam_words, false);
    const uint64_t slots = sl::table_slots((uint64_t)max_states, (uint64_t)chunk);
    if (hipMalloc(&s->d_pool, (size_t)lay.n_words * (size_t)max_states * 4) != hipSuccess || hipMalloc(&s->d_depth, (size_t)max_states * 2) != hipSuccess ||
        hipMalloc(&s->d_value, (size_t)max_states * 4) != hipSuccess || hipMalloc(&s->d_table, (size_t)slots * 4) != hipSuccess ||
        hipMalloc(&s->d_valid, (size_t)chunk) != hipSuccess || hipMalloc(&s->d_win, (size_t)chunk * 4) != hipSuccess ||
        hipMalloc(&s->d_counters, lle::CNT_COUNT * 4) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating the state pool failed (" + std::to_string((size_t)lay.n_words * (size_t)max_states * 4) + " bytes for " +
                              std::to_string(max_states) + " states of " + std::to_string(lay.n_words) + " words)");
        lle_policy_free(s);
        return nullptr;
    }
    PolicyParams& p = s->p;
    p.pool = s->d_pool;
    p.depth = s->d_depth;
    p.value = s->d_value;
    p.table = s->d_table;
    p.valid = s->d_valid;
    p.win_slot = s->d_win;
    p.counters = s->d_counters;
    p.lay = lay;
    p.max_states = (uint32_t)max_states;
    p.table_mask = (uint32_t)(slots - 1);
    p.G = info.n_gems;
    p.n_joint = sl::pow5(info.n_agents);
    if (sd::read_root(p.b, lay, s->stream, &s->root) != LLE_OK) {  // the batch is freshly reset (World::new calls reset)
        lle_policy_free(s);
        return nullptr;
    }
    g_error.clear();
    return s;
}

int lle_policy_build(lle_policy* s, const lle_policy_args* args, lle_policy_result* result) {
    if (!s || !args || !result) return fail(LLE_ERR_NULL, "NULL handle, arguments or result");
    if (args->struct_bytes != sizeof(lle_policy_args)) return fail(LLE_ERR_ARG, "lle_policy_args.struct_bytes is not sizeof(lle_policy_args)");
    if (result->struct_bytes != sizeof(lle_policy_result)) return fail(LLE_ERR_ARG, "lle_policy_result.struct_bytes is not sizeof(lle_policy_result)");
    if (args->horizon < 0 || args->horizon > LLE_POLICY_MAX_HORIZON) return fail(LLE_ERR_ARG, "horizon must be 0 .. 32767");
    DeviceGuard g(s->device);
    const bool collect = args->collect_gems != 0;
    PolicyParams p = s->p;
    p.lay = sl::make_layout(s->info.n_agents, s->info.n_beam_words, collect);
    p.collect_gems = collect ? 1u : 0u;
    const sl::RecordLayout& r = p.lay;
    const int A = r.A;
    s->built = false;  // (until the end: a failed build leaves no table)
    s->batches.clear();
    s->frontier.assign(1, 1);
    s->expanded.clear();
    result->depth_reached = 0;
    result->n_states = 1;
    result->complete = 0;
    result->passes = 0;
    result->root_steps = LLE_POLICY_UNKNOWN;
    result->pad = 0;
    result->step_errors = 0;
    result->explore_ms = result->relax_ms = 0.0;
    const auto t_explore = std::chrono::steady_clock::now();

    // ---- pool, table and counters: the reset state is state 0, at depth 0
    const std::vector<uint32_t>& root = s->root;
    uint32_t counters[lle::CNT_COUNT] = {};
    counters[lle::CNT_STATES] = 1;
    const bool root_goal = !sl::anybody_dead(root[(size_t)r.w_bits], A) && sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, collect, p.G);
    const uint32_t root_value = root_goal ? pl::pack_value(0u, pl::stay_code(A)) : pl::NO_PLAN;
    const uint16_t zero16 = 0;
    const bool ok = sd::seed_root(p.table, p.table_mask, p.pool, p.max_states, root.data(), r, s->stream) &&
                    hipMemcpyAsync(p.counters, counters, sizeof(counters), hipMemcpyHostToDevice, s->stream) == hipSuccess &&
                    hipMemcpyAsync(p.value, &root_value, 4, hipMemcpyHostToDevice, s->stream) == hipSuccess &&
                    hipMemcpyAsync(p.depth, &zero16, 2, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(s->stream) != hipSuccess) {  // (the sources are stack and handle memory: copied before they change)
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "preparing the pool failed");
    }

    // ---- phase A: level by level until the frontier is empty or `horizon` levels are expanded
    std::vector<uint64_t> level_start(1, 0);  // level_start[d] = pool index of the first state of depth d; one entry more than levels
    level_start.push_back(1);
    uint64_t expanded_before = 0;
    int depth = 0;
    p.count_expanded = 1u;
    while (depth < args->horizon && level_start[(size_t)depth + 1] > level_start[(size_t)depth]) {
        int rc = walk_level(s, p, level_start[(size_t)depth], level_start[(size_t)depth + 1], (uint32_t)depth, explore_piece);
        if (rc != LLE_OK) return rc;
        if ((rc = read_counters(s, counters)) != LLE_OK) return rc;
        depth++;
        result->depth_reached = depth;
        result->step_errors = (int64_t)pair64(counters, lle::CNT_ERRORS_LO);
        const uint64_t expanded_now = pair64(counters, lle::CNT_EXPANDED_LO);
        s->expanded.push_back((int64_t)(expanded_now - expanded_before));
        expanded_before = expanded_now;
        if (counters[lle::CNT_OVERFLOW] != 0u || counters[lle::CNT_STATES] > p.max_states) {
            result->n_states = s->max_states;
            s->frontier.assign(1, 1);
            s->expanded.clear();
            return fail(LLE_POLICY_CAPACITY, "more than max_states = " + std::to_string(s->max_states) + " distinct states at depth " + std::to_string(depth) +
                                                 ": there is no table; create the handle with a larger max_states");
        }
        if (result->step_errors != 0)
            return fail(LLE_ERR_HIP, "the step refused " + std::to_string(result->step_errors) + " joint actions their availability masks allow");
        const uint64_t new_end = counters[lle::CNT_STATES];
        s->frontier.push_back((int64_t)(new_end - level_start[(size_t)depth]));
        level_start.push_back(new_end);
        result->n_states = (int64_t)new_end;
    }
    const bool complete = level_start[(size_t)depth + 1] == level_start[(size_t)depth];
    result->complete = complete ? 1 : 0;
    result->explore_ms = ms_since(t_explore);

    // ---- phase B: every expanded level, the deepest first, until a pass changes nothing
    const auto t_relax = std::chrono::steady_clock::now();
    p.count_expanded = 0u;
    for (bool changed = depth > 0; changed;) {
        for (int d = depth - 1; d >= 0; d--) {
            const int rc = walk_level(s, p, level_start[(size_t)d], level_start[(size_t)d + 1], (uint32_t)d, relax_piece);
            if (rc != LLE_OK) return rc;
        }
        const int rc = read_counters(s, counters);
        if (rc != LLE_OK) return rc;
        result->passes++;
        if (counters[lle::CNT_SATURATED] != 0u) return fail(LLE_ERR_UNSUPPORTED, "a shortest plan of more than 65 534 steps: a value does not hold it");
        changed = counters[lle::CNT_CHANGED] != 0u;
        if (changed && (hipMemsetAsync(p.counters + lle::CNT_CHANGED, 0, 4, s->stream) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(LLE_ERR_HIP, "clearing the pass counter failed");
        }
    }
    uint32_t v0 = pl::NO_PLAN;
    if (hipMemcpyAsync(&v0, p.value, 4, hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "reading the reset state's value failed");
    }
    result->relax_ms = ms_since(t_relax);
    result->root_steps = sl::anybody_dead(root[(size_t)r.w_bits], A) ? LLE_POLICY_DEAD_END : pl::answer_of(v0, 0u, args->horizon, complete);
    s->lay = r;
    s->horizon = args->horizon;
    s->complete = complete ? 1 : 0;
    s->n_states = (uint32_t)result->n_states;
    s->built = true;
    return LLE_OK;
}

int lle_policy_stats(const lle_policy* s, int64_t* frontier, int64_t* expanded, int cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    for (int d = 0; frontier && d < std::min(cap, (int)s->frontier.size()); d++) frontier[d] = s->frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)s->expanded.size()); d++) expanded[d] = s->expanded[(size_t)d];
    return (int)s->frontier.size();
}

int lle_policy_lookup(lle_policy* s, const lle_batch* batch, int32_t* steps_out, uint8_t* actions_out, int64_t action_stride, void* stream) {
    if (!s || !batch) return fail(LLE_ERR_NULL, "NULL handle or batch");
    if (!steps_out && !actions_out) return fail(LLE_ERR_NULL, "NULL steps_out and actions_out: nothing to write");
    if (!s->built) return fail(LLE_ERR_ARG, "the handle holds no table: lle_policy_build has not run, or it failed (LLE_POLICY_CAPACITY: no table at all)");
    if (actions_out && action_stride < s->lay.A) return fail(LLE_ERR_ARG, "action_stride is smaller than the number of agents");
    lle_buffer_desc pos{}, beams{};
    if (lle_batch_get_buffer(batch, LLE_BUF_POS, &pos) || lle_batch_get_buffer(batch, LLE_BUF_BEAMS, &beams)) return fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
    BatchEntry* entry = nullptr;
    for (auto& b : s->batches)
        if (b.batch == batch) entry = &b;
    if (entry && !(same_desc(entry->pos, pos) && same_desc(entry->beams, beams))) {  // the address now serves another batch
        s->batches.erase(s->batches.begin() + (entry - s->batches.data()));
        entry = nullptr;
    }
    if (!entry) {
        lle_buffer_desc bits{}, gems{};
        if (lle_batch_get_buffer(batch, LLE_BUF_BITS, &bits) || lle_batch_get_buffer(batch, LLE_BUF_GEMS, &gems)) return fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
        if (lle_batch_n_maps(batch) != 1) return fail(LLE_ERR_UNSUPPORTED, "a batch of several maps: the table is one map's");
        const int64_t n = lle_batch_n_envs(batch);
        if (pos.ndim != 3 || pos.shape[1] != s->lay.A) return fail(LLE_ERR_ARG, "the batch has " + std::to_string(pos.shape[1]) + " agents, the table's map " + std::to_string(s->lay.A));
        if (beams.ndim != 2 || beams.shape[1] != s->lay.Lw)
            return fail(LLE_ERR_ARG, "the batch has " + std::to_string(beams.shape[1]) + " beam words, the table's map " + std::to_string(s->lay.Lw));
        if (n < 1 || pos.shape[0] != n || beams.shape[0] != n || bits.shape[0] != n || gems.shape[0] != n || pos.elem_bytes != 1 || bits.elem_bytes != 8 ||
            gems.elem_bytes != 4 || beams.elem_bytes != 4 || pos.stride[0] < 2 * s->lay.A || pos.stride[1] < 2 || beams.stride[0] < s->lay.Lw)
            return fail(LLE_ERR_UNSUPPORTED, "the batch's buffers do not have the layout include/lle_hip.h describes");
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, pos.ptr) != hipSuccess) {
            (void)hipGetLastError();
            return fail(LLE_ERR_ARG, "the batch's buffers are not device memory");
        }
        if (attr.device != s->device) return fail(LLE_ERR_ARG, "the batch lives on HIP device " + std::to_string(attr.device) + ", the table on " + std::to_string(s->device));
        BatchEntry b;
        b.batch = batch;
        b.pos = pos;
        b.beams = beams;
        b.n_envs = n;
        b.view = sl::KeyView{static_cast<const uint8_t*>(pos.ptr), static_cast<const uint64_t*>(bits.ptr), static_cast<const uint32_t*>(gems.ptr),
                                static_cast<const uint32_t*>(beams.ptr), pos.stride[0], pos.stride[1], beams.stride[0]};
        if (s->batches.size() >= 64) s->batches.erase(s->batches.begin());  // (a bound, not a policy: entries are a few words)
        s->batches.push_back(b);
        entry = &s->batches.back();
    }
    DeviceGuard g(s->device);
    LookupParams q{};
    q.env = entry->view;
    q.n_envs = entry->n_envs;
    q.pool = s->d_pool;
    q.depth = s->d_depth;
    q.value = s->d_value;
    q.table = s->d_table;
    q.lay = s->lay;
    q.max_states = s->p.max_states;
    q.table_mask = s->p.table_mask;
    q.n_states = s->n_states;
    q.horizon = s->horizon;
    q.complete = s->complete;
    q.steps_out = steps_out;
    q.actions_out = actions_out;
    q.action_stride = action_stride;
    const dim3 grid((unsigned)((q.n_envs + lle::POLICY_THREADS - 1) / lle::POLICY_THREADS));
    hipLaunchKernelGGL(lle::policy_lookup, grid, dim3(lle::POLICY_THREADS), 0, reinterpret_cast<hipStream_t>(stream), q);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "policy_lookup launch failed");
    g_launched.fetch_or(K_LOOKUP);
    return LLE_OK;
}

size_t lle_policy_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, N_KERNELS, g_launched.load(), buf, cap); }
size_t lle_policy_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, N_KERNELS, (1u << N_KERNELS) - 1u, buf, cap); }

}  // extern "C"
