// forest.hip -- liblle_forest.so: the exact shortest joint plans of many equally shaped maps at once, one breadth-first tree per map,
// every tree walked depth by depth in the same launches (C ABI: include/lle_forest.h; DESIGN.md "Forest search").
//
// The library touches its batch only through include/lle_hip.h, like search.hip: ONE lle_batch of n_maps * E environments made with
// lle_batch_create_multi, in which map m owns the environments [m * E, (m + 1) * E).  Per map a segment of everything search.hip
// keeps: `cap` pool records (structure of arrays inside the segment), parent (u32, local index) and action (u16) per state, a table
// segment of a power of two >= max(2 cap, cap + E + 1) slots, eight u64 counters and the foreign-beam table (H * W bytes).  Record
// layout, hash, probe step, record predicates and the record I/O (scatter_item, occupant_is, copy_record) are those of
// ../search/search_logic.hpp, the host-side helpers of a C ABI call those of ../search/search_device.hpp; a tag is TAG_BIT | the
// candidate's index inside its map's block, so a table segment only ever names records of its own map and every map's search is
// exactly the single one.  What is this file's own: which lane serves which map, the descriptors, the per-map counters and fates.
//
// A level: the host reads all counters in one copy, decides each map's fate (forest_logic.hpp: advance), writes one descriptor per map
// in one copy and launches max over the active maps of ceil(items_m / E) pieces.  A piece is four launches over all n_maps * E lanes:
//   forest_expand    lane k serves map k / E and item piece * E + k % E of it (forest_logic.hpp: lane_work); an idle lane writes
//                    valid = 0 and nothing else; the others scatter their state and joint action as search_expand does
//   lle_batch_step   the unchanged step kernel, every environment of the batch
//   forest_insert    as search_insert, on the map's table segment; the foreign-beam table is read from memory (a workgroup spans several
//                    maps when E is no multiple of 256, and a table is H * W bytes that every lane of the map reads: it stays in cache)
//   forest_commit    as search_commit, on the map's pool segment and counters
// forest_roots reads every map's reset state once at creation, forest_seed puts it into state 0 of every searching map, forest_plans
// walks the parent links of every solved map, one lane per map.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_forest.h"
#include "../search/search_device.hpp"
#include "forest_logic.hpp"

namespace lle {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace fl = lle_forest_logic;

constexpr int FOREST_THREADS = 256;

struct ForestParams {
    sl::BatchView b;       // the batch (include/lle_hip.h buffer descriptors, read once)
    // the handle: one segment per map of each
    uint32_t* pool;        // [n_maps][n_words][cap]
    uint32_t* parent;      // [n_maps][cap]
    uint16_t* action;      // [n_maps][cap]
    uint32_t* table;       // [n_maps][slots]
    unsigned long long* counters;  // [n_maps][N_COUNTERS]
    const uint8_t* foreign;        // [n_maps][H * W]
    uint32_t* roots;       // [n_maps][n_words]: the record of every map's reset state
    const fl::MapDescriptor* desc;  // [n_maps]
    uint8_t* valid;        // [n_lanes]
    uint32_t* win_slot;    // [n_lanes]: the slot (inside the map's segment) candidate k claimed, SLOT_EMPTY when it is no winner
    uint8_t* plans;        // [n_maps][plan_rows][A], then [n_maps] flags: the parent links led back to state 0
    sl::RecordLayout lay;
    uint64_t cap, slots;
    int64_t n_maps, E, n_lanes;
    int32_t H, W, G;
    uint32_t collect_gems, n_joint;
    int32_t plan_rows;
    // the piece
    uint64_t piece;
};

// The pool segment of map `map`: word w of local state s at [w * cap + s] (forest_logic.hpp: pool_index).
__device__ inline uint32_t* pool_segment(const ForestParams& p, int64_t map) { return p.pool + (uint64_t)map * (uint64_t)p.lay.n_words * p.cap; }

__device__ inline int64_t lane_index() { return (int64_t)blockIdx.x * FOREST_THREADS + threadIdx.x; }

// One lane per map: the record of the map's first environment (freshly reset) into roots.
__global__ __launch_bounds__(FOREST_THREADS) void forest_roots(ForestParams p) {
    const int64_t m = lane_index();
    if (m >= p.n_maps) return;
    const sl::EnvRecord rec{p.b, p.lay, fl::env_index(m, p.E, 0)};
    for (int w = 0; w < p.lay.n_words; w++) p.roots[m * p.lay.n_words + w] = rec(w);
}

// One lane per map: state 0 of a searching map is its reset state (the table segment is all SLOT_EMPTY, the counters come from the host).
__global__ __launch_bounds__(FOREST_THREADS) void forest_seed(ForestParams p) {
    const int64_t m = lane_index();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const sl::RecordLayout& r = p.lay;
    const uint32_t* root = p.roots + m * r.n_words;
    for (int w = 0; w < r.n_words; w++) p.pool[fl::pool_index(m, r.n_words, w, p.cap, 0)] = root[w];
    const uint64_t h = sl::hash_record([&](int w) { return root[w]; }, r.n_key);
    p.table[fl::table_base(m, p.slots) + ((uint32_t)h & (uint32_t)(p.slots - 1))] = 0u;
    p.parent[fl::state_index(m, p.cap, 0)] = 0xFFFFFFFFu;
    p.action[fl::state_index(m, p.cap, 0)] = 0;
}

__global__ __launch_bounds__(FOREST_THREADS) void forest_expand(ForestParams p) {
    const int64_t k = lane_index();
    if (k >= p.n_lanes) return;
    const fl::LaneWork lw = fl::lane_work(k, p.piece, p.E, p.desc);
    if (lw.idle) {
        p.valid[k] = 0;
        return;
    }
    const uint32_t s = p.desc[lw.map].first_state + (uint32_t)(lw.item / p.n_joint);  // < the frontier's end <= cap
    // (an invalid item leaves environment k as it is: whatever the step makes of it, forest_insert drops the item)
    const bool valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{pool_segment(p, lw.map), p.cap, s}, k, (uint32_t)(lw.item % p.n_joint));
    p.valid[k] = valid ? 1 : 0;
    if (!valid) return;
    atomicAdd(&p.counters[fl::counter_index(lw.map, fl::CNT_EXPANDED)], 1ull);
}

// NO_COOP: mode no-cooperation.
template <bool NO_COOP>
__global__ __launch_bounds__(FOREST_THREADS) void forest_insert(ForestParams p) {
    const int64_t k = lane_index();
    if (k >= p.n_lanes || !p.valid[k]) return;  // (an idle lane has valid = 0)
    p.win_slot[k] = sl::SLOT_EMPTY;
    const int64_t map = k / p.E;
    const uint32_t local = (uint32_t)(k % p.E);
    unsigned long long* counters = p.counters + fl::counter_index(map, 0);
    if (counters[fl::CNT_OVERFLOW] != 0ull) return;  // (set by an earlier launch: this map's search has failed already)
    if (p.b.err[k] != 0) {  // the step refused a joint action the mask allowed
        atomicAdd(&counters[fl::CNT_STEP_ERRORS], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    if (sl::anybody_dead(me(r.w_bits), r.A)) return;
    if constexpr (NO_COOP) {
        const uint8_t* foreign = p.foreign + fl::foreign_base(map, p.H, p.W);
        for (int a = 0; a < r.A; a++) {
            const uint8_t* q = p.b.pos + k * p.b.pos_stride + a * p.b.pos_agent_stride;
            const int i = q[0], j = q[1];
            if (i < p.H && j < p.W && sl::on_foreign_beam(foreign[i * p.W + j], a)) return;
        }
    }
    const uint64_t h = sl::hash_record(me, r.n_key);
    const sl::Occupants who{p.b.key(), fl::env_index(map, p.E, 0), (uint32_t)p.E, pool_segment(p, map), p.cap, p.cap};
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, me); };
    const int64_t slot = sl::table_insert(p.table + fl::table_base(map, p.slots), (uint32_t)(p.slots - 1), h, sl::TAG_BIT | local, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) p.win_slot[k] = (uint32_t)slot;
    else if (slot == sl::INSERT_FULL) atomicMax(&counters[fl::CNT_OVERFLOW], 1ull);
}

__global__ __launch_bounds__(FOREST_THREADS) void forest_commit(ForestParams p) {
    const int64_t k = lane_index();
    if (k >= p.n_lanes || !p.valid[k]) return;
    const uint32_t slot = p.win_slot[k];
    if (slot == sl::SLOT_EMPTY) return;
    const int64_t map = k / p.E;
    unsigned long long* counters = p.counters + fl::counter_index(map, 0);
    const unsigned long long idx = atomicAdd(&counters[fl::CNT_STATES], 1ull);
    if (idx >= (unsigned long long)p.cap) {  // this map's pool is full: no answer (the tag stays; later launches return at once)
        atomicMax(&counters[fl::CNT_OVERFLOW], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    sl::copy_record(p.b, r, k, pool_segment(p, map), p.cap, idx);
    const uint64_t item = p.piece * (uint64_t)p.E + (uint64_t)(k % p.E);
    p.parent[fl::state_index(map, p.cap, idx)] = p.desc[map].first_state + (uint32_t)(item / p.n_joint);
    p.action[fl::state_index(map, p.cap, idx)] = (uint16_t)(item % p.n_joint);
    p.table[fl::table_base(map, p.slots) + slot] = (uint32_t)idx;
    if (sl::is_goal(me(r.w_bits), me(r.w_gems), r, p.collect_gems != 0u, p.G)) atomicMin(&counters[fl::CNT_GOAL], idx);
}

// One lane per map; desc[m]: active = solved, first_state = the goal state, items = the plan's length (<= plan_rows).
__global__ __launch_bounds__(FOREST_THREADS) void forest_plans(ForestParams p) {
    const int64_t m = lane_index();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const int A = p.lay.A;
    uint8_t* rows = p.plans + (uint64_t)m * (uint64_t)p.plan_rows * (uint64_t)A;
    uint8_t* flags = p.plans + (uint64_t)p.n_maps * (uint64_t)p.plan_rows * (uint64_t)A;
    uint64_t at = p.desc[m].first_state;
    const int64_t length = p.desc[m].items < (uint64_t)p.plan_rows ? (int64_t)p.desc[m].items : (int64_t)p.plan_rows;
    bool ok = true;
    for (int64_t t = length - 1; t >= 0; t--) {
        if (at >= p.cap) {
            ok = false;
            break;
        }
        uint32_t code = p.action[fl::state_index(m, p.cap, at)];
        for (int a = 0; a < A; a++) {
            rows[t * A + a] = (uint8_t)(code % 5u);
            code /= 5u;
        }
        at = p.parent[fl::state_index(m, p.cap, at)];
    }
    flags[m] = ok && at == 0u ? 1 : 0;
}

template __global__ void forest_insert<false>(ForestParams);
template __global__ void forest_insert<true>(ForestParams);

}  // namespace lle

// ================================================================================================ host side
using lle::ForestParams;
namespace sl = lle_search_logic;
namespace fl = lle_forest_logic;
namespace sd = lle_search_device;
using sd::DeviceGuard;
using sd::fail;
using sd::g_error;

namespace {

std::atomic<uint32_t> g_launched{0};
enum { K_ROOTS = 0, K_SEED, K_EXPAND, K_INSERT, K_INSERT_NO_COOP, K_COMMIT, K_PLANS, K_COUNT };
const char* const KERNEL_NAMES[K_COUNT] = {"forest_roots", "forest_seed", "forest_expand", "forest_insert<false>", "forest_insert<true>", "forest_commit",
                                           "forest_plans"};

static_assert(LLE_SEARCH_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_search.h and search_logic.hpp disagree");

struct MapRun {  // one map in the last run
    fl::MapProgress progress{};
    std::vector<int64_t> frontier, expanded;
    std::vector<uint8_t> plan;
};

}  // namespace

struct lle_forest {
    int device = 0;
    hipStream_t stream = nullptr;
    lle_batch* batch = nullptr;
    lle_map_info info{};            // of map 0: the maps agree on everything the search reads from it
    int64_t n_maps = 0, E = 0, cap = 0;
    std::vector<uint8_t> foreign;   // [n_maps][H * W]
    std::vector<uint32_t> roots;    // [n_maps][n_words]
    uint32_t* d_pool = nullptr;
    uint32_t* d_parent = nullptr;
    uint16_t* d_action = nullptr;
    uint32_t* d_table = nullptr;
    uint8_t* d_valid = nullptr;
    uint32_t* d_win = nullptr;
    unsigned long long* d_counters = nullptr;
    uint8_t* d_foreign = nullptr;
    uint32_t* d_roots = nullptr;
    fl::MapDescriptor* d_desc = nullptr;
    uint8_t* d_plans = nullptr;
    size_t plans_bytes = 0;
    // pinned: what the host reads and writes once per level
    fl::MapDescriptor* h_desc = nullptr;
    uint64_t* h_counters = nullptr;
    ForestParams p{};
    // the last run
    std::vector<MapRun> maps;
    int64_t valid_items = 0, launched_lanes = 0;
};

namespace {

dim3 grid_for(int64_t lanes) { return dim3((unsigned)((lanes + lle::FOREST_THREADS - 1) / lle::FOREST_THREADS)); }

int launch_piece(lle_forest* f, const ForestParams& p, int mode) {
    const dim3 grid = grid_for(p.n_lanes), block(lle::FOREST_THREADS);
    hipLaunchKernelGGL(lle::forest_expand, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "forest_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(f->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, f->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    if (mode == LLE_SEARCH_NO_COOPERATION) {
        hipLaunchKernelGGL((lle::forest_insert<true>), grid, block, 0, f->stream, p);
    } else {
        hipLaunchKernelGGL((lle::forest_insert<false>), grid, block, 0, f->stream, p);
    }
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "forest_insert launch failed");
    hipLaunchKernelGGL(lle::forest_commit, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "forest_commit launch failed");
    g_launched.fetch_or(1u << K_EXPAND | 1u << (mode == LLE_SEARCH_NO_COOPERATION ? K_INSERT_NO_COOP : K_INSERT) | 1u << K_COMMIT);
    return LLE_OK;
}

// h_desc to the device (the pinned buffer is not written again before the stream has been synchronised).
bool upload_descriptors(lle_forest* f) {
    return hipMemcpyAsync(f->d_desc, f->h_desc, (size_t)f->n_maps * sizeof(fl::MapDescriptor), hipMemcpyHostToDevice, f->stream) == hipSuccess;
}

}  // namespace

extern "C" {

const char* lle_forest_last_error(void) { return g_error.c_str(); }

void lle_forest_free(lle_forest* f) {
    if (!f) return;
    DeviceGuard g(f->device);
    (void)hipStreamSynchronize(f->stream);
    if (f->batch) lle_batch_free(f->batch);
    (void)hipFree(f->d_pool);
    (void)hipFree(f->d_parent);
    (void)hipFree(f->d_action);
    (void)hipFree(f->d_table);
    (void)hipFree(f->d_valid);
    (void)hipFree(f->d_win);
    (void)hipFree(f->d_counters);
    (void)hipFree(f->d_foreign);
    (void)hipFree(f->d_roots);
    (void)hipFree(f->d_desc);
    (void)hipFree(f->d_plans);
    if (f->h_desc) (void)hipHostFree(f->h_desc);
    if (f->h_counters) (void)hipHostFree(f->h_counters);
    delete f;
}

lle_forest* lle_forest_create(const lle_map* const* maps, int n_maps, const lle_forest_options* opt) {
    auto refuse = [](int code, const std::string& why) -> lle_forest* {
        fail(code, why);
        return nullptr;
    };
    if (!maps) return refuse(LLE_ERR_NULL, "NULL maps");
    if (n_maps < 1) return refuse(LLE_ERR_ARG, "n_maps must be at least 1");
    for (int m = 0; m < n_maps; m++)
        if (!maps[m]) return refuse(LLE_ERR_NULL, "NULL map (entry " + std::to_string(m) + ")");
    if (opt && opt->struct_bytes != sizeof(lle_forest_options)) return refuse(LLE_ERR_ARG, "lle_forest_options.struct_bytes is not sizeof(lle_forest_options)");
    const int64_t E = opt && opt->envs_per_map ? opt->envs_per_map : 256;
    const int64_t cap = opt && opt->max_states_per_map ? opt->max_states_per_map : 65536;
    if (E < 1 || E > fl::MAX_ENVS_PER_MAP) return refuse(LLE_ERR_ARG, "envs_per_map must be 1 .. 2^30");
    if (cap < 1 || cap > fl::MAX_STATES_PER_MAP) return refuse(LLE_ERR_ARG, "max_states_per_map must be 1 .. 2^30");
    if ((int64_t)n_maps * E > fl::MAX_LANES) return refuse(LLE_ERR_ARG, "n_maps * envs_per_map must be at most 2^30");
    if (fl::table_slots((uint64_t)cap, (uint64_t)E) > fl::MAX_TABLE_SLOTS)
        return refuse(LLE_ERR_ARG, "max_states_per_map + envs_per_map must be below 2^31 (a table segment has at most 2^31 slots)");
    lle_map_info info{};
    if (lle_map_get_info(maps[0], &info) != LLE_OK) return refuse(LLE_ERR_ARG, "lle_map_get_info failed");
    if (!sd::record_limits_ok(
            info, "more than 6 agents: a state has 5^A joint actions, the search serves maps of at most 6 agents (these maps have "))
        return nullptr;
    // the shapes, judged by the step library itself without a device: its refusal is the one lle_batch_create_multi would give
    if (lle_batch_arena_bytes_multi(maps, n_maps, E) < 0) return refuse(LLE_ERR_ARG, std::string("lle_batch_create_multi: ") + lle_last_error());
    const int H = info.height, W = info.width;
    std::vector<uint8_t> foreign;
    for (int m = 0; m < n_maps; m++)
        if (!sd::build_foreign(maps[m], H, W, foreign)) return refuse(LLE_ERR_ARG, "laser tile out of range (map " + std::to_string(m) + ")");
    int device = -1;
    if (sd::choose_device(opt ? opt->device : -1, "no HIP device: the search runs on the GPU only (there is no CPU fallback)", &device) != LLE_OK)
        return nullptr;

    auto* f = new lle_forest();
    f->device = device;
    f->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    f->info = info;
    f->n_maps = n_maps;
    f->E = E;
    f->cap = cap;
    f->foreign = std::move(foreign);
    f->maps.assign((size_t)n_maps, MapRun{});
    for (auto& mr : f->maps) mr.progress = fl::fresh_progress(false);
    DeviceGuard g(device);
    auto give_up = [&](int code, const std::string& why) -> lle_forest* {
        lle_forest_free(f);
        fail(code, why);
        return nullptr;
    };
    f->batch = lle_batch_create_multi(maps, n_maps, E, device, nullptr, 0, f->stream);
    if (!f->batch) return give_up(LLE_ERR_HIP, std::string("lle_batch_create_multi: ") + lle_last_error());
    if (sd::bind_batch(f->batch, info, (int64_t)n_maps * E, &f->p.b) != LLE_OK) {
        lle_forest_free(f);
        return nullptr;
    }
    const sl::RecordLayout lay = sl::make_layout(info.n_agents, info.n_beam_words, false);
    const uint64_t slots = fl::table_slots((uint64_t)cap, (uint64_t)E);
    const size_t HW = (size_t)H * W, M = (size_t)n_maps, lanes = M * (size_t)E;
    const size_t pool_bytes = M * (size_t)lay.n_words * (size_t)cap * 4;
    if (hipMalloc(&f->d_pool, pool_bytes) != hipSuccess || hipMalloc(&f->d_parent, M * (size_t)cap * 4) != hipSuccess ||
        hipMalloc(&f->d_action, M * (size_t)cap * 2) != hipSuccess || hipMalloc(&f->d_table, M * (size_t)slots * 4) != hipSuccess ||
        hipMalloc(&f->d_valid, lanes) != hipSuccess || hipMalloc(&f->d_win, lanes * 4) != hipSuccess ||
        hipMalloc(&f->d_counters, M * fl::N_COUNTERS * 8) != hipSuccess || hipMalloc(&f->d_foreign, std::max<size_t>(16, M * HW)) != hipSuccess ||
        hipMalloc(&f->d_roots, M * (size_t)lay.n_words * 4) != hipSuccess || hipMalloc(&f->d_desc, M * sizeof(fl::MapDescriptor)) != hipSuccess ||
        hipHostMalloc(&f->h_desc, M * sizeof(fl::MapDescriptor)) != hipSuccess || hipHostMalloc(&f->h_counters, M * fl::N_COUNTERS * 8) != hipSuccess ||
        hipMemcpyAsync(f->d_foreign, f->foreign.data(), M * HW, hipMemcpyHostToDevice, f->stream) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(LLE_ERR_HIP, "allocating the state pools failed (" + std::to_string(pool_bytes) + " bytes for " + std::to_string(n_maps) + " maps of " +
                                        std::to_string(cap) + " states of " + std::to_string(lay.n_words) + " words)");
    }
    ForestParams& p = f->p;
    p.pool = f->d_pool;
    p.parent = f->d_parent;
    p.action = f->d_action;
    p.table = f->d_table;
    p.counters = f->d_counters;
    p.foreign = f->d_foreign;
    p.roots = f->d_roots;
    p.desc = f->d_desc;
    p.valid = f->d_valid;
    p.win_slot = f->d_win;
    p.plans = nullptr;
    p.lay = lay;
    p.cap = (uint64_t)cap;
    p.slots = slots;
    p.n_maps = n_maps;
    p.E = E;
    p.n_lanes = (int64_t)n_maps * E;
    p.H = H;
    p.W = W;
    p.G = info.n_gems;
    p.n_joint = sl::pow5(info.n_agents);
    // ---- every map's reset state (the batch is freshly reset: World::new calls reset)
    f->roots.assign(M * (size_t)lay.n_words, 0u);
    hipLaunchKernelGGL(lle::forest_roots, grid_for(n_maps), dim3(lle::FOREST_THREADS), 0, f->stream, p);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(f->roots.data(), f->d_roots, f->roots.size() * 4, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(LLE_ERR_HIP, "reading the reset states failed");
    }
    g_launched.fetch_or(1u << K_ROOTS);
    g_error.clear();
    return f;
}

int lle_forest_run(lle_forest* f, const lle_search_args* args, lle_forest_result* per_map) {
    if (!f || !args || !per_map) return fail(LLE_ERR_NULL, "NULL handle, arguments or results");
    if (args->struct_bytes != sizeof(lle_search_args)) return fail(LLE_ERR_ARG, "lle_search_args.struct_bytes is not sizeof(lle_search_args)");
    if (args->mode != LLE_SEARCH_STANDARD && args->mode != LLE_SEARCH_NO_COOPERATION) return fail(LLE_ERR_ARG, "unknown mode");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    DeviceGuard g(f->device);
    const bool collect = args->collect_gems != 0;
    ForestParams p = f->p;
    p.lay = sl::make_layout(f->info.n_agents, f->info.n_beam_words, collect);
    p.collect_gems = collect ? 1u : 0u;
    const sl::RecordLayout& r = p.lay;
    const int A = r.A;
    const size_t M = (size_t)f->n_maps, HW = (size_t)p.H * p.W;
    f->valid_items = f->launched_lanes = 0;
    auto report = [&]() {
        for (size_t m = 0; m < M; m++) {
            const fl::MapProgress& pr = f->maps[m].progress;
            per_map[m].status = pr.status;
            per_map[m].length = pr.length;
            per_map[m].n_states = pr.n_states;
            per_map[m].depth_reached = pr.depth_reached;
            per_map[m].pad = 0;
        }
    };

    // ---- every reset state, judged on the host with the kernels' own functions
    bool any_active = false;
    for (size_t m = 0; m < M; m++) {
        MapRun& mr = f->maps[m];
        mr.frontier.assign(1, 1);
        mr.expanded.clear();
        mr.plan.clear();
        const uint32_t* root = f->roots.data() + m * (size_t)r.n_words;
        const bool root_ok = !sl::anybody_dead(root[r.w_bits], A) &&
                             !(args->mode == LLE_SEARCH_NO_COOPERATION && sl::root_on_foreign_beam(root, r, f->foreign.data() + m * HW, p.H, p.W));
        const bool solved = root_ok && sl::is_goal(root[r.w_bits], root[r.w_gems], r, collect, p.G);
        mr.progress = fl::fresh_progress(root_ok && !solved);  // (not ok: no plan starts here)
        if (solved) mr.progress.length = 0;
        any_active = any_active || mr.progress.active;
        uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
        std::fill(c, c + fl::N_COUNTERS, 0ull);
        c[fl::CNT_STATES] = 1;
        c[fl::CNT_GOAL] = fl::NO_GOAL;
        f->h_desc[m] = fl::level_descriptor(mr.progress, p.n_joint);
    }
    if (!any_active || args->t_max == 0) {
        report();
        return LLE_OK;
    }

    // ---- tables, counters and state 0 of every searching map
    hipError_t e = hipMemsetAsync(p.table, 0xFF, M * (size_t)p.slots * 4, f->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p.counters, f->h_counters, M * fl::N_COUNTERS * 8, hipMemcpyHostToDevice, f->stream);
    if (e == hipSuccess && !upload_descriptors(f)) e = hipErrorUnknown;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(lle::forest_seed, grid_for(f->n_maps), dim3(lle::FOREST_THREADS), 0, f->stream, p);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(f->stream);
        return fail(LLE_ERR_HIP, "preparing the pools failed");
    }
    g_launched.fetch_or(1u << K_SEED);

    // ---- level by level, all maps in lock-step (the first level's descriptors are on their way already)
    int depth = 0;
    while (depth < args->t_max && any_active) {
        if (depth > 0) {
            for (size_t m = 0; m < M; m++) f->h_desc[m] = fl::level_descriptor(f->maps[m].progress, p.n_joint);
            if (!upload_descriptors(f)) {
                (void)hipGetLastError();
                (void)hipStreamSynchronize(f->stream);
                return fail(LLE_ERR_HIP, "writing the level's descriptors failed");
            }
        }
        const uint64_t pieces = fl::piece_count(f->h_desc, f->n_maps, f->E);
        f->valid_items += (int64_t)fl::level_items(f->h_desc, f->n_maps);
        f->launched_lanes += (int64_t)pieces * p.n_lanes;
        for (uint64_t q = 0; q < pieces; q++) {
            p.piece = q;
            const int rc = launch_piece(f, p, args->mode);
            if (rc != LLE_OK) {
                (void)hipStreamSynchronize(f->stream);
                return rc;
            }
        }
        if (hipMemcpyAsync(f->h_counters, p.counters, M * fl::N_COUNTERS * 8, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
            hipStreamSynchronize(f->stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(LLE_ERR_HIP, "reading the level's counters failed");
        }
        depth++;
        any_active = false;
        for (size_t m = 0; m < M; m++) {
            MapRun& mr = f->maps[m];
            if (!mr.progress.active) continue;
            const uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
            int64_t frontier_new = 0, expanded_new = 0;
            const int fate = fl::advance(mr.progress, c, p.cap, depth, LLE_SEARCH_CAPACITY, &frontier_new, &expanded_new);
            if (fate == fl::FATE_STEP_ERROR) {
                report();
                return fail(LLE_ERR_HIP, "the step refused " + std::to_string(c[fl::CNT_STEP_ERRORS]) + " joint actions their availability masks allow (map " +
                                             std::to_string(m) + ")");
            }
            if (fate == fl::FATE_CAPACITY) {  // this map alone has no answer
                mr.frontier.assign(1, 1);
                mr.expanded.clear();
                continue;
            }
            mr.frontier.push_back(frontier_new);
            mr.expanded.push_back(expanded_new);
            any_active = any_active || mr.progress.active;
        }
    }

    // ---- the plans of the solved maps: one launch walks the parent links, one copy brings them back
    int rows = 0;
    for (size_t m = 0; m < M; m++) {
        const fl::MapProgress& pr = f->maps[m].progress;
        const bool solved = pr.length > 0;
        f->h_desc[m].active = solved ? 1u : 0u;
        f->h_desc[m].first_state = solved ? (uint32_t)pr.goal : 0u;
        f->h_desc[m].items = solved ? (uint64_t)pr.length : 0u;
        if (solved) rows = std::max(rows, pr.length);
    }
    if (rows > 0) {
        const size_t bytes = M * (size_t)rows * (size_t)A + M;
        if (bytes > f->plans_bytes) {
            (void)hipFree(f->d_plans);
            f->d_plans = nullptr;
            f->plans_bytes = 0;
            if (hipMalloc(&f->d_plans, bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(LLE_ERR_HIP, "allocating the plan buffer failed");
            }
            f->plans_bytes = bytes;
        }
        p.plans = f->d_plans;
        p.plan_rows = rows;
        std::vector<uint8_t> host(bytes, 0);
        bool ok = upload_descriptors(f);
        if (ok) {
            hipLaunchKernelGGL(lle::forest_plans, grid_for(f->n_maps), dim3(lle::FOREST_THREADS), 0, f->stream, p);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && hipMemcpyAsync(host.data(), f->d_plans, bytes, hipMemcpyDeviceToHost, f->stream) == hipSuccess;
        if (hipStreamSynchronize(f->stream) != hipSuccess || !ok) {
            (void)hipGetLastError();
            return fail(LLE_ERR_HIP, "reading the plans back failed");
        }
        g_launched.fetch_or(1u << K_PLANS);
        for (size_t m = 0; m < M; m++) {
            MapRun& mr = f->maps[m];
            if (mr.progress.length <= 0) continue;
            if (!host[M * (size_t)rows * (size_t)A + m]) {
                report();
                return fail(LLE_ERR_HIP, "the parent links of map " + std::to_string(m) + " do not lead back to the reset state");
            }
            const uint8_t* first = host.data() + m * (size_t)rows * (size_t)A;
            mr.plan.assign(first, first + (size_t)mr.progress.length * (size_t)A);
        }
    }
    report();
    return LLE_OK;
}

int lle_forest_plan(const lle_forest* f, int map_index, uint8_t* out, int64_t cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const MapRun& mr = f->maps[(size_t)map_index];
    if (mr.progress.length < 0) return fail(LLE_ERR_ARG, "the last run found no plan for this map");
    if (mr.progress.length > 0 && (!out || cap < (int64_t)mr.plan.size())) return fail(LLE_ERR_ARG, "the plan needs length * n_agents bytes");
    if (!mr.plan.empty()) std::memcpy(out, mr.plan.data(), mr.plan.size());
    return mr.progress.length;
}

int lle_forest_stats(const lle_forest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const MapRun& mr = f->maps[(size_t)map_index];
    for (int d = 0; frontier && d < std::min(cap, (int)mr.frontier.size()); d++) frontier[d] = mr.frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)mr.expanded.size()); d++) expanded[d] = mr.expanded[(size_t)d];
    return (int)mr.frontier.size();
}

int lle_forest_occupancy(const lle_forest* f, int64_t* valid_items, int64_t* launched_lanes) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (valid_items) *valid_items = f->valid_items;
    if (launched_lanes) *launched_lanes = f->launched_lanes;
    return LLE_OK;
}

size_t lle_forest_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, g_launched.load(), buf, cap); }
size_t lle_forest_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, (1u << K_COUNT) - 1u, buf, cap); }

}  // extern "C"
