// helpforest.hip -- liblle_helpforest.so: the solve modes over the help graph and no-sequence-N for many equally shaped maps at once, one
// breadth-first tree per map, every tree walked depth by depth in the same launches (C ABI: include/lle_helpforest.h; INTEGRATION.md
// section 19; DESIGN.md "Help forest").
//
// ../forest/forest.hip with the records of ../helpgraph/helpgraph.hip (help kind: two more words, the help value) or of
// ../trails/trails.hip (trail kind: one more word, the trail value).  ONE lle_batch of n_maps * E environments made with
// lle_batch_create_multi, in which map m owns the environments [m * E, (m + 1) * E); per map a segment of the pool (n_words + 2 arrays
// of `cap` words, whichever kind runs), parent, action, a table segment, eight counters -- and the map's OWN static data: its cell
// table (H * W words) and its edge rule.  Lanes, segments and the fates of a map are ../forest/forest_logic.hpp's, the edge rule and
// the modes ../helpgraph/helpgraph_logic.hpp's, the walk ../trails/trails_logic.hpp's.  Both kinds (hl::HelpKind, tl::TrailKind) run
// through the same code of ../search/search_logic.hpp: a LOCAL tag (TAG_BIT | index inside the map's block) is taken apart by sl::Piece,
// sl::occupant_is compares; helpforest_logic.hpp holds the fate of a map whose walk ran out of budget.
//
// A piece is four launches over all n_maps * E lanes:
//   hf_expand        lane k serves map k / E and item piece * E + k % E of it, or idles (valid = 0, nothing else written)
//   lle_batch_step   the unchanged step kernel, every environment of the batch
//   hf_insert<KIND>  as hg_insert / tr_insert on the map's table segment, with the map's own cell table and rule read from memory (a
//                    workgroup spans several maps when E is no multiple of 256; a table is H * W words that every lane of the map
//                    reads: it stays in cache).  The extra words of a candidate a tag names are worked out again by the comparing
//                    lane, from environment map * E + tag and that candidate's own parent in the map's segment: nothing is handed
//                    from lane to lane inside the launch, no lane waits, nothing needs a fence
//   hf_commit<KIND>  every winner takes an index of its map's segment, copies its record and its extra words (kept per lane by
//                    hf_insert: read in this later launch only), parent and action, and reports a goal the mode accepts
// hf_roots reads every map's reset state once at creation, hf_seed<KIND> puts it and its extra words into record 0 of every
// searching map, hf_plans walks the parent links of every solved map and fetches the goal's extra words, one lane per map.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lle_helpforest.h"
#include "../search/search_core.hpp"
#include "helpforest_logic.hpp"

namespace lle {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
namespace fl = lle_forest_logic;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;
namespace hfl = lle_helpforest_logic;

constexpr int HF_THREADS = 256;
template <int KIND>
using KindOf = std::conditional_t<KIND == hfl::KIND_HELP, hl::HelpKind, tl::TrailKind>;

struct HfParams {
    sl::BatchView b;       // the batch (include/lle_hip.h buffer descriptors, read once)
    // the handle: one segment per map of each
    uint32_t* pool;        // [n_maps][n_words + 2][cap]: the record, then the extra words
    uint32_t* parent;      // [n_maps][cap]
    uint16_t* action;      // [n_maps][cap]
    uint32_t* table;       // [n_maps][slots]
    unsigned long long* counters;  // [n_maps][N_COUNTERS]
    const uint32_t* cells;         // [n_maps][H * W]: the sources that own a laser tile on the cell (bit laser_id), per map
    const hl::EdgeRule* rules;     // [n_maps]
    uint32_t* roots;       // [n_maps][n_words]: the record of every map's reset state
    const uint32_t* root_extra;    // [n_maps][2]: the extra words of every map's reset state in this run
    const fl::MapDescriptor* desc; // [n_maps]
    uint8_t* valid;        // [n_lanes]
    uint32_t* win_slot;    // [n_lanes]: the slot (inside the map's segment) candidate k claimed, SLOT_EMPTY when it is no winner
    uint64_t* cand_extra;  // [n_lanes]: the extra words of winner k (help value, or the trail value in the low word), for hf_commit
    uint8_t* plans;        // [n_maps][plan_rows][A], then [n_maps] flags: the parent links led back to record 0
    uint32_t* goal_extra;  // [n_maps][2]: the extra words of every solved map's goal record
    sl::RecordLayout lay;
    uint64_t cap, slots;
    int64_t n_maps, E, n_lanes;
    int32_t H, W, G;
    int32_t mode, param;
    uint32_t collect_gems, n_joint;
    int32_t plan_rows;
    // the piece
    uint64_t piece;
};

__device__ inline uint32_t* pool_segment(const HfParams& p, int64_t map) { return p.pool + hfl::pool_segment_offset(map, p.lay.n_words, p.cap); }
__device__ inline sc::Cells map_cells(const HfParams& p, int64_t map) { return sc::Cells{p.cells + (uint64_t)map * (uint64_t)p.H * (uint64_t)p.W}; }
__device__ inline int64_t lane_index() { return (int64_t)blockIdx.x * HF_THREADS + threadIdx.x; }
// The kind a map searches with in this run: its own edge rule, the run's mode and param (k of a help mode, or N).
template <int KIND>
__device__ inline KindOf<KIND> map_kind(const HfParams& p, int64_t map) {
    if constexpr (KIND == hfl::KIND_HELP) return hl::HelpKind{p.rules[map], p.mode, p.param};
    else return tl::TrailKind{p.rules[map], p.param};
}
// A value as a lane keeps it between insert and commit, and as the host hands a reset state's over: a 64-bit word, the low one first.
template <class Kind>
__device__ inline typename Kind::Value value_of(uint32_t lo, uint32_t hi) {
    return (typename Kind::Value)((uint64_t)lo | (uint64_t)hi << 32);
}

// One lane per map: the record of the map's first environment (freshly reset) into roots.
__global__ __launch_bounds__(HF_THREADS) void hf_roots(HfParams p) {
    const int64_t m = lane_index();
    if (m >= p.n_maps) return;
    const sl::EnvRecord rec{p.b, p.lay, fl::env_index(m, p.E, 0)};
    for (int w = 0; w < p.lay.n_words; w++) p.roots[m * p.lay.n_words + w] = rec(w);
}

// One lane per map: record 0 of a searching map is its reset state with the extra words the host worked out, under the hash of its
// identity (the table segment is all SLOT_EMPTY, the counters come from the host).
template <int KIND>
__global__ __launch_bounds__(HF_THREADS) void hf_seed(HfParams p) {
    const int64_t m = lane_index();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const sl::RecordLayout& r = p.lay;
    const uint32_t* root = p.roots + m * r.n_words;
    uint32_t* seg = pool_segment(p, m);
    for (int w = 0; w < r.n_words; w++) seg[(uint64_t)w * p.cap] = root[w];
    const auto x = KindOf<KIND>::words(value_of<KindOf<KIND>>(p.root_extra[2 * m], p.root_extra[2 * m + 1]));
    sl::store_pool_extra(seg, p.cap, r, 0, x);
    const uint64_t h = sl::hash_record(sl::key_with_extra([&](int w) { return root[w]; }, r.n_key, x), r.n_key + KindOf<KIND>::EXTRA);
    p.table[fl::table_base(m, p.slots) + ((uint32_t)h & (uint32_t)(p.slots - 1))] = 0u;
    p.parent[fl::state_index(m, p.cap, 0)] = 0xFFFFFFFFu;
    p.action[fl::state_index(m, p.cap, 0)] = 0;
}

__global__ __launch_bounds__(HF_THREADS) void hf_expand(HfParams p) {
    const int64_t k = lane_index();
    if (k >= p.n_lanes) return;
    const fl::LaneWork lw = fl::lane_work(k, p.piece, p.E, p.desc);
    if (lw.idle) {
        p.valid[k] = 0;
        return;
    }
    const uint32_t s = p.desc[lw.map].first_state + (uint32_t)(lw.item / p.n_joint);  // < the frontier's end <= cap
    // (an invalid item leaves environment k as it is: whatever the step makes of it, hf_insert drops the item)
    const bool valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{pool_segment(p, lw.map), p.cap, s}, k, (uint32_t)(lw.item % p.n_joint));
    p.valid[k] = valid ? 1 : 0;
    if (!valid) return;
    atomicAdd(&p.counters[fl::counter_index(lw.map, fl::CNT_EXPANDED)], 1ull);
}

template <int KIND>
__global__ __launch_bounds__(HF_THREADS) void hf_insert(HfParams p) {
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
    const sl::EnvRecord rec{p.b, r, k};
    if (sl::anybody_dead(rec(r.w_bits), r.A)) return;
    const fl::MapDescriptor d = p.desc[map];
    const uint32_t* seg = pool_segment(p, map);
    const sl::Piece who{p.b, fl::env_index(map, p.E, 0), (uint32_t)p.E, seg, p.cap, p.cap, d.first_state, p.piece * (uint64_t)p.E, d.items, p.n_joint};
    const uint64_t parent = sl::tag_parent(who, local);  // < the frontier's end <= cap: the lane is not idle
    const auto kind = map_kind<KIND>(p, map);
    const uint64_t arcs = kind.state(rec, r, map_cells(p, map));
    typename KindOf<KIND>::Value extra;
    if (!kind.successor(seg, p.cap, r, parent, arcs, &extra)) {  // the walk did not finish: this map has no answer
        atomicAdd(&counters[hfl::CNT_DENSE], 1ull);
        return;
    }
    if (kind.violates(extra, r.A)) return;
    const auto me = sl::key_with_extra(rec, r.n_key, kind.words(extra));
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, kind, arcs, occupant, me); };
    const int64_t slot = sl::table_insert(p.table + fl::table_base(map, p.slots), (uint32_t)(p.slots - 1), sl::hash_record(me, r.n_key + KindOf<KIND>::EXTRA),
                                          sl::TAG_BIT | local, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) {
        p.win_slot[k] = (uint32_t)slot;
        p.cand_extra[k] = extra;  // for hf_commit, a later launch; no lane of this launch reads it
    } else if (slot == sl::INSERT_FULL) {
        atomicMax(&counters[fl::CNT_OVERFLOW], 1ull);
    }
}

template <int KIND>
__global__ __launch_bounds__(HF_THREADS) void hf_commit(HfParams p) {
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
    const sl::EnvRecord rec{p.b, r, k};
    uint32_t* seg = pool_segment(p, map);
    const auto kind = map_kind<KIND>(p, map);
    const auto extra = (typename KindOf<KIND>::Value)p.cand_extra[k];
    sl::copy_record(p.b, r, k, seg, p.cap, idx);
    sl::store_pool_extra(seg, p.cap, r, idx, kind.words(extra));
    const uint64_t item = p.piece * (uint64_t)p.E + (uint64_t)(k % p.E);
    p.parent[fl::state_index(map, p.cap, idx)] = p.desc[map].first_state + (uint32_t)(item / p.n_joint);
    p.action[fl::state_index(map, p.cap, idx)] = (uint16_t)(item % p.n_joint);
    p.table[fl::table_base(map, p.slots) + slot] = (uint32_t)idx;
    if (sl::is_goal(rec(r.w_bits), rec(r.w_gems), r, p.collect_gems != 0u, p.G) && kind.accepts(extra, r.A)) atomicMin(&counters[fl::CNT_GOAL], idx);
}

// One lane per map; desc[m]: active = solved, first_state = the goal record, items = the plan's length (<= plan_rows).
__global__ __launch_bounds__(HF_THREADS) void hf_plans(HfParams p) {
    const int64_t m = lane_index();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const int A = p.lay.A;
    uint8_t* rows = p.plans + (uint64_t)m * (uint64_t)p.plan_rows * (uint64_t)A;
    uint8_t* flags = p.plans + (uint64_t)p.n_maps * (uint64_t)p.plan_rows * (uint64_t)A;
    uint64_t at = p.desc[m].first_state;
    const uint32_t* seg = pool_segment(p, m);
    for (int w = 0; w < hfl::EXTRA_WORDS; w++) p.goal_extra[2 * m + w] = at < p.cap ? seg[(uint64_t)(p.lay.n_words + w) * p.cap + at] : 0u;
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

template __global__ void hf_seed<hfl::KIND_HELP>(HfParams);
template __global__ void hf_seed<hfl::KIND_TRAIL>(HfParams);
template __global__ void hf_insert<hfl::KIND_HELP>(HfParams);
template __global__ void hf_insert<hfl::KIND_TRAIL>(HfParams);
template __global__ void hf_commit<hfl::KIND_HELP>(HfParams);
template __global__ void hf_commit<hfl::KIND_TRAIL>(HfParams);

}  // namespace lle

// ================================================================================================ host side
using lle::HfParams;
namespace sl = lle_search_logic;
namespace fl = lle_forest_logic;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;
namespace hfl = lle_helpforest_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
using sd::DeviceGuard;
using sd::fail;
using sd::g_error;

namespace {

std::atomic<uint32_t> g_launched{0};
enum { K_ROOTS = 0, K_SEED_HELP, K_SEED_TRAIL, K_EXPAND, K_INSERT_HELP, K_INSERT_TRAIL, K_COMMIT_HELP, K_COMMIT_TRAIL, K_PLANS, K_COUNT };
const char* const KERNEL_NAMES[K_COUNT] = {"hf_roots",         "hf_seed<help>",   "hf_seed<trail>",   "hf_expand", "hf_insert<help>",
                                           "hf_insert<trail>", "hf_commit<help>", "hf_commit<trail>", "hf_plans"};

static_assert(LLE_HELPFOREST_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_helpforest.h and search_logic.hpp disagree");
static_assert(LLE_HELPFOREST_MAX_SOURCES == hl::MAX_SOURCES, "include/lle_helpforest.h and helpgraph_logic.hpp disagree");
static_assert(LLE_HELPGRAPH_STANDARD == hl::STANDARD && LLE_HELPGRAPH_NO_ASYMMETRIC == hl::NO_ASYMMETRIC && LLE_HELPGRAPH_NO_MUTUAL == hl::NO_MUTUAL &&
                  LLE_HELPGRAPH_NO_FULLY_COUPLED == hl::NO_FULLY_COUPLED && LLE_HELPGRAPH_NO_CONVERGENCE == hl::NO_CONVERGENCE &&
                  LLE_HELPGRAPH_NO_DIVERGENCE == hl::NO_DIVERGENCE,
              "include/lle_helpgraph.h and helpgraph_logic.hpp disagree");
static_assert(LLE_HELPFOREST_NO_SEQUENCE == hfl::NO_SEQUENCE && hfl::NO_SEQUENCE == hl::N_MODES, "include/lle_helpforest.h and helpforest_logic.hpp disagree");
static_assert(LLE_TRAILS_MIN_LENGTH == tl::MIN_LENGTH && LLE_TRAILS_MAX_LENGTH == tl::MAX_LENGTH && LLE_TRAILS_WALK_BUDGET == tl::WALK_BUDGET,
              "include/lle_trails.h and trails_logic.hpp disagree");
static_assert(LLE_HELPGRAPH_CAPACITY == LLE_TRAILS_CAPACITY, "one capacity status for both kinds");

struct MapRun {  // one map in the last run
    fl::MapProgress progress{};
    std::vector<int64_t> frontier, expanded;
    std::vector<uint8_t> plan;
    uint32_t extra[2] = {0u, 0u};  // of the plan's last state
};

}  // namespace

struct lle_helpforest {
    int device = 0;
    hipStream_t stream = nullptr;
    lle_batch* batch = nullptr;
    lle_map_info info{};            // of map 0: the maps agree on everything the search reads from it
    int64_t n_maps = 0, E = 0, cap = 0;
    std::vector<uint32_t> cells;    // [n_maps][H * W]
    std::vector<hl::EdgeRule> rules;  // [n_maps]
    std::vector<uint32_t> roots;    // [n_maps][n_words]
    uint32_t* d_pool = nullptr;
    uint32_t* d_parent = nullptr;
    uint16_t* d_action = nullptr;
    uint32_t* d_table = nullptr;
    uint8_t* d_valid = nullptr;
    uint32_t* d_win = nullptr;
    uint64_t* d_cand = nullptr;
    unsigned long long* d_counters = nullptr;
    uint32_t* d_cells = nullptr;
    hl::EdgeRule* d_rules = nullptr;
    uint32_t* d_roots = nullptr;
    uint32_t* d_root_extra = nullptr;
    uint32_t* d_goal_extra = nullptr;
    fl::MapDescriptor* d_desc = nullptr;
    uint8_t* d_plans = nullptr;
    size_t plans_bytes = 0;
    // pinned: what the host reads and writes once per level, and once per run
    fl::MapDescriptor* h_desc = nullptr;
    uint64_t* h_counters = nullptr;
    uint32_t* h_extra = nullptr;    // [n_maps][2]: up, the reset states' extra words; down, the goals'
    HfParams p{};
    // the last run
    std::vector<MapRun> maps;
    int64_t valid_items = 0, launched_lanes = 0;
};

namespace {

dim3 grid_for(int64_t lanes) { return dim3((unsigned)((lanes + lle::HF_THREADS - 1) / lle::HF_THREADS)); }

int launch_piece(lle_helpforest* f, const HfParams& p, int kind) {
    const dim3 grid = grid_for(p.n_lanes), block(lle::HF_THREADS);
    hipLaunchKernelGGL(lle::hf_expand, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "hf_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(f->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, f->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    if (kind == hfl::KIND_HELP) hipLaunchKernelGGL((lle::hf_insert<hfl::KIND_HELP>), grid, block, 0, f->stream, p);
    else hipLaunchKernelGGL((lle::hf_insert<hfl::KIND_TRAIL>), grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "hf_insert launch failed");
    if (kind == hfl::KIND_HELP) hipLaunchKernelGGL((lle::hf_commit<hfl::KIND_HELP>), grid, block, 0, f->stream, p);
    else hipLaunchKernelGGL((lle::hf_commit<hfl::KIND_TRAIL>), grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "hf_commit launch failed");
    g_launched.fetch_or(1u << K_EXPAND | 1u << (kind == hfl::KIND_HELP ? K_INSERT_HELP : K_INSERT_TRAIL) | 1u << (kind == hfl::KIND_HELP ? K_COMMIT_HELP : K_COMMIT_TRAIL));
    return LLE_OK;
}

// h_desc to the device (the pinned buffer is not written again before the stream has been synchronised).
bool upload_descriptors(lle_helpforest* f) {
    return hipMemcpyAsync(f->d_desc, f->h_desc, (size_t)f->n_maps * sizeof(fl::MapDescriptor), hipMemcpyHostToDevice, f->stream) == hipSuccess;
}

}  // namespace

extern "C" {

const char* lle_helpforest_last_error(void) { return g_error.c_str(); }

void lle_helpforest_free(lle_helpforest* f) {
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
    (void)hipFree(f->d_cand);
    (void)hipFree(f->d_counters);
    (void)hipFree(f->d_cells);
    (void)hipFree(f->d_rules);
    (void)hipFree(f->d_roots);
    (void)hipFree(f->d_root_extra);
    (void)hipFree(f->d_goal_extra);
    (void)hipFree(f->d_desc);
    (void)hipFree(f->d_plans);
    if (f->h_desc) (void)hipHostFree(f->h_desc);
    if (f->h_counters) (void)hipHostFree(f->h_counters);
    if (f->h_extra) (void)hipHostFree(f->h_extra);
    delete f;
}

lle_helpforest* lle_helpforest_create(const lle_map* const* maps, int n_maps, const lle_helpforest_options* opt) {
    auto refuse = [](int code, const std::string& why) -> lle_helpforest* {
        fail(code, why);
        return nullptr;
    };
    if (!maps) return refuse(LLE_ERR_NULL, "NULL maps");
    if (n_maps < 1) return refuse(LLE_ERR_ARG, "n_maps must be at least 1");
    for (int m = 0; m < n_maps; m++)
        if (!maps[m]) return refuse(LLE_ERR_NULL, "NULL map (entry " + std::to_string(m) + ")");
    if (opt && opt->struct_bytes != sizeof(lle_helpforest_options))
        return refuse(LLE_ERR_ARG, "lle_helpforest_options.struct_bytes is not sizeof(lle_helpforest_options)");
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
            info, "more than 6 agents: a state has 5^A joint actions, the help forest serves maps of at most 6 agents (these maps have "))
        return nullptr;
    // the shapes, judged by the step library itself without a device: its refusal is the one lle_batch_create_multi would give
    if (lle_batch_arena_bytes_multi(maps, n_maps, E) < 0) return refuse(LLE_ERR_ARG, std::string("lle_batch_create_multi: ") + lle_last_error());
    std::vector<uint32_t> cells;
    std::vector<hl::EdgeRule> rules((size_t)n_maps);
    for (int m = 0; m < n_maps; m++) {
        std::string why;
        if (!sc::build_rule(maps[m], info, cells, rules[(size_t)m], why)) return refuse(LLE_ERR_UNSUPPORTED, why + " (map " + std::to_string(m) + ")");
    }
    int device = -1;
    if (sd::choose_device(opt ? opt->device : -1, "no HIP device: the help forest runs on the GPU only (there is no CPU fallback)", &device) != LLE_OK)
        return nullptr;

    auto* f = new lle_helpforest();
    f->device = device;
    f->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    f->info = info;
    f->n_maps = n_maps;
    f->E = E;
    f->cap = cap;
    f->cells = std::move(cells);
    f->rules = std::move(rules);
    f->maps.assign((size_t)n_maps, MapRun{});
    for (auto& mr : f->maps) mr.progress = fl::fresh_progress(false);
    DeviceGuard g(device);
    auto give_up = [&](int code, const std::string& why) -> lle_helpforest* {
        lle_helpforest_free(f);
        fail(code, why);
        return nullptr;
    };
    f->batch = lle_batch_create_multi(maps, n_maps, E, device, nullptr, 0, f->stream);
    if (!f->batch) return give_up(LLE_ERR_HIP, std::string("lle_batch_create_multi: ") + lle_last_error());
    if (sd::bind_batch(f->batch, info, (int64_t)n_maps * E, &f->p.b) != LLE_OK) {
        lle_helpforest_free(f);
        return nullptr;
    }
    const sl::RecordLayout lay = sl::make_layout(info.n_agents, info.n_beam_words, false);
    const uint64_t slots = fl::table_slots((uint64_t)cap, (uint64_t)E);
    const size_t HW = (size_t)info.height * info.width, M = (size_t)n_maps, lanes = M * (size_t)E;
    const size_t pool_bytes = M * (size_t)(lay.n_words + hfl::EXTRA_WORDS) * (size_t)cap * 4;
    if (hipMalloc(&f->d_pool, pool_bytes) != hipSuccess || hipMalloc(&f->d_parent, M * (size_t)cap * 4) != hipSuccess ||
        hipMalloc(&f->d_action, M * (size_t)cap * 2) != hipSuccess || hipMalloc(&f->d_table, M * (size_t)slots * 4) != hipSuccess ||
        hipMalloc(&f->d_valid, lanes) != hipSuccess || hipMalloc(&f->d_win, lanes * 4) != hipSuccess || hipMalloc(&f->d_cand, lanes * 8) != hipSuccess ||
        hipMalloc(&f->d_counters, M * fl::N_COUNTERS * 8) != hipSuccess || hipMalloc(&f->d_cells, std::max<size_t>(16, M * HW * 4)) != hipSuccess ||
        hipMalloc(&f->d_rules, M * sizeof(hl::EdgeRule)) != hipSuccess || hipMalloc(&f->d_roots, M * (size_t)lay.n_words * 4) != hipSuccess ||
        hipMalloc(&f->d_root_extra, M * 8) != hipSuccess || hipMalloc(&f->d_goal_extra, M * 8) != hipSuccess ||
        hipMalloc(&f->d_desc, M * sizeof(fl::MapDescriptor)) != hipSuccess || hipHostMalloc(&f->h_desc, M * sizeof(fl::MapDescriptor)) != hipSuccess ||
        hipHostMalloc(&f->h_counters, M * fl::N_COUNTERS * 8) != hipSuccess || hipHostMalloc(&f->h_extra, M * 8) != hipSuccess ||
        (HW > 0 && hipMemcpyAsync(f->d_cells, f->cells.data(), M * HW * 4, hipMemcpyHostToDevice, f->stream) != hipSuccess) ||
        hipMemcpyAsync(f->d_rules, f->rules.data(), M * sizeof(hl::EdgeRule), hipMemcpyHostToDevice, f->stream) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(LLE_ERR_HIP, "allocating the record pools failed (" + std::to_string(pool_bytes) + " bytes for " + std::to_string(n_maps) + " maps of " +
                                        std::to_string(cap) + " records of " + std::to_string(lay.n_words + hfl::EXTRA_WORDS) + " words)");
    }
    HfParams& p = f->p;
    p.pool = f->d_pool;
    p.parent = f->d_parent;
    p.action = f->d_action;
    p.table = f->d_table;
    p.counters = f->d_counters;
    p.cells = f->d_cells;
    p.rules = f->d_rules;
    p.roots = f->d_roots;
    p.root_extra = f->d_root_extra;
    p.goal_extra = f->d_goal_extra;
    p.desc = f->d_desc;
    p.valid = f->d_valid;
    p.win_slot = f->d_win;
    p.cand_extra = f->d_cand;
    p.plans = nullptr;
    p.lay = lay;
    p.cap = (uint64_t)cap;
    p.slots = slots;
    p.n_maps = n_maps;
    p.E = E;
    p.n_lanes = (int64_t)n_maps * E;
    p.H = info.height;
    p.W = info.width;
    p.G = info.n_gems;
    p.n_joint = sl::pow5(info.n_agents);
    // ---- every map's reset state (the batch is freshly reset: World::new calls reset)
    f->roots.assign(M * (size_t)lay.n_words, 0u);
    hipLaunchKernelGGL(lle::hf_roots, grid_for(n_maps), dim3(lle::HF_THREADS), 0, f->stream, p);
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

int lle_helpforest_run(lle_helpforest* f, const lle_helpforest_args* args, const uint8_t* search, lle_helpforest_result* per_map) {
    if (!args || !per_map) return fail(LLE_ERR_NULL, "NULL arguments or results");
    // (the arguments are judged before the handle is looked at: what they refuse they refuse on a machine without a device too)
    if (args->struct_bytes != sizeof(lle_helpforest_args)) return fail(LLE_ERR_ARG, "lle_helpforest_args.struct_bytes is not sizeof(lle_helpforest_args)");
    if (args->mode < 0 || args->mode >= hfl::N_MODES) return fail(LLE_ERR_ARG, "unknown mode");
    if ((args->mode == LLE_HELPGRAPH_NO_CONVERGENCE || args->mode == LLE_HELPGRAPH_NO_DIVERGENCE) && args->param < 2)
        return fail(LLE_ERR_ARG, "param must be at least 2: a convergence or divergence has at least two helpers or beneficiaries");
    if (args->mode == LLE_HELPFOREST_NO_SEQUENCE && (args->param < tl::MIN_LENGTH || args->param > tl::MAX_LENGTH))
        return fail(LLE_ERR_ARG, "param must be 2 .. 16: a sequence has at least two edges, and a field of the trail value has 4 bits");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    DeviceGuard g(f->device);
    const bool collect = args->collect_gems != 0;
    const int kind = hfl::kind_of(args->mode);
    HfParams p = f->p;
    p.lay = sl::make_layout(f->info.n_agents, f->info.n_beam_words, collect);
    p.mode = args->mode;
    p.param = args->param;
    p.collect_gems = collect ? 1u : 0u;
    const sl::RecordLayout& r = p.lay;
    const int A = r.A;
    const size_t M = (size_t)f->n_maps, HW = (size_t)p.H * p.W;
    f->valid_items = f->launched_lanes = 0;
    auto report = [&]() {
        for (size_t m = 0; m < M; m++) {
            const MapRun& mr = f->maps[m];
            const bool plan = mr.progress.length >= 0;
            per_map[m].status = mr.progress.status;
            per_map[m].length = mr.progress.length;
            per_map[m].n_states = mr.progress.n_states;
            per_map[m].depth_reached = mr.progress.depth_reached;
            per_map[m].help_lo = plan && kind == hfl::KIND_HELP ? mr.extra[0] : 0u;
            per_map[m].help_hi = plan && kind == hfl::KIND_HELP ? mr.extra[1] : 0u;
            per_map[m].trail = plan && kind == hfl::KIND_TRAIL ? mr.extra[0] : 0u;
        }
    };

    // ---- every reset state (t = 0: its edges count), judged on the host with the kernels' own functions
    bool any_active = false;
    for (size_t m = 0; m < M; m++) {
        MapRun& mr = f->maps[m];
        mr.expanded.clear();
        mr.plan.clear();
        mr.extra[0] = mr.extra[1] = 0u;
        uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
        std::fill(c, c + fl::N_COUNTERS, 0ull);
        c[fl::CNT_STATES] = 1;
        c[fl::CNT_GOAL] = fl::NO_GOAL;
        f->h_extra[2 * m] = f->h_extra[2 * m + 1] = 0u;
        if (search && !search[m]) {  // not asked for: idle from the first level
            mr.frontier.clear();
            mr.progress = hfl::skipped_progress();
            f->h_desc[m] = fl::level_descriptor(mr.progress, p.n_joint);
            continue;
        }
        mr.frontier.assign(1, 1);
        const uint32_t* root = f->roots.data() + m * (size_t)r.n_words;
        const uint32_t* cells = f->cells.data() + m * HW;
        const uint64_t root_edges = hl::state_edges([&](int w) { return root[w]; }, r, f->rules[m], [&](int c_) { return cells[c_]; });
        bool root_ok = !sl::anybody_dead(root[r.w_bits], A), accepted = true, dense = false;
        if (kind == hfl::KIND_HELP) {
            root_ok = root_ok && !hl::violates(root_edges, p.mode, p.param, A);
            accepted = hl::accepts(root_edges, p.mode, A);
            f->h_extra[2 * m] = hl::help_lo(root_edges);
            f->h_extra[2 * m + 1] = hl::help_hi(root_edges);
        } else {
            int budget = tl::WALK_BUDGET;
            const uint32_t root_trail = tl::layer_update(0u, root_edges, p.param, A, budget);
            dense = budget < 0;
            root_ok = root_ok && !dense && !tl::violates_sequence(root_trail, p.param, A);  // a reset state that holds a trail of N: no plan
            f->h_extra[2 * m] = dense ? 0u : root_trail;
        }
        const bool solved = root_ok && accepted && sl::is_goal(root[r.w_bits], root[r.w_gems], r, collect, p.G);
        mr.progress = fl::fresh_progress(root_ok && !solved);  // (not ok: no plan starts here)
        if (dense) mr.progress.status = LLE_TRAILS_DENSE;
        if (solved) {
            mr.progress.length = 0;
            mr.extra[0] = f->h_extra[2 * m];
            mr.extra[1] = f->h_extra[2 * m + 1];
        }
        any_active = any_active || mr.progress.active;
        f->h_desc[m] = fl::level_descriptor(mr.progress, p.n_joint);
    }
    if (!any_active || args->t_max == 0) {
        report();
        return LLE_OK;
    }

    // ---- tables, counters and record 0 of every searching map
    hipError_t e = hipMemsetAsync(p.table, 0xFF, M * (size_t)p.slots * 4, f->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p.counters, f->h_counters, M * fl::N_COUNTERS * 8, hipMemcpyHostToDevice, f->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_root_extra, f->h_extra, M * 8, hipMemcpyHostToDevice, f->stream);
    if (e == hipSuccess && !upload_descriptors(f)) e = hipErrorUnknown;
    if (e == hipSuccess) {
        if (kind == hfl::KIND_HELP) hipLaunchKernelGGL((lle::hf_seed<hfl::KIND_HELP>), grid_for(f->n_maps), dim3(lle::HF_THREADS), 0, f->stream, p);
        else hipLaunchKernelGGL((lle::hf_seed<hfl::KIND_TRAIL>), grid_for(f->n_maps), dim3(lle::HF_THREADS), 0, f->stream, p);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(f->stream);
        return fail(LLE_ERR_HIP, "preparing the pools failed");
    }
    g_launched.fetch_or(1u << (kind == hfl::KIND_HELP ? K_SEED_HELP : K_SEED_TRAIL));

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
            const int rc = launch_piece(f, p, kind);
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
            const int fate = hfl::advance(mr.progress, c, p.cap, depth, LLE_HELPGRAPH_CAPACITY, LLE_TRAILS_DENSE, &frontier_new, &expanded_new);
            if (fate == fl::FATE_STEP_ERROR) {
                report();
                return fail(LLE_ERR_HIP, "the step refused " + std::to_string(c[fl::CNT_STEP_ERRORS]) + " joint actions their availability masks allow (map " +
                                             std::to_string(m) + ")");
            }
            if (fate == fl::FATE_CAPACITY || fate == hfl::FATE_DENSE) {  // this map alone has no answer
                mr.frontier.assign(1, 1);
                mr.expanded.clear();
                continue;
            }
            mr.frontier.push_back(frontier_new);
            mr.expanded.push_back(expanded_new);
            any_active = any_active || mr.progress.active;
        }
    }

    // ---- the plans of the solved maps: one launch walks the parent links and fetches the goals' extra words, two copies bring them back
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
            hipLaunchKernelGGL(lle::hf_plans, grid_for(f->n_maps), dim3(lle::HF_THREADS), 0, f->stream, p);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && hipMemcpyAsync(host.data(), f->d_plans, bytes, hipMemcpyDeviceToHost, f->stream) == hipSuccess &&
             hipMemcpyAsync(f->h_extra, f->d_goal_extra, M * 8, hipMemcpyDeviceToHost, f->stream) == hipSuccess;
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
            mr.extra[0] = f->h_extra[2 * m];
            mr.extra[1] = kind == hfl::KIND_HELP ? f->h_extra[2 * m + 1] : 0u;
        }
    }
    report();
    return LLE_OK;
}

int lle_helpforest_plan(const lle_helpforest* f, int map_index, uint8_t* out, int64_t cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const MapRun& mr = f->maps[(size_t)map_index];
    if (mr.progress.length < 0) return fail(LLE_ERR_ARG, "the last run found no plan for this map");
    if (mr.progress.length > 0 && (!out || cap < (int64_t)mr.plan.size())) return fail(LLE_ERR_ARG, "the plan needs length * n_agents bytes");
    if (!mr.plan.empty()) std::memcpy(out, mr.plan.data(), mr.plan.size());
    return mr.progress.length;
}

int lle_helpforest_stats(const lle_helpforest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const MapRun& mr = f->maps[(size_t)map_index];
    for (int d = 0; frontier && d < std::min(cap, (int)mr.frontier.size()); d++) frontier[d] = mr.frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)mr.expanded.size()); d++) expanded[d] = mr.expanded[(size_t)d];
    return (int)mr.frontier.size();
}

int lle_helpforest_occupancy(const lle_helpforest* f, int64_t* valid_items, int64_t* launched_lanes) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (valid_items) *valid_items = f->valid_items;
    if (launched_lanes) *launched_lanes = f->launched_lanes;
    return LLE_OK;
}

size_t lle_helpforest_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, g_launched.load(), buf, cap); }
size_t lle_helpforest_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, (1u << K_COUNT) - 1u, buf, cap); }

}  // extern "C"
