// trails.hip -- liblle_trails.so: the exact shortest joint plan of a map that holds no sequence of N help events (no-sequence-N), by
// breadth-first search over (world state, trail lengths) through the step kernel of liblle_hip.so (C ABI: include/lle_trails.h;
// INTEGRATION.md section 18; DESIGN.md "Trail search").
//
// The search of ../helpgraph/helpgraph.hip with ONE more word per record in place of two: the TRAIL VALUE of the trajectory that
// reached the state (4 bits per agent: the length of the longest trail of help edges that ends at the agent).  The trail word is part
// of a record's identity -- hashed and compared after the search's key words -- and lives only in the pool: the batch has no buffer
// for it.  A level is walked in pieces of at most `chunk` work items, four launches each:
//   tr_expand       as search_expand: lane k scatters the record of its state into environment k and writes its joint action
//   lle_batch_step  the unchanged step kernel
//   tr_insert       lane k drops refused and deadly successors, works out L' = layer_update(L(parent), state_edges(successor)) in
//                   registers, drops the item when some trail has N edges, hashes the record with L' and probes the table.  An occupied
//                   slot is compared word for word -- with the pool, or with the candidate a tag names: that candidate's key words lie
//                   complete in the batch since the step, and its trail word is worked out AGAIN by the comparing lane, from its own
//                   arcs (equal key words, equal arcs) and the other parent's pool record, both written by earlier launches.  Nothing
//                   is handed from lane to lane inside the launch, so no lane waits and nothing needs a fence.
//   tr_commit       every winner takes a pool index, copies its record and its trail word (kept for it, per candidate, by tr_insert:
//                   read in this later launch only), parent and action, and reports a goal
// The host reads the counters once per level.  Layout, hash, table, record I/O, batch binding and the reset state are those of
// ../search/search_logic.hpp and ../search/search_device.hpp; the edge rule is ../helpgraph/helpgraph_logic.hpp's state_edges;
// trails_logic.hpp holds the walk over one state's arcs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_trails.h"
#include "../search/search_device.hpp"
#include "../search/search_logic.hpp"
#include "trails_logic.hpp"

namespace lle {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;

constexpr int TR_THREADS = 256;
constexpr size_t LDS_TABLE_MAX_BYTES = 16384;  // H * W * 4 up to here: the cell table is staged in LDS, as hg_insert<true> does
enum { CNT_STATES = 0, CNT_EXPANDED, CNT_GOAL, CNT_OVERFLOW, CNT_STEP_ERRORS, CNT_DENSE, CNT_COUNT = 8 };
constexpr unsigned long long NO_GOAL = ~0ull;

struct TrParams {
    sl::BatchView b;       // the batch (include/lle_hip.h buffer descriptors, read once)
    // the handle
    uint32_t* pool;        // [n_words + 1][max_states]: the record, then the trail word
    uint32_t* parent;      // [max_states]
    uint16_t* action;      // [max_states]
    uint32_t* table;       // [table_mask + 1]
    uint8_t* valid;        // [chunk]
    uint32_t* win_slot;    // [chunk]: the slot candidate k claimed, SLOT_EMPTY when it is no winner
    uint32_t* cand_trail;  // [chunk]: the trail value of winner k, written by tr_insert for tr_commit
    unsigned long long* counters;  // [CNT_COUNT]
    const uint32_t* cells; // [H * W]: the sources that own a laser tile on the cell (bit laser_id)
    hl::EdgeRule rule;
    sl::RecordLayout lay;
    uint32_t max_states, table_mask;
    int32_t G;
    int32_t N;             // no trail of N edges
    uint32_t collect_gems;
    // the piece
    uint32_t first_state;  // pool index of the frontier's first record
    uint32_t n_joint;      // 5^A
    uint64_t item0;        // first work item of the piece, counted over the level
    uint32_t n_items;      // <= chunk
};

__global__ __launch_bounds__(TR_THREADS) void tr_expand(TrParams p) {
    const uint32_t k = blockIdx.x * TR_THREADS + threadIdx.x;
    bool valid = false;
    if (k < p.n_items) {
        const uint64_t item = p.item0 + k;
        const uint32_t s = p.first_state + (uint32_t)(item / p.n_joint);  // < the frontier's end <= max_states
        // (an invalid item leaves environment k as it is: whatever the step makes of it, tr_insert drops the item)
        valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{p.pool, p.max_states, s}, k, (uint32_t)(item % p.n_joint));
        p.valid[k] = valid ? 1 : 0;
    }
    if (valid) atomicAdd(&p.counters[CNT_EXPANDED], 1ull);
}

struct Cells {  // the cell table, in LDS or in global memory
    const uint32_t* cells;
    __host__ __device__ uint32_t operator()(int c) const { return cells[c]; }
};

template <class Cell>
__device__ __forceinline__ void insert_lane(const TrParams& p, const Cell& cell, uint32_t k) {
    p.win_slot[k] = sl::SLOT_EMPTY;
    if (p.counters[CNT_OVERFLOW] != 0ull) return;  // (set by an earlier launch: the search has failed already)
    if (!p.valid[k]) return;
    if (p.b.err[k] != 0) {  // the step refused a joint action the mask allowed
        atomicAdd(&p.counters[CNT_STEP_ERRORS], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord rec{p.b, r, k};
    if (sl::anybody_dead(rec(r.w_bits), r.A)) return;
    const uint64_t parent = p.first_state + (p.item0 + k) / p.n_joint;
    const uint64_t edges = hl::state_edges(rec, r, p.rule, cell);
    int budget = tl::WALK_BUDGET;
    const uint32_t trail = tl::successor_trail(p.pool, p.max_states, r, parent, edges, p.N, budget);
    if (budget < 0) {  // the walk did not finish: the run has no answer
        atomicAdd(&p.counters[CNT_DENSE], 1ull);
        return;
    }
    if (tl::violates_sequence(trail, p.N, r.A)) return;
    const auto me = tl::key_with_trail(rec, r.n_key, trail);
    const uint64_t h = sl::hash_record(me, r.n_key + 1);
    const tl::TrailOccupants who{p.b, p.n_items, p.pool, p.max_states, p.max_states, p.first_state, p.item0, p.n_joint, p.N};
    auto same_as = [&](uint32_t occupant) { return tl::trail_occupant_is(who, r, occupant, me, edges); };
    const int64_t slot = sl::table_insert(p.table, p.table_mask, h, sl::TAG_BIT | k, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) {
        p.win_slot[k] = (uint32_t)slot;
        p.cand_trail[k] = trail;  // for tr_commit, a later launch; no lane of this launch reads it
    } else if (slot == sl::INSERT_FULL) {
        atomicMax(&p.counters[CNT_OVERFLOW], 1ull);
    }
}

// LDS_TABLE: the cell table (H * W words <= LDS_TABLE_MAX_BYTES) staged in LDS; otherwise every read goes to global memory.
template <bool LDS_TABLE>
__global__ __launch_bounds__(TR_THREADS) void tr_insert(TrParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cells[];
    if constexpr (LDS_TABLE) {  // (every lane of the workgroup gets here: no exit before the barrier)
        const int HW = p.rule.H * p.rule.W;
        for (int c = threadIdx.x; c < HW; c += TR_THREADS) lds_cells[c] = p.cells[c];
        __syncthreads();
    }
    const uint32_t k = blockIdx.x * TR_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    if constexpr (LDS_TABLE) insert_lane(p, Cells{lds_cells}, k);
    else insert_lane(p, Cells{p.cells}, k);
}

__global__ __launch_bounds__(TR_THREADS) void tr_commit(TrParams p) {
    const uint32_t k = blockIdx.x * TR_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    const uint32_t slot = p.win_slot[k];
    if (slot == sl::SLOT_EMPTY) return;
    const unsigned long long idx = atomicAdd(&p.counters[CNT_STATES], 1ull);
    if (idx >= (unsigned long long)p.max_states) {  // the pool is full: no answer (the tag stays; later launches return at once)
        atomicMax(&p.counters[CNT_OVERFLOW], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord rec{p.b, r, k};
    sl::copy_record(p.b, r, k, p.pool, p.max_states, idx);
    tl::store_pool_trail(p.pool, p.max_states, r, idx, p.cand_trail[k]);
    const uint64_t item = p.item0 + k;
    p.parent[idx] = p.first_state + (uint32_t)(item / p.n_joint);
    p.action[idx] = (uint16_t)(item % p.n_joint);
    p.table[slot] = (uint32_t)idx;
    if (sl::is_goal(rec(r.w_bits), rec(r.w_gems), r, p.collect_gems != 0u, p.G)) atomicMin(&p.counters[CNT_GOAL], idx);
}

template __global__ void tr_insert<false>(TrParams);
template __global__ void tr_insert<true>(TrParams);

}  // namespace lle

// ================================================================================================ host side
using lle::TrParams;
namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;
using sd::DeviceGuard;
using sd::fail;
using sd::g_error;

namespace {

std::atomic<uint32_t> g_launched{0};
const char* const KERNEL_NAMES[4] = {"tr_expand", "tr_insert<false>", "tr_insert<true>", "tr_commit"};
static_assert(LLE_TRAILS_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_trails.h and search_logic.hpp disagree");
static_assert(LLE_TRAILS_MAX_SOURCES == hl::MAX_SOURCES, "include/lle_trails.h and helpgraph_logic.hpp disagree");
static_assert(LLE_TRAILS_MIN_LENGTH == tl::MIN_LENGTH && LLE_TRAILS_MAX_LENGTH == tl::MAX_LENGTH && LLE_TRAILS_WALK_BUDGET == tl::WALK_BUDGET,
              "include/lle_trails.h and trails_logic.hpp disagree");
static_assert(4 * LLE_TRAILS_MAX_AGENTS <= 31 && LLE_TRAILS_MAX_LENGTH - 1 <= 15, "a trail value is 4 bits per agent below the REACHED bit");

// Host copy of the static map data the edge rule needs (helpgraph_logic.hpp: EdgeRule), from lle_map_laser_tiles / lle_map_sources.
struct MapData {
    lle_map_info info{};
    std::vector<uint32_t> cells;  // [H * W]
    hl::EdgeRule rule{};
};

bool build_rule(const lle_map* map, MapData& md, std::string& err) {
    const int H = md.info.height, W = md.info.width;
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    if ((int)src.size() > hl::MAX_SOURCES) {
        err = "more than 32 sources: a cell's word has one bit per source";
        return false;
    }
    md.rule.A = md.info.n_agents;
    md.rule.H = H;
    md.rule.W = W;
    md.rule.enabled = 0u;
    for (int a = 0; a < sl::MAX_AGENTS; a++) md.rule.mine[a] = 0u;
    for (size_t l = 0; l < src.size(); l++) {
        if (src[l].enabled) md.rule.enabled |= 1u << l;
        if (src[l].agent_id >= 0 && src[l].agent_id < sl::MAX_AGENTS) md.rule.mine[src[l].agent_id] |= 1u << l;
    }
    md.cells.assign((size_t)H * W, 0u);
    std::vector<lle_laser_tile> tiles((size_t)std::max(0, lle_map_laser_tiles(map, nullptr, 0)));
    lle_map_laser_tiles(map, tiles.data(), (int)tiles.size());
    for (const auto& t : tiles) {
        if (t.i < 0 || t.i >= H || t.j < 0 || t.j >= W || t.laser_id < 0 || t.laser_id >= (int)src.size()) {
            err = "laser tile out of range";
            return false;
        }
        md.cells[(size_t)t.i * W + t.j] |= 1u << t.laser_id;
    }
    return true;
}

}  // namespace

struct lle_trails {
    int device = 0;
    hipStream_t stream = nullptr;
    lle_batch* batch = nullptr;
    MapData map;
    int64_t chunk = 0, max_states = 0;
    uint32_t* d_pool = nullptr;
    uint32_t* d_parent = nullptr;
    uint16_t* d_action = nullptr;
    uint32_t* d_table = nullptr;
    uint8_t* d_valid = nullptr;
    uint32_t* d_win = nullptr;
    uint32_t* d_cand_trail = nullptr;
    unsigned long long* d_counters = nullptr;
    uint32_t* d_cells = nullptr;
    std::vector<uint32_t> root;  // the record of the reset state, read from environment 0 right after lle_batch_create
    TrParams p{};
    // the last run
    int length = -1;
    std::vector<uint8_t> plan;
    std::vector<int64_t> frontier, expanded;
};

namespace {

int launch_piece(lle_trails* s, const TrParams& p) {
    const dim3 grid((p.n_items + lle::TR_THREADS - 1) / lle::TR_THREADS), block(lle::TR_THREADS);
    hipLaunchKernelGGL(lle::tr_expand, grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "tr_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(s->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, s->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    const size_t table_bytes = (size_t)p.rule.H * p.rule.W * 4;
    const bool in_lds = table_bytes <= lle::LDS_TABLE_MAX_BYTES;
    if (in_lds) hipLaunchKernelGGL((lle::tr_insert<true>), grid, block, (table_bytes + 15) / 16 * 16, s->stream, p);
    else hipLaunchKernelGGL((lle::tr_insert<false>), grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "tr_insert launch failed");
    hipLaunchKernelGGL(lle::tr_commit, grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "tr_commit launch failed");
    g_launched.fetch_or(1u | (in_lds ? 4u : 2u) | 8u);
    return LLE_OK;
}

}  // namespace

extern "C" {

const char* lle_trails_last_error(void) { return g_error.c_str(); }

void lle_trails_free(lle_trails* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    (void)hipStreamSynchronize(s->stream);
    if (s->batch) lle_batch_free(s->batch);
    (void)hipFree(s->d_pool);
    (void)hipFree(s->d_parent);
    (void)hipFree(s->d_action);
    (void)hipFree(s->d_table);
    (void)hipFree(s->d_valid);
    (void)hipFree(s->d_win);
    (void)hipFree(s->d_cand_trail);
    (void)hipFree(s->d_counters);
    (void)hipFree(s->d_cells);
    delete s;
}

lle_trails* lle_trails_create(const lle_map* map, const lle_trails_options* opt) {
    if (!map) {
        fail(LLE_ERR_NULL, "NULL map");
        return nullptr;
    }
    if (opt && opt->struct_bytes != sizeof(lle_trails_options)) {
        fail(LLE_ERR_ARG, "lle_trails_options.struct_bytes is not sizeof(lle_trails_options)");
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
    MapData md;
    if (lle_map_get_info(map, &md.info) != LLE_OK) {
        fail(LLE_ERR_ARG, "lle_map_get_info failed");
        return nullptr;
    }
    if (!sd::record_limits_ok(md.info, "more than 6 agents: a state has 5^A joint actions, the trail search serves maps of at most 6 agents (this map has "))
        return nullptr;
    std::string why;
    if (!build_rule(map, md, why)) {
        fail(LLE_ERR_UNSUPPORTED, why);
        return nullptr;
    }
    int device = -1;
    if (sd::choose_device(opt ? opt->device : -1, "no HIP device: the trail search runs on the GPU only (there is no CPU fallback)", &device) != LLE_OK)
        return nullptr;
    auto* s = new lle_trails();
    s->device = device;
    s->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    s->map = md;
    s->chunk = chunk;
    s->max_states = max_states;
    DeviceGuard g(device);
    s->batch = lle_batch_create(map, chunk, device, nullptr, 0, s->stream);
    if (!s->batch) {
        fail(LLE_ERR_HIP, std::string("lle_batch_create: ") + lle_last_error());
        lle_trails_free(s);
        return nullptr;
    }
    if (sd::bind_batch(s->batch, md.info, chunk, &s->p.b) != LLE_OK) {
        lle_trails_free(s);
        return nullptr;
    }
    const sl::RecordLayout lay = sl::make_layout(md.info.n_agents, md.info.n_beam_words, false);
    const uint64_t slots = sl::table_slots((uint64_t)max_states, (uint64_t)chunk);
    const size_t HW = (size_t)md.info.height * md.info.width;
    const size_t pool_bytes = (size_t)(lay.n_words + 1) * (size_t)max_states * 4;
    if (hipMalloc(&s->d_pool, pool_bytes) != hipSuccess || hipMalloc(&s->d_parent, (size_t)max_states * 4) != hipSuccess ||
        hipMalloc(&s->d_action, (size_t)max_states * 2) != hipSuccess || hipMalloc(&s->d_table, (size_t)slots * 4) != hipSuccess ||
        hipMalloc(&s->d_valid, (size_t)chunk) != hipSuccess || hipMalloc(&s->d_win, (size_t)chunk * 4) != hipSuccess ||
        hipMalloc(&s->d_cand_trail, (size_t)chunk * 4) != hipSuccess || hipMalloc(&s->d_counters, lle::CNT_COUNT * 8) != hipSuccess ||
        hipMalloc(&s->d_cells, std::max<size_t>(16, HW * 4)) != hipSuccess ||
        (HW > 0 && hipMemcpyAsync(s->d_cells, md.cells.data(), HW * 4, hipMemcpyHostToDevice, s->stream) != hipSuccess) ||
        hipStreamSynchronize(s->stream) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating the record pool failed (" + std::to_string(pool_bytes) + " bytes for " + std::to_string(max_states) + " records of " +
                              std::to_string(lay.n_words + 1) + " words)");
        lle_trails_free(s);
        return nullptr;
    }
    TrParams& p = s->p;
    p.pool = s->d_pool;
    p.parent = s->d_parent;
    p.action = s->d_action;
    p.table = s->d_table;
    p.valid = s->d_valid;
    p.win_slot = s->d_win;
    p.cand_trail = s->d_cand_trail;
    p.counters = s->d_counters;
    p.cells = s->d_cells;
    p.rule = md.rule;
    p.lay = lay;
    p.max_states = (uint32_t)max_states;
    p.table_mask = (uint32_t)(slots - 1);
    p.G = md.info.n_gems;
    p.n_joint = sl::pow5(md.info.n_agents);
    if (sd::read_root(p.b, lay, s->stream, &s->root) != LLE_OK) {  // the batch is freshly reset (World::new calls reset)
        lle_trails_free(s);
        return nullptr;
    }
    g_error.clear();
    return s;
}

int lle_trails_run(lle_trails* s, const lle_trails_args* args, lle_trails_result* result) {
    if (!args || !result) return fail(LLE_ERR_NULL, "NULL arguments or result");
    // (the arguments are judged before the handle is looked at: what they refuse they refuse on a machine without a device too)
    if (args->struct_bytes != sizeof(lle_trails_args)) return fail(LLE_ERR_ARG, "lle_trails_args.struct_bytes is not sizeof(lle_trails_args)");
    if (result->struct_bytes != sizeof(lle_trails_result)) return fail(LLE_ERR_ARG, "lle_trails_result.struct_bytes is not sizeof(lle_trails_result)");
    if (args->length_n < tl::MIN_LENGTH || args->length_n > tl::MAX_LENGTH)
        return fail(LLE_ERR_ARG, "length_n must be 2 .. 16: a sequence has at least two edges, and a field of the trail value has 4 bits");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    DeviceGuard g(s->device);
    const bool collect = args->collect_gems != 0;
    TrParams p = s->p;
    p.lay = sl::make_layout(s->map.info.n_agents, s->map.info.n_beam_words, collect);
    p.N = args->length_n;
    p.collect_gems = collect ? 1u : 0u;
    const sl::RecordLayout& r = p.lay;
    const int A = r.A;
    s->length = -1;
    s->plan.clear();
    s->frontier.assign(1, 1);
    s->expanded.clear();
    result->length = -1;
    result->n_states = 1;
    result->depth_reached = 0;
    result->trail = 0u;
    result->step_errors = 0;

    // ---- the reset state (t = 0: its edges count), judged on the host with the kernels' own functions
    const std::vector<uint32_t>& root = s->root;
    const uint32_t* cells = s->map.cells.data();
    const uint64_t root_edges = hl::state_edges([&](int w) { return root[(size_t)w]; }, r, p.rule, [&](int c) { return cells[c]; });
    int budget = tl::WALK_BUDGET;
    const uint32_t root_trail = tl::layer_update(0u, root_edges, p.N, A, budget);
    if (budget < 0)
        return fail(LLE_TRAILS_DENSE, "the arcs of the reset state allow more than " + std::to_string(tl::WALK_BUDGET) + " trail extensions: the search has no answer");
    if (sl::anybody_dead(root[(size_t)r.w_bits], A) || tl::violates_sequence(root_trail, p.N, A)) return LLE_OK;  // no plan starts here
    if (sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, collect, p.G)) {
        s->length = result->length = 0;
        result->trail = root_trail;
        return LLE_OK;
    }

    // ---- pool, table and counters: the root is record 0, under the hash of its key words and its trail word
    // (sd::seed_root hashes the first n_key words of what it copies; here the identity goes on behind the record, so the seed is laid out here)
    unsigned long long counters[lle::CNT_COUNT] = {};
    counters[lle::CNT_STATES] = 1;
    counters[lle::CNT_GOAL] = lle::NO_GOAL;
    const uint32_t none = 0xFFFFFFFFu, zero = 0u;
    const uint16_t zero16 = 0;
    std::vector<uint32_t> seed(root.begin(), root.begin() + r.n_words);  // the pool's words of record 0
    seed.push_back(root_trail);
    const uint64_t root_hash = sl::hash_record(tl::key_with_trail([&](int w) { return root[(size_t)w]; }, r.n_key, root_trail), r.n_key + 1);
    bool ok = hipMemsetAsync(p.table, 0xFF, ((size_t)p.table_mask + 1) * 4, s->stream) == hipSuccess &&
              hipMemcpyAsync(p.table + ((uint32_t)root_hash & p.table_mask), &zero, 4, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    for (size_t w = 0; ok && w < seed.size(); w++)
        ok = hipMemcpyAsync(p.pool + w * (size_t)p.max_states, &seed[w], 4, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(p.counters, counters, sizeof(counters), hipMemcpyHostToDevice, s->stream) == hipSuccess &&
         hipMemcpyAsync(p.parent, &none, 4, hipMemcpyHostToDevice, s->stream) == hipSuccess &&
         hipMemcpyAsync(p.action, &zero16, 2, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(s->stream) != hipSuccess) {  // (the sources are stack memory: copied before they change)
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "preparing the pool failed");
    }

    // ---- level by level
    uint64_t level_start = 0, level_end = 1;
    unsigned long long expanded_before = 0;
    int depth = 0;
    while (depth < args->t_max && level_end > level_start) {
        const uint64_t total = (level_end - level_start) * (uint64_t)p.n_joint;
        for (uint64_t item0 = 0; item0 < total; item0 += (uint64_t)s->chunk) {
            p.first_state = (uint32_t)level_start;
            p.item0 = item0;
            p.n_items = (uint32_t)std::min<uint64_t>((uint64_t)s->chunk, total - item0);
            const int rc = launch_piece(s, p);
            if (rc != LLE_OK) {
                (void)hipStreamSynchronize(s->stream);
                return rc;
            }
        }
        if (hipMemcpyAsync(counters, p.counters, sizeof(counters), hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
            (void)hipGetLastError();
            return fail(LLE_ERR_HIP, "reading the level's counters failed");
        }
        depth++;
        result->depth_reached = depth;
        result->step_errors = (int64_t)counters[lle::CNT_STEP_ERRORS];
        s->expanded.push_back((int64_t)(counters[lle::CNT_EXPANDED] - expanded_before));
        expanded_before = counters[lle::CNT_EXPANDED];
        const bool overflow = counters[lle::CNT_OVERFLOW] != 0ull || counters[lle::CNT_STATES] > (unsigned long long)p.max_states;
        if (overflow || counters[lle::CNT_DENSE] != 0ull) {  // no answer, never a partial one
            result->n_states = overflow ? s->max_states : 1;
            s->frontier.clear();
            s->frontier.push_back(1);
            s->expanded.clear();
            if (overflow)
                return fail(LLE_TRAILS_CAPACITY, "more than max_states = " + std::to_string(s->max_states) + " distinct records at depth " + std::to_string(depth) +
                                                     ": the search has no answer; create the handle with a larger max_states");
            return fail(LLE_TRAILS_DENSE, "the arcs of one state allow more than " + std::to_string(tl::WALK_BUDGET) + " trail extensions (" +
                                              std::to_string(counters[lle::CNT_DENSE]) + " work items at depth " + std::to_string(depth) + "): the search has no answer");
        }
        if (counters[lle::CNT_STEP_ERRORS] != 0ull)
            return fail(LLE_ERR_HIP, "the step refused " + std::to_string(counters[lle::CNT_STEP_ERRORS]) + " joint actions their availability masks allow");
        const uint64_t new_end = counters[lle::CNT_STATES];
        s->frontier.push_back((int64_t)(new_end - level_end));
        result->n_states = (int64_t)new_end;
        if (counters[lle::CNT_GOAL] != lle::NO_GOAL) {
            // ---- the goal's trail word, and the plan back through the parent links
            uint32_t at = (uint32_t)counters[lle::CNT_GOAL];
            uint32_t trail = 0u;
            if (at >= p.max_states || hipMemcpyAsync(&trail, p.pool + (size_t)r.n_words * p.max_states + at, 4, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
                hipStreamSynchronize(s->stream) != hipSuccess) {
                (void)hipGetLastError();
                return fail(LLE_ERR_HIP, "reading the goal's trail word failed");
            }
            s->plan.assign((size_t)depth * A, 4);
            for (int t = depth - 1; t >= 0; t--) {
                uint32_t parent = 0;
                uint16_t code = 0;
                if (at >= p.max_states || hipMemcpyAsync(&parent, p.parent + at, 4, hipMemcpyDeviceToHost, s->stream) != hipSuccess ||
                    hipMemcpyAsync(&code, p.action + at, 2, hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(LLE_ERR_HIP, "reading the plan back failed");
                }
                for (int a = 0; a < A; a++) {
                    s->plan[(size_t)t * A + a] = (uint8_t)(code % 5);
                    code /= 5;
                }
                at = parent;
            }
            if (at != 0u) return fail(LLE_ERR_HIP, "the parent links do not lead back to the reset state");
            s->length = result->length = depth;
            result->trail = trail;
            return LLE_OK;
        }
        level_start = level_end;
        level_end = new_end;
    }
    return LLE_OK;
}

int lle_trails_plan(const lle_trails* s, uint8_t* out, int64_t cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    if (s->length < 0) return fail(LLE_ERR_ARG, "the last run found no plan");
    if (s->length > 0 && (!out || cap < (int64_t)s->plan.size())) return fail(LLE_ERR_ARG, "the plan needs length * n_agents bytes");
    if (!s->plan.empty()) std::memcpy(out, s->plan.data(), s->plan.size());
    return s->length;
}

int lle_trails_stats(const lle_trails* s, int64_t* frontier, int64_t* expanded, int cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    for (int d = 0; frontier && d < std::min(cap, (int)s->frontier.size()); d++) frontier[d] = s->frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)s->expanded.size()); d++) expanded[d] = s->expanded[(size_t)d];
    return (int)s->frontier.size();
}

size_t lle_trails_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, g_launched.load(), buf, cap); }
size_t lle_trails_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, 0xFu, buf, cap); }

}  // extern "C"
