// search.hip -- liblle_search.so: the exact shortest joint plan of a map by breadth-first search through the step kernel of
// liblle_hip.so (C ABI: include/lle_search.h; DESIGN.md "Shortest-plan search").
//
// The library touches a batch only through include/lle_hip.h: it owns an lle_batch of `chunk` environments, scatters frontier states
// into the batch's five dynamic-state buffers, steps the batch with lle_batch_step(LLE_STEP_NO_OBS) and reads the successors back out
// of the same buffers, so liblle_hip.so keeps its kernels.
//
// State: a pool of max_states records stored as structure of arrays (pool[w * max_states + s] = word w of state s: a wavefront's reads
// of word w are as dense as its state indices), parent (u32) and action (u16, base 5) per state, and an open-addressing table of u32
// slots.  The frontier of a level is a contiguous range of the pool; a work item is (frontier state, joint action); a level is walked
// in pieces of at most `chunk` items, four launches each:
//   search_expand   lane k scatters the record of its state into environment k and writes its joint action; valid[k] says whether every
//                   component is in the state's availability mask (all 5^A codes are enumerated; the others are neither scattered nor inserted)
//   lle_batch_step  the unchanged step kernel
//   search_insert   lane k drops refused, deadly and (no-cooperation) forbidden successors, hashes the rest and probes the table:
//                   an empty slot is claimed with a tag, an occupied one is compared word for word -- with the pool, or with the
//                   candidate the tag names, whose record lies complete in the batch since the step.  No lane waits for another.
//   search_commit   every winner takes a pool index, copies its record, parent and action, and puts the index where its tag was
// The host reads five counters once per level.
//
// What this file shares with ../forest/forest.hip and the steps-to-go library lives in two headers: search_logic.hpp (host and device:
// record layout, hash, table, and the record I/O between a batch, a pool and a table slot) and search_device.hpp (HIP: error string,
// device guard, batch binding, reset state, foreign-beam table).  Here are the counters, the LDS foreign table, the level loop and
// the plan walk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/lle_search.h"
#include "search_device.hpp"
#include "search_logic.hpp"

namespace lle {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;

constexpr int SEARCH_THREADS = 256;
enum { CNT_STATES = 0, CNT_EXPANDED, CNT_GOAL, CNT_OVERFLOW, CNT_STEP_ERRORS, CNT_COUNT = 8 };
constexpr unsigned long long NO_GOAL = ~0ull;

struct SearchParams {
    sl::BatchView b;       // the batch (include/lle_hip.h buffer descriptors, read once)
    // the handle
    uint32_t* pool;        // [n_words][max_states]
    uint32_t* parent;      // [max_states]
    uint16_t* action;      // [max_states]
    uint32_t* table;       // [table_mask + 1]
    uint8_t* valid;        // [chunk]
    uint32_t* win_slot;    // [chunk]: the slot candidate k claimed, SLOT_EMPTY when it is no winner
    unsigned long long* counters;  // [CNT_COUNT]
    const uint8_t* foreign;        // [H * W]: colours of the sources that own a laser tile on the cell (bit min(colour, 7))
    sl::RecordLayout lay;
    uint32_t max_states, table_mask;
    int32_t H, W, G;
    uint32_t mode, collect_gems;
    // the piece
    uint32_t first_state;  // pool index of the frontier's first state
    uint32_t n_joint;      // 5^A
    uint64_t item0;        // first work item of the piece, counted over the level
    uint32_t n_items;      // <= chunk
};

__global__ __launch_bounds__(SEARCH_THREADS) void search_expand(SearchParams p) {
    const uint32_t k = blockIdx.x * SEARCH_THREADS + threadIdx.x;
    bool valid = false;
    if (k < p.n_items) {
        const uint64_t item = p.item0 + k;
        const uint32_t s = p.first_state + (uint32_t)(item / p.n_joint);  // < the frontier's end <= max_states
        // (an invalid item leaves environment k as it is: whatever the step makes of it, search_insert drops the item)
        valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{p.pool, p.max_states, s}, k, (uint32_t)(item % p.n_joint));
        p.valid[k] = valid ? 1 : 0;
    }
    if (valid) atomicAdd(&p.counters[CNT_EXPANDED], 1ull);
}

// NO_COOP: mode no-cooperation, the foreign-beam table staged in LDS (one byte per cell: at most 255 x 255 bytes).
template <bool NO_COOP>
__global__ __launch_bounds__(SEARCH_THREADS) void search_insert(SearchParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_foreign[];
    if constexpr (NO_COOP) {
        const int HW = p.H * p.W;
        for (int c = threadIdx.x; c < HW; c += SEARCH_THREADS) lds_foreign[c] = p.foreign[c];
        __syncthreads();
    }
    const uint32_t k = blockIdx.x * SEARCH_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    p.win_slot[k] = sl::SLOT_EMPTY;
    if (p.counters[CNT_OVERFLOW] != 0ull) return;  // (set by an earlier launch: the search has failed already)
    if (!p.valid[k]) return;
    if (p.b.err[k] != 0) {  // the step refused a joint action the mask allowed
        atomicAdd(&p.counters[CNT_STEP_ERRORS], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    if (sl::anybody_dead(me(r.w_bits), r.A)) return;
    if constexpr (NO_COOP) {
        for (int a = 0; a < r.A; a++) {
            const uint8_t* q = p.b.pos + (int64_t)k * p.b.pos_stride + a * p.b.pos_agent_stride;
            const int i = q[0], j = q[1];
            if (i < p.H && j < p.W && sl::on_foreign_beam(lds_foreign[i * p.W + j], a)) return;
        }
    }
    const uint64_t h = sl::hash_record(me, r.n_key);
    const sl::Occupants who{p.b.key(), 0, p.n_items, p.pool, p.max_states, p.max_states};
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, occupant, me); };
    const int64_t slot = sl::table_insert(p.table, p.table_mask, h, sl::TAG_BIT | k, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) p.win_slot[k] = (uint32_t)slot;
    else if (slot == sl::INSERT_FULL) atomicMax(&p.counters[CNT_OVERFLOW], 1ull);
}

__global__ __launch_bounds__(SEARCH_THREADS) void search_commit(SearchParams p) {
    const uint32_t k = blockIdx.x * SEARCH_THREADS + threadIdx.x;
    if (k >= p.n_items) return;
    const uint32_t slot = p.win_slot[k];
    if (slot == sl::SLOT_EMPTY) return;
    const unsigned long long idx = atomicAdd(&p.counters[CNT_STATES], 1ull);
    if (idx >= (unsigned long long)p.max_states) {  // the pool is full: no answer (the tag stays; later launches return at once)
        atomicMax(&p.counters[CNT_OVERFLOW], 1ull);
        return;
    }
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord me{p.b, r, k};
    sl::copy_record(p.b, r, k, p.pool, p.max_states, idx);
    const uint64_t item = p.item0 + k;
    p.parent[idx] = p.first_state + (uint32_t)(item / p.n_joint);
    p.action[idx] = (uint16_t)(item % p.n_joint);
    p.table[slot] = (uint32_t)idx;
    if (sl::is_goal(me(r.w_bits), me(r.w_gems), r, p.collect_gems != 0u, p.G)) atomicMin(&p.counters[CNT_GOAL], idx);
}

template __global__ void search_insert<false>(SearchParams);
template __global__ void search_insert<true>(SearchParams);

}  // namespace lle

// ================================================================================================ host side
using lle::SearchParams;
namespace sl = lle_search_logic;
namespace sd = lle_search_device;
using sd::DeviceGuard;
using sd::fail;
using sd::g_error;

namespace {

std::atomic<uint32_t> g_launched{0};
const char* const KERNEL_NAMES[4] = {"search_expand", "search_insert<false>", "search_insert<true>", "search_commit"};
static_assert(LLE_SEARCH_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_search.h and search_logic.hpp disagree");

// Host copy of the static map data the search needs.
struct MapData {
    lle_map_info info{};
    std::vector<uint8_t> foreign;  // [H * W]
};

}  // namespace

struct lle_search {
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
    unsigned long long* d_counters = nullptr;
    uint8_t* d_foreign = nullptr;
    std::vector<uint32_t> root;  // the record of the reset state, read from environment 0 right after lle_batch_create
    SearchParams p{};
    // the last run
    int length = -1;
    std::vector<uint8_t> plan;
    std::vector<int64_t> frontier, expanded;
};

namespace {

int launch_piece(lle_search* s, const SearchParams& p) {
    const dim3 grid((p.n_items + lle::SEARCH_THREADS - 1) / lle::SEARCH_THREADS), block(lle::SEARCH_THREADS);
    hipLaunchKernelGGL(lle::search_expand, grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "search_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(s->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, s->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    if (p.mode == LLE_SEARCH_NO_COOPERATION) {
        const size_t lds = ((size_t)p.H * p.W + 15) / 16 * 16;
        hipLaunchKernelGGL((lle::search_insert<true>), grid, block, lds, s->stream, p);
    } else {
        hipLaunchKernelGGL((lle::search_insert<false>), grid, block, 0, s->stream, p);
    }
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "search_insert launch failed");
    hipLaunchKernelGGL(lle::search_commit, grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "search_commit launch failed");
    g_launched.fetch_or(1u | (p.mode == LLE_SEARCH_NO_COOPERATION ? 4u : 2u) | 8u);
    return LLE_OK;
}

}  // namespace

extern "C" {

const char* lle_search_last_error(void) { return g_error.c_str(); }

int lle_search_lower_bound(const lle_map* map) {
    if (!map) return fail(LLE_ERR_NULL, "NULL map");
    lle_map_info info{};
    if (lle_map_get_info(map, &info) != LLE_OK) return fail(LLE_ERR_ARG, "lle_map_get_info failed");
    const int H = info.height, W = info.width;
    enum : uint8_t { FREE = 0, BLOCKED = 1, EXIT = 2 };
    std::vector<uint8_t> kind((size_t)H * W, FREE);
    auto mark = [&](int which, uint8_t value) {
        std::vector<int32_t> ij((size_t)2 * std::max(0, lle_map_positions(map, which, nullptr, 0)));
        lle_map_positions(map, which, ij.data(), (int)ij.size() / 2);
        for (size_t k = 0; k + 1 < ij.size(); k += 2)
            if (ij[k] >= 0 && ij[k] < H && ij[k + 1] >= 0 && ij[k + 1] < W) kind[(size_t)ij[k] * W + ij[k + 1]] = value;
    };
    mark(LLE_POS_EXIT, EXIT);
    mark(LLE_POS_WALL, BLOCKED);
    mark(LLE_POS_VOID, BLOCKED);
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    for (const auto& q : src)
        if (q.i >= 0 && q.i < H && q.j >= 0 && q.j < W) kind[(size_t)q.i * W + q.j] = BLOCKED;
    std::vector<int32_t> starts((size_t)2 * std::max(0, lle_map_positions(map, LLE_POS_START, nullptr, 0)));
    lle_map_positions(map, LLE_POS_START, starts.data(), (int)starts.size() / 2);
    int bound = 0;
    for (size_t a = 0; a + 1 < starts.size(); a += 2) {
        if (starts[a] < 0 || starts[a] >= H || starts[a + 1] < 0 || starts[a + 1] >= W) continue;
        std::vector<int32_t> dist((size_t)H * W, -1);
        std::deque<int32_t> queue;
        const int32_t first = starts[a] * W + starts[a + 1];
        dist[(size_t)first] = 0;
        queue.push_back(first);
        int found = 0;  // an agent with no reachable exit counts 0
        while (!queue.empty()) {
            const int32_t c = queue.front();
            queue.pop_front();
            if (kind[(size_t)c] == EXIT) { found = dist[(size_t)c]; break; }  // (an exit has no outgoing move)
            const int i = c / W, j = c % W;
            const int di[4] = {-1, 1, 0, 0}, dj[4] = {0, 0, 1, -1};
            for (int d = 0; d < 4; d++) {
                const int ni = i + di[d], nj = j + dj[d];
                if (ni < 0 || ni >= H || nj < 0 || nj >= W) continue;
                const int32_t n = ni * W + nj;
                if (kind[(size_t)n] == BLOCKED || dist[(size_t)n] >= 0) continue;
                dist[(size_t)n] = dist[(size_t)c] + 1;
                queue.push_back(n);
            }
        }
        bound = std::max(bound, found);
    }
    return bound;
}

void lle_search_free(lle_search* s) {
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
    (void)hipFree(s->d_counters);
    (void)hipFree(s->d_foreign);
    delete s;
}

lle_search* lle_search_create(const lle_map* map, const lle_search_options* opt) {
    if (!map) {
        fail(LLE_ERR_NULL, "NULL map");
        return nullptr;
    }
    if (opt && opt->struct_bytes != sizeof(lle_search_options)) {
        fail(LLE_ERR_ARG, "lle_search_options.struct_bytes is not sizeof(lle_search_options)");
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
    if (!sd::build_foreign(map, md.info.height, md.info.width, md.foreign)) {
        fail(LLE_ERR_ARG, "laser tile out of range");
        return nullptr;
    }
    if (!sd::record_limits_ok(
            md.info, "more than 6 agents: a state has 5^A joint actions, the search serves maps of at most 6 agents (this map has "))
        return nullptr;
    int device = -1;
    if (sd::choose_device(opt ? opt->device : -1, "no HIP device: the search runs on the GPU only (there is no CPU fallback)", &device) != LLE_OK)
        return nullptr;
    auto* s = new lle_search();
    s->device = device;
    s->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    s->map = md;
    s->chunk = chunk;
    s->max_states = max_states;
    DeviceGuard g(device);
    s->batch = lle_batch_create(map, chunk, device, nullptr, 0, s->stream);
    if (!s->batch) {
        fail(LLE_ERR_HIP, std::string("lle_batch_create: ") + lle_last_error());
        lle_search_free(s);
        return nullptr;
    }
    if (sd::bind_batch(s->batch, md.info, chunk, &s->p.b) != LLE_OK) {
        lle_search_free(s);
        return nullptr;
    }
    const sl::RecordLayout lay = sl::make_layout(md.info.n_agents, md.info.n_beam_words, false);
    const uint64_t slots = sl::table_slots((uint64_t)max_states, (uint64_t)chunk);
    const size_t HW = (size_t)md.info.height * md.info.width;
    if (hipMalloc(&s->d_pool, (size_t)lay.n_words * (size_t)max_states * 4) != hipSuccess || hipMalloc(&s->d_parent, (size_t)max_states * 4) != hipSuccess ||
        hipMalloc(&s->d_action, (size_t)max_states * 2) != hipSuccess || hipMalloc(&s->d_table, (size_t)slots * 4) != hipSuccess ||
        hipMalloc(&s->d_valid, (size_t)chunk) != hipSuccess || hipMalloc(&s->d_win, (size_t)chunk * 4) != hipSuccess ||
        hipMalloc(&s->d_counters, lle::CNT_COUNT * 8) != hipSuccess || hipMalloc(&s->d_foreign, std::max<size_t>(16, HW)) != hipSuccess ||
        hipMemcpyAsync(s->d_foreign, md.foreign.data(), HW, hipMemcpyHostToDevice, s->stream) != hipSuccess ||
        hipStreamSynchronize(s->stream) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating the state pool failed (" + std::to_string((size_t)lay.n_words * (size_t)max_states * 4) + " bytes for " +
                              std::to_string(max_states) + " states of " + std::to_string(lay.n_words) + " words)");
        lle_search_free(s);
        return nullptr;
    }
    SearchParams& p = s->p;
    p.pool = s->d_pool;
    p.parent = s->d_parent;
    p.action = s->d_action;
    p.table = s->d_table;
    p.valid = s->d_valid;
    p.win_slot = s->d_win;
    p.counters = s->d_counters;
    p.foreign = s->d_foreign;
    p.lay = lay;
    p.max_states = (uint32_t)max_states;
    p.table_mask = (uint32_t)(slots - 1);
    p.H = md.info.height;
    p.W = md.info.width;
    p.G = md.info.n_gems;
    p.n_joint = sl::pow5(md.info.n_agents);
    if (sd::read_root(p.b, lay, s->stream, &s->root) != LLE_OK) {  // the batch is freshly reset (World::new calls reset)
        lle_search_free(s);
        return nullptr;
    }
    g_error.clear();
    return s;
}

int lle_search_run(lle_search* s, const lle_search_args* args, lle_search_result* result) {
    if (!s || !args || !result) return fail(LLE_ERR_NULL, "NULL handle, arguments or result");
    if (args->struct_bytes != sizeof(lle_search_args)) return fail(LLE_ERR_ARG, "lle_search_args.struct_bytes is not sizeof(lle_search_args)");
    if (result->struct_bytes != sizeof(lle_search_result)) return fail(LLE_ERR_ARG, "lle_search_result.struct_bytes is not sizeof(lle_search_result)");
    if (args->mode != LLE_SEARCH_STANDARD && args->mode != LLE_SEARCH_NO_COOPERATION) return fail(LLE_ERR_ARG, "unknown mode");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    DeviceGuard g(s->device);
    const bool collect = args->collect_gems != 0;
    SearchParams p = s->p;
    p.lay = sl::make_layout(s->map.info.n_agents, s->map.info.n_beam_words, collect);
    p.mode = (uint32_t)args->mode;
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
    result->pad = 0;
    result->step_errors = 0;

    // ---- the reset state, judged on the host with the kernels' own functions
    const std::vector<uint32_t>& root = s->root;
    if (sl::anybody_dead(root[(size_t)r.w_bits], A) ||
        (args->mode == LLE_SEARCH_NO_COOPERATION && sl::root_on_foreign_beam(root.data(), r, s->map.foreign.data(), p.H, p.W)))
        return LLE_OK;  // no plan starts here
    if (sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, collect, p.G)) {
        s->length = result->length = 0;
        return LLE_OK;
    }

    // ---- pool, table and counters
    unsigned long long counters[lle::CNT_COUNT] = {};
    counters[lle::CNT_STATES] = 1;
    counters[lle::CNT_GOAL] = lle::NO_GOAL;
    const uint32_t none = 0xFFFFFFFFu;
    const uint16_t zero16 = 0;
    const bool ok = sd::seed_root(p.table, p.table_mask, p.pool, p.max_states, root.data(), r, s->stream) &&
                    hipMemcpyAsync(p.counters, counters, sizeof(counters), hipMemcpyHostToDevice, s->stream) == hipSuccess &&
                    hipMemcpyAsync(p.parent, &none, 4, hipMemcpyHostToDevice, s->stream) == hipSuccess &&
                    hipMemcpyAsync(p.action, &zero16, 2, hipMemcpyHostToDevice, s->stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(s->stream) != hipSuccess) {  // (the sources are stack and handle memory: copied before they change)
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
        if (counters[lle::CNT_OVERFLOW] != 0ull || counters[lle::CNT_STATES] > (unsigned long long)p.max_states) {
            result->n_states = s->max_states;
            s->frontier.clear();
            s->frontier.push_back(1);
            s->expanded.clear();
            return fail(LLE_SEARCH_CAPACITY, "more than max_states = " + std::to_string(s->max_states) + " distinct states at depth " + std::to_string(depth) +
                                                 ": the search has no answer; create the handle with a larger max_states");
        }
        if (counters[lle::CNT_STEP_ERRORS] != 0ull)
            return fail(LLE_ERR_HIP, "the step refused " + std::to_string(counters[lle::CNT_STEP_ERRORS]) + " joint actions their availability masks allow");
        const uint64_t new_end = counters[lle::CNT_STATES];
        s->frontier.push_back((int64_t)(new_end - level_end));
        result->n_states = (int64_t)new_end;
        if (counters[lle::CNT_GOAL] != lle::NO_GOAL) {
            // ---- the plan, back through the parent links
            s->plan.assign((size_t)depth * A, 4);
            uint32_t at = (uint32_t)counters[lle::CNT_GOAL];
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
            return LLE_OK;
        }
        level_start = level_end;
        level_end = new_end;
    }
    return LLE_OK;
}

int lle_search_plan(const lle_search* s, uint8_t* out, int64_t cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    if (s->length < 0) return fail(LLE_ERR_ARG, "the last run found no plan");
    if (s->length > 0 && (!out || cap < (int64_t)s->plan.size())) return fail(LLE_ERR_ARG, "the plan needs length * n_agents bytes");
    if (!s->plan.empty()) std::memcpy(out, s->plan.data(), s->plan.size());
    return s->length;
}

int lle_search_stats(const lle_search* s, int64_t* frontier, int64_t* expanded, int cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    for (int d = 0; frontier && d < std::min(cap, (int)s->frontier.size()); d++) frontier[d] = s->frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)s->expanded.size()); d++) expanded[d] = s->expanded[(size_t)d];
    return (int)s->frontier.size();
}

size_t lle_search_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, g_launched.load(), buf, cap); }
size_t lle_search_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, 0xFu, buf, cap); }

}  // extern "C"
