// search_core.hpp -- the single-tree search that search.hip, ../helpgraph/helpgraph.hip, ../trails/trails.hip and ../cycles/cycles.hip share: ONE breadth-first
// tree over the records of one map, with the extra words of a KIND behind them (search_logic.hpp: PlainKind, none; helpgraph_logic.hpp:
// HelpKind, two; trails_logic.hpp: TrailKind, one; ../cycles/cycles_logic.hpp:
// CycleKind, three or twenty-one).  Here are the shared kernel parameters and counters, the device bodies of the
// expand, insert and commit kernels, the handle with its device buffers, the two halves of a create, the seeding of record 0, the
// level loop with its counter read-back, the plan walk, and plan / stats.  A library keeps its extern "C" functions, its argument
// checks, the judgement of the reset state, its result struct and thin __global__ kernels under its own names, which stage the
// library's own static table in LDS where it has one (the tests of the table's sizes read that loop in the library's file).
// Everything here has internal linkage, as in search_device.hpp: every library keeps its own error string.
//
// A level is walked in pieces of at most `chunk` work items (frontier state, joint action), four launches each:
//   expand          lane k scatters the record of its state into environment k and writes its joint action; valid[k] says whether every
//                   component is in the state's availability mask (all 5^A codes are enumerated; the others are neither scattered nor inserted)
//   lle_batch_step  the unchanged step kernel
//   insert          lane k drops refused and deadly successors (insert_front) and whatever the library filters itself, works out the value
//                   of its kind from its parent's pool words and its own state in registers, drops what the kind rejects, hashes the
//                   record with the value's words and probes the table: an empty slot is claimed with a tag, an occupied one is compared
//                   word for word -- with the pool, or with the candidate the tag names.  That candidate's key words lie complete in the
//                   batch since the step, and its extra words are worked out AGAIN by the comparing lane, from that candidate's own
//                   parent's pool record, written by an earlier launch.  Nothing is handed from lane to lane inside the launch, so no
//                   lane waits and nothing needs a fence.
//   commit          every winner takes a pool index, copies its record and its extra words (kept for it, per candidate, by the insert:
//                   read in this later launch only), parent and action, puts the index where its tag was and reports a goal the kind accepts
// The host reads the counters once per level.
#ifndef LLE_SEARCH_CORE_HPP
#define LLE_SEARCH_CORE_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "search_device.hpp"
#include "search_logic.hpp"

namespace lle_search_core {
namespace {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
using sd::fail;

constexpr int THREADS = 256;  // lanes of a workgroup of every kernel that runs these bodies
enum { CNT_STATES = 0, CNT_EXPANDED, CNT_GOAL, CNT_OVERFLOW, CNT_STEP_ERRORS, CNT_DENSE /* the kinds with a walk: trail, cycle */, CNT_COUNT = 8 };
constexpr unsigned long long NO_GOAL = ~0ull;

struct Params {  // what every library's kernel parameters begin with
    sl::BatchView b;       // the batch (include/lle_hip.h buffer descriptors, read once)
    // the handle
    uint32_t* pool;        // [n_words + EXTRA][max_states]: the record, then the kind's extra words
    uint32_t* parent;      // [max_states]
    uint16_t* action;      // [max_states]
    uint32_t* table;       // [table_mask + 1]
    uint8_t* valid;        // [chunk]
    uint32_t* win_slot;    // [chunk]: the slot candidate k claimed, SLOT_EMPTY when it is no winner
    unsigned long long* counters;  // [CNT_COUNT]
    sl::RecordLayout lay;
    uint32_t max_states, table_mask;
    int32_t G;
    uint32_t collect_gems;
    // the piece
    uint32_t first_state;  // pool index of the frontier's first record
    uint32_t n_joint;      // 5^A
    uint64_t item0;        // first work item of the piece, counted over the level
    uint32_t n_items;      // <= chunk
};

// ================================================================================================ device side
struct Cells {  // a cell table of words, in LDS or in global memory
    const uint32_t* cells;
    __host__ __device__ uint32_t operator()(int c) const { return cells[c]; }
};

__device__ __forceinline__ uint32_t lane() { return blockIdx.x * THREADS + threadIdx.x; }

__device__ __forceinline__ void expand(const Params& p) {
    const uint32_t k = lane();
    bool valid = false;
    if (k < p.n_items) {
        const uint64_t item = p.item0 + k;
        const uint32_t s = p.first_state + (uint32_t)(item / p.n_joint);  // < the frontier's end <= max_states
        // (an invalid item leaves environment k as it is: whatever the step makes of it, the insert drops the item)
        valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{p.pool, p.max_states, s}, k, (uint32_t)(item % p.n_joint));
        p.valid[k] = valid ? 1 : 0;
    }
    if (valid) atomicAdd(&p.counters[CNT_EXPANDED], 1ull);
}

// Lane k < n_items of the insert, up to the library's own filters: does the successor in environment k go on to the table?
__device__ __forceinline__ bool insert_front(const Params& p, uint32_t k) {
    p.win_slot[k] = sl::SLOT_EMPTY;
    if (p.counters[CNT_OVERFLOW] != 0ull) return false;  // (set by an earlier launch: the search has failed already)
    if (!p.valid[k]) return false;
    if (p.b.err[k] != 0) {  // the step refused a joint action the mask allowed
        atomicAdd(&p.counters[CNT_STEP_ERRORS], 1ull);
        return false;
    }
    return !sl::anybody_dead(sl::env_word(p.b, p.lay, k, p.lay.w_bits), p.lay.A);
}

// The rest of lane k: the value of the kind, the hash, the probe.  cand[k] keeps a winner's value for the commit (no extra words: unused).
template <class Kind, class Cell>
__device__ __forceinline__ void insert_back(const Params& p, const Kind& kind, const Cell& cell, typename Kind::Value* cand, uint32_t k) {
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord rec{p.b, r, k};
    const sl::Piece who{p.b, 0, p.n_items, p.pool, p.max_states, p.max_states, p.first_state, p.item0, sl::ALL_ITEMS, p.n_joint};
    const uint64_t arcs = kind.state(rec, r, cell);
    typename Kind::Value value;
    if (!kind.successor(p.pool, p.max_states, r, sl::tag_parent(who, k), arcs, &value)) {  // the walk did not finish: the run has no answer
        atomicAdd(&p.counters[CNT_DENSE], 1ull);
        return;
    }
    if (kind.violates(value, r.A)) return;
    const auto me = sl::key_with_extra(rec, r.n_key, kind.words(value));
    const uint64_t h = sl::hash_record(me, r.n_key + Kind::EXTRA);
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, kind, arcs, occupant, me); };
    const int64_t slot = sl::table_insert(p.table, p.table_mask, h, sl::TAG_BIT | k, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) {
        p.win_slot[k] = (uint32_t)slot;
        if constexpr (Kind::EXTRA > 0) cand[k] = value;  // for the commit, a later launch; no lane of this launch reads it
    } else if (slot == sl::INSERT_FULL) {
        atomicMax(&p.counters[CNT_OVERFLOW], 1ull);
    }
}

template <class Kind>
__device__ __forceinline__ void commit(const Params& p, const Kind& kind, const typename Kind::Value* cand, uint32_t k) {
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
    typename Kind::Value value{};
    if constexpr (Kind::EXTRA > 0) value = cand[k];
    sl::copy_record(p.b, r, k, p.pool, p.max_states, idx);
    sl::store_pool_extra(p.pool, p.max_states, r, idx, kind.words(value));
    const uint64_t item = p.item0 + k;
    p.parent[idx] = p.first_state + (uint32_t)(item / p.n_joint);
    p.action[idx] = (uint16_t)(item % p.n_joint);
    p.table[slot] = (uint32_t)idx;
    if (sl::is_goal(rec(r.w_bits), rec(r.w_gems), r, p.collect_gems != 0u, p.G) && kind.accepts(value, r.A)) atomicMin(&p.counters[CNT_GOAL], idx);
}

// ================================================================================================ host side
// One map's cell table appended to `cells` (cells[i * W + j] = the sources that own a laser tile on the cell, bit laser_id) and its
// edge rule (helpgraph_logic.hpp: EdgeRule), from lle_map_laser_tiles / lle_map_sources.
template <class Rule>
bool build_rule(const lle_map* map, const lle_map_info& info, std::vector<uint32_t>& cells, Rule& rule, std::string& err) {
    const int H = info.height, W = info.width;
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    if (src.size() > 32) {
        err = "more than 32 sources: a cell's word has one bit per source";
        return false;
    }
    rule.A = info.n_agents;
    rule.H = H;
    rule.W = W;
    rule.enabled = 0u;
    for (int a = 0; a < sl::MAX_AGENTS; a++) rule.mine[a] = 0u;
    for (size_t l = 0; l < src.size(); l++) {
        if (src[l].enabled) rule.enabled |= 1u << l;
        if (src[l].agent_id >= 0 && src[l].agent_id < sl::MAX_AGENTS) rule.mine[src[l].agent_id] |= 1u << l;
    }
    const size_t base = cells.size();
    cells.resize(base + (size_t)H * W, 0u);
    std::vector<lle_laser_tile> tiles((size_t)std::max(0, lle_map_laser_tiles(map, nullptr, 0)));
    lle_map_laser_tiles(map, tiles.data(), (int)tiles.size());
    for (const auto& t : tiles) {
        if (t.i < 0 || t.i >= H || t.j < 0 || t.j >= W || t.laser_id < 0 || t.laser_id >= (int)src.size()) {
            err = "laser tile out of range";
            return false;
        }
        cells[base + (size_t)t.i * W + t.j] |= 1u << t.laser_id;
    }
    return true;
}

// What a library's texts and statuses differ by.
struct Library {
    const char* prefix;      // of its kernels' names: "search", "hg", "tr"
    const char* options;     // the name of its options struct
    const char* search;      // "the search", "the help-graph search", "the trail search"
    const char* record;      // what it calls a pool entry: "state", "record"
    const char* goal_words;  // what it calls the extra words: "help words", "trail word"
    int extra;               // words of a pool record behind the search's
    size_t cand_bytes;       // bytes per candidate between insert and commit
    int capacity_status, dense_status;  // LLE_*_CAPACITY, LLE_TRAILS_DENSE (0: the kind has no walk)
};

struct Options {  // a library's options struct, judged
    int64_t chunk, max_states;
    int device;
    hipStream_t stream;
    lle_map_info info;
};

struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    lle_batch* batch = nullptr;
    lle_map_info info{};
    int64_t chunk = 0, max_states = 0;
    uint32_t *d_pool = nullptr, *d_parent = nullptr, *d_table = nullptr, *d_win = nullptr;
    uint16_t* d_action = nullptr;
    uint8_t* d_valid = nullptr;
    void* d_cand = nullptr;   // [chunk] values of the kind
    unsigned long long* d_counters = nullptr;
    void* d_static = nullptr;  // the map's static table: foreign-beam bytes, or cell words
    std::vector<uint32_t> root;  // the record of the reset state, read from environment 0 right after lle_batch_create
    // the last run
    int length = -1;
    std::vector<uint8_t> plan;
    std::vector<int64_t> frontier, expanded;
};

// What a run reports, whatever the library's result struct calls it.
struct Outcome {
    int length = -1, depth_reached = 0;
    int64_t n_states = 1, step_errors = 0;
    unsigned long long dense = 0;        // work items whose walk ran out of budget, when the run ends with dense_status
    uint32_t goal_extra[sl::MAX_EXTRA] = {};  // the extra words of the plan's last state
};

// The kernels of one piece: insert is the instantiation this run launches, with `lds` bytes of dynamic LDS; `staged`: it is <true>.
template <class P>
struct Launch {
    void (*expand)(P);
    void (*insert)(P);
    void (*commit)(P);
    size_t lds;
    bool staged;
};

// create, first half: the map and the options.  `opt` may be NULL.
template <class O>
bool read_options(const lle_map* map, const O* opt, const Library& lib, Options* o) {
    if (!map) return fail(LLE_ERR_NULL, "NULL map"), false;
    if (opt && opt->struct_bytes != sizeof(O)) return fail(LLE_ERR_ARG, std::string(lib.options) + ".struct_bytes is not sizeof(" + lib.options + ")"), false;
    o->chunk = opt && opt->chunk ? opt->chunk : 65536;
    o->max_states = opt && opt->max_states ? opt->max_states : (int64_t)1 << 22;
    o->device = opt ? opt->device : -1;
    o->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    if (o->chunk < 1 || o->chunk > (int64_t)sl::MAX_CHUNK) return fail(LLE_ERR_ARG, "chunk must be 1 .. 2^30"), false;
    if (o->max_states < 1 || o->max_states > (int64_t)sl::MAX_STATES) return fail(LLE_ERR_ARG, "max_states must be 1 .. 2^30"), false;
    if (lle_map_get_info(map, &o->info) != LLE_OK) return fail(LLE_ERR_ARG, "lle_map_get_info failed"), false;
    return true;
}

// Everything of the handle on the device; the handle itself stays the caller's.
void close(Handle* s) {
    sd::DeviceGuard g(s->device);
    (void)hipStreamSynchronize(s->stream);
    if (s->batch) lle_batch_free(s->batch);
    void* const buffers[] = {s->d_pool, s->d_parent, s->d_action, s->d_table, s->d_valid, s->d_win, s->d_cand, s->d_counters, s->d_static};
    for (void* b : buffers) (void)hipFree(b);
}

// What a state record holds, refused in the library's words.
bool limits_ok(const lle_map_info& info, const Library& lib) {
    const std::string agents = std::string("more than 6 agents: a state has 5^A joint actions, ") + lib.search + " serves maps of at most 6 agents (this map has ";
    return sd::record_limits_ok(info, agents.c_str());
}

// create, second half: the device, the batch of `chunk` environments bound to p->b, the buffers (the static table of `static_bytes`
// copied up), the handle's part of *p, the reset state.  On failure nothing is left on the device.
int open(Handle* s, const lle_map* map, const Options& o, const Library& lib, const void* static_table, size_t static_bytes, Params* p) {
    const std::string no_device = std::string("no HIP device: ") + lib.search + " runs on the GPU only (there is no CPU fallback)";
    if (const int rc = sd::choose_device(o.device, no_device.c_str(), &s->device)) return rc;
    s->stream = o.stream;
    s->info = o.info;
    s->chunk = o.chunk;
    s->max_states = o.max_states;
    sd::DeviceGuard g(s->device);
    s->batch = lle_batch_create(map, o.chunk, s->device, nullptr, 0, s->stream);
    int rc = s->batch ? sd::bind_batch(s->batch, o.info, o.chunk, &p->b) : fail(LLE_ERR_HIP, std::string("lle_batch_create: ") + lle_last_error());
    const sl::RecordLayout lay = sl::make_layout(o.info.n_agents, o.info.n_beam_words, false);
    const uint64_t slots = sl::table_slots((uint64_t)o.max_states, (uint64_t)o.chunk);
    const size_t states = (size_t)o.max_states, chunk = (size_t)o.chunk, words = (size_t)(lay.n_words + lib.extra), pool_bytes = words * states * 4;
    if (rc == LLE_OK &&
        (hipMalloc(&s->d_pool, pool_bytes) != hipSuccess || hipMalloc(&s->d_parent, states * 4) != hipSuccess || hipMalloc(&s->d_action, states * 2) != hipSuccess ||
         hipMalloc(&s->d_table, (size_t)slots * 4) != hipSuccess || hipMalloc(&s->d_valid, chunk) != hipSuccess || hipMalloc(&s->d_win, chunk * 4) != hipSuccess ||
         (lib.cand_bytes > 0 && hipMalloc(&s->d_cand, chunk * lib.cand_bytes) != hipSuccess) || hipMalloc(&s->d_counters, CNT_COUNT * 8) != hipSuccess ||
         hipMalloc(&s->d_static, std::max<size_t>(16, static_bytes)) != hipSuccess ||
         (static_bytes > 0 && hipMemcpyAsync(s->d_static, static_table, static_bytes, hipMemcpyHostToDevice, s->stream) != hipSuccess) ||
         hipStreamSynchronize(s->stream) != hipSuccess)) {
        (void)hipGetLastError();
        rc = fail(LLE_ERR_HIP, std::string("allocating the ") + lib.record + " pool failed (" + std::to_string(pool_bytes) + " bytes for " + std::to_string(o.max_states) + " " +
                                   lib.record + "s of " + std::to_string(words) + " words)");
    }
    p->pool = s->d_pool;
    p->parent = s->d_parent;
    p->action = s->d_action;
    p->table = s->d_table;
    p->valid = s->d_valid;
    p->win_slot = s->d_win;
    p->counters = s->d_counters;
    p->lay = lay;
    p->max_states = (uint32_t)o.max_states;
    p->table_mask = (uint32_t)(slots - 1);
    p->G = o.info.n_gems;
    p->n_joint = sl::pow5(o.info.n_agents);
    if (rc == LLE_OK) rc = sd::read_root(p->b, lay, s->stream, &s->root);  // the batch is freshly reset (World::new calls reset)
    if (rc != LLE_OK) close(s);  // (the error text stays: nothing in there fails into it)
    else sd::g_error.clear();
    return rc;
}

// A run begins: the layout of this run's identity in *p, no plan and a frontier of the reset state alone in the handle.
void begin_run(Handle* s, Params* p, bool collect_gems) {
    p->lay = sl::make_layout(s->info.n_agents, s->info.n_beam_words, collect_gems);
    p->collect_gems = collect_gems ? 1u : 0u;
    s->length = -1;
    s->plan.clear();
    s->frontier.assign(1, 1);
    s->expanded.clear();
}

template <class P>
int launch_piece(Handle* s, const P& p, const Launch<P>& l, const Library& lib, std::atomic<uint32_t>& launched) {
    const dim3 grid((p.n_items + THREADS - 1) / THREADS), block(THREADS);
    hipLaunchKernelGGL(l.expand, grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, std::string(lib.prefix) + "_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(s->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, s->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    hipLaunchKernelGGL(l.insert, grid, block, l.lds, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, std::string(lib.prefix) + "_insert launch failed");
    hipLaunchKernelGGL(l.commit, grid, block, 0, s->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, std::string(lib.prefix) + "_commit launch failed");
    launched.fetch_or(1u | (l.staged ? 4u : 2u) | 8u);  // (the bits of the library's kernel name table: expand, insert<false>, insert<true>, commit)
    return LLE_OK;
}

// The search from the reset state `s->root` with the extra words `extra` (lib.extra of them), which the library has judged to be
// neither dead, rejected nor a goal: record 0, then level by level to depth t_max.  Fills *out on every path, plan and stats on success.
template <class P>
int search_tree(Handle* s, P& p, int t_max, const uint32_t* extra, const Launch<P>& l, const Library& lib, std::atomic<uint32_t>& launched, Outcome* out) {
    const sl::RecordLayout& r = p.lay;
    const int A = r.A;
    // ---- pool, table and counters: the root is record 0, under the hash of its key words and its extra words
    unsigned long long counters[CNT_COUNT] = {};
    counters[CNT_STATES] = 1;
    counters[CNT_GOAL] = NO_GOAL;
    const uint32_t none = 0xFFFFFFFFu;
    const uint16_t zero16 = 0;
    const bool ok = sd::seed_root(p.table, p.table_mask, p.pool, p.max_states, s->root.data(), r, s->stream, extra, lib.extra) &&
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
    while (depth < t_max && level_end > level_start) {
        const uint64_t total = (level_end - level_start) * (uint64_t)p.n_joint;
        for (uint64_t item0 = 0; item0 < total; item0 += (uint64_t)s->chunk) {
            p.first_state = (uint32_t)level_start;
            p.item0 = item0;
            p.n_items = (uint32_t)std::min<uint64_t>((uint64_t)s->chunk, total - item0);
            const int rc = launch_piece(s, p, l, lib, launched);
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
        out->depth_reached = depth;
        out->step_errors = (int64_t)counters[CNT_STEP_ERRORS];
        s->expanded.push_back((int64_t)(counters[CNT_EXPANDED] - expanded_before));
        expanded_before = counters[CNT_EXPANDED];
        const bool overflow = counters[CNT_OVERFLOW] != 0ull || counters[CNT_STATES] > (unsigned long long)p.max_states;
        if (overflow || (lib.dense_status != 0 && counters[CNT_DENSE] != 0ull)) {  // no answer, never a partial one; capacity goes first
            out->n_states = overflow ? s->max_states : 1;
            out->dense = counters[CNT_DENSE];
            s->frontier.assign(1, 1);
            s->expanded.clear();
            if (!overflow) return lib.dense_status;  // (the library has the text)
            return fail(lib.capacity_status, "more than max_states = " + std::to_string(s->max_states) + " distinct " + lib.record + "s at depth " + std::to_string(depth) +
                                                 ": the search has no answer; create the handle with a larger max_states");
        }
        if (counters[CNT_STEP_ERRORS] != 0ull)
            return fail(LLE_ERR_HIP, "the step refused " + std::to_string(counters[CNT_STEP_ERRORS]) + " joint actions their availability masks allow");
        const uint64_t new_end = counters[CNT_STATES];
        s->frontier.push_back((int64_t)(new_end - level_end));
        out->n_states = (int64_t)new_end;
        if (counters[CNT_GOAL] != NO_GOAL) {
            // ---- the goal's extra words, and the plan back through the parent links
            uint32_t at = (uint32_t)counters[CNT_GOAL];
            bool read = at < p.max_states;
            for (int x = 0; read && x < lib.extra; x++)
                read = hipMemcpyAsync(&out->goal_extra[x], p.pool + (size_t)(r.n_words + x) * p.max_states + at, 4, hipMemcpyDeviceToHost, s->stream) == hipSuccess;
            if (lib.extra > 0 && (!read || hipStreamSynchronize(s->stream) != hipSuccess)) {
                (void)hipGetLastError();
                return fail(LLE_ERR_HIP, std::string("reading the goal's ") + lib.goal_words + " failed");
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
            s->length = out->length = depth;
            return LLE_OK;
        }
        level_start = level_end;
        level_end = new_end;
    }
    return LLE_OK;
}

int plan(const Handle* s, uint8_t* out, int64_t cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    if (s->length < 0) return fail(LLE_ERR_ARG, "the last run found no plan");
    if (s->length > 0 && (!out || cap < (int64_t)s->plan.size())) return fail(LLE_ERR_ARG, "the plan needs length * n_agents bytes");
    if (!s->plan.empty()) std::memcpy(out, s->plan.data(), s->plan.size());
    return s->length;
}

int stats(const Handle* s, int64_t* frontier, int64_t* expanded, int cap) {
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    for (int d = 0; frontier && d < std::min(cap, (int)s->frontier.size()); d++) frontier[d] = s->frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)s->expanded.size()); d++) expanded[d] = s->expanded[(size_t)d];
    return (int)s->frontier.size();
}

}  // namespace
}  // namespace lle_search_core
#endif  // LLE_SEARCH_CORE_HPP
