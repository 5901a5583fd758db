// forest_core.hpp -- the many-tree search that forest.hip, ../helpforest/helpforest.hip and ../cycleforest/cycleforest.hip share: one
// breadth-first tree per map over the records of a KIND (../search/search_logic.hpp: PlainKind, no extra words;
// ../helpgraph/helpgraph_logic.hpp: HelpKind, two; ../trails/trails_logic.hpp: TrailKind, one; ../cycles/cycles_logic.hpp: CycleKind,
// three or twenty-one), every tree walked depth by depth in the same launches.  Here are the shared kernel
// parameters, the device bodies of the roots, seed, expand, insert, commit and plans kernels, the handle with its device and pinned
// buffers, the two halves of a create, the run from judged reset states (counters, seeding, the level loop with the per-map fates of
// forest_logic.hpp, the plan read-back), and plan / stats / occupancy.  A library keeps its extern "C" functions, its argument checks,
// the judgement of the reset states, its result struct, its static tables and thin __global__ kernels under its own names.
// Everything here has internal linkage, as in ../search/search_core.hpp: every library keeps its own error string.
//
// ONE lle_batch of n_maps * E environments, in which map m owns the environments [m * E, (m + 1) * E); per map a segment of the pool
// (seg_words arrays of `cap` words: the record, then the library's extra words), of parent, action and the table, and eight counters.
// A tag is LOCAL: TAG_BIT | (k % E).  A piece is the four launches of ../search/search_core.hpp (expand, lle_batch_step, insert,
// commit) over all n_maps * E lanes: lane k serves map k / E and item piece * E + k % E of it (forest_logic.hpp: lane_work) on the
// map's own segments and counters, or idles (valid = 0, nothing else written).
#ifndef LLE_FOREST_CORE_HPP
#define LLE_FOREST_CORE_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../search/search_device.hpp"
#include "forest_logic.hpp"

namespace lle_forest_core {
namespace {

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace fl = lle_forest_logic;
using sd::fail;

constexpr int THREADS = 256;  // lanes of a workgroup of every kernel that runs these bodies

struct Params {  // what every library's kernel parameters begin with
    sl::BatchView b;       // the batch (include/lle_hip.h buffer descriptors, read once)
    // the handle: one segment per map of each
    uint32_t* pool;        // [n_maps][seg_words][cap]: the record, then the extra words
    uint32_t* parent;      // [n_maps][cap]
    uint16_t* action;      // [n_maps][cap]
    uint32_t* table;       // [n_maps][slots]
    unsigned long long* counters;  // [n_maps][N_COUNTERS]
    uint32_t* roots;       // [n_maps][n_words]: the record of every map's reset state
    const fl::MapDescriptor* desc;  // [n_maps]
    uint8_t* valid;        // [n_lanes]
    uint32_t* win_slot;    // [n_lanes]: the slot (inside the map's segment) candidate k claimed, SLOT_EMPTY when it is no winner
    uint8_t* plans;        // [n_maps][plan_rows][A], then [n_maps] flags: the parent links led back to record 0
    sl::RecordLayout lay;
    uint64_t cap, slots;
    int64_t n_maps, E, n_lanes;
    int32_t G, seg_words;  // seg_words: word arrays of a map's pool segment (n_words + the library's extra words)
    int32_t extra_stride;  // words per map of root_extra and goal_extra: the library's extra words, whatever the kind's EXTRA
    uint32_t collect_gems, n_joint;
    int32_t plan_rows;
    // the piece
    uint64_t piece;
};

// ================================================================================================ device side
__device__ __forceinline__ int64_t lane() { return (int64_t)blockIdx.x * THREADS + threadIdx.x; }
// The pool segment of map `map`: word w of local record s at [w * cap + s].
__device__ __forceinline__ uint32_t* pool_segment(const Params& p, int64_t map) { return p.pool + fl::pool_segment_offset(map, p.seg_words, p.cap); }

// One lane per map: the record of the map's first environment (freshly reset) into roots.
__device__ __forceinline__ void roots(const Params& p) {
    const int64_t m = lane();
    if (m >= p.n_maps) return;
    const sl::EnvRecord rec{p.b, p.lay, fl::env_index(m, p.E, 0)};
    for (int w = 0; w < p.lay.n_words; w++) p.roots[m * p.lay.n_words + w] = rec(w);
}

// One lane per map: record 0 of a searching map is its reset state with the extra words the host worked out, under the hash of its
// identity (the table segment is all SLOT_EMPTY, the counters come from the host).
template <class Kind>
__device__ __forceinline__ void seed(const Params& p, const uint32_t* root_extra) {
    const int64_t m = lane();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const sl::RecordLayout& r = p.lay;
    const uint32_t* root = p.roots + m * r.n_words;
    uint32_t* seg = pool_segment(p, m);
    for (int w = 0; w < r.n_words; w++) seg[(uint64_t)w * p.cap] = root[w];
    sl::ExtraWords<Kind::EXTRA> x{};  // (the host hands the words over as the pool stores them)
    for (int i = 0; i < Kind::EXTRA; i++) x.w[i] = root_extra[(int64_t)p.extra_stride * m + i];
    sl::store_pool_extra(seg, p.cap, r, 0, x);
    const uint64_t h = sl::hash_record(sl::key_with_extra([&](int w) { return root[w]; }, r.n_key, x), r.n_key + Kind::EXTRA);
    p.table[fl::table_base(m, p.slots) + ((uint32_t)h & (uint32_t)(p.slots - 1))] = 0u;
    p.parent[fl::state_index(m, p.cap, 0)] = 0xFFFFFFFFu;
    p.action[fl::state_index(m, p.cap, 0)] = 0;
}

__device__ __forceinline__ void expand(const Params& p) {
    const int64_t k = lane();
    if (k >= p.n_lanes) return;
    const fl::LaneWork lw = fl::lane_work(k, p.piece, p.E, p.desc);
    if (lw.idle) {
        p.valid[k] = 0;
        return;
    }
    const uint32_t s = p.desc[lw.map].first_state + (uint32_t)(lw.item / p.n_joint);  // < the frontier's end <= cap
    // (an invalid item leaves environment k as it is: whatever the step makes of it, the insert drops the item)
    const bool valid = sl::scatter_item(p.b, p.lay, sl::PoolRecord{pool_segment(p, lw.map), p.cap, s}, k, (uint32_t)(lw.item % p.n_joint));
    p.valid[k] = valid ? 1 : 0;
    if (valid) atomicAdd(&p.counters[fl::counter_index(lw.map, fl::CNT_EXPANDED)], 1ull);
}

// Lane k of the insert, up to the library's own filters: does the successor in environment k go on to its map's table?
__device__ __forceinline__ bool insert_front(const Params& p, int64_t k) {
    if (k >= p.n_lanes || !p.valid[k]) return false;  // (an idle lane has valid = 0)
    p.win_slot[k] = sl::SLOT_EMPTY;
    unsigned long long* counters = p.counters + fl::counter_index(k / p.E, 0);
    if (counters[fl::CNT_OVERFLOW] != 0ull) return false;  // (set by an earlier launch: this map's search has failed already)
    if (p.b.err[k] != 0) {  // the step refused a joint action the mask allowed
        atomicAdd(&counters[fl::CNT_STEP_ERRORS], 1ull);
        return false;
    }
    return !sl::anybody_dead(sl::env_word(p.b, p.lay, k, p.lay.w_bits), p.lay.A);
}

// The rest of lane k: the value of the kind (of map k / E, as `cell` is), the hash, the probe.  cand[k] keeps a winner's value for
// the commit (no extra words: unused).  The extra words of a candidate a tag names are worked out again by the comparing lane, from
// environment map * E + tag and that candidate's own parent in the map's segment (sl::Piece, sl::occupant_is): nothing is handed from
// lane to lane inside the launch, no lane waits, nothing needs a fence.
template <class Kind, class Cell>
__device__ __forceinline__ void insert_back(const Params& p, const Kind& kind, const Cell& cell, typename Kind::Value* cand, int64_t k) {
    const int64_t map = k / p.E;
    const uint32_t local = (uint32_t)(k % p.E);
    unsigned long long* counters = p.counters + fl::counter_index(map, 0);
    const sl::RecordLayout& r = p.lay;
    const sl::EnvRecord rec{p.b, r, k};
    const fl::MapDescriptor d = p.desc[map];
    const uint32_t* seg = pool_segment(p, map);
    const sl::Piece who{p.b, fl::env_index(map, p.E, 0), (uint32_t)p.E, seg, p.cap, p.cap, d.first_state, p.piece * (uint64_t)p.E, d.items, p.n_joint};
    const uint64_t arcs = kind.state(rec, r, cell);
    typename Kind::Value value;
    // (the parent is < the frontier's end <= cap: the lane is not idle)
    if (!kind.successor(seg, p.cap, r, sl::tag_parent(who, local), arcs, &value)) {  // the walk did not finish: this map has no answer
        atomicAdd(&counters[fl::CNT_DENSE], 1ull);
        return;
    }
    if (kind.violates(value, r.A)) return;
    const auto me = sl::key_with_extra(rec, r.n_key, kind.words(value));
    auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, kind, arcs, occupant, me); };
    const int64_t slot = sl::table_insert(p.table + fl::table_base(map, p.slots), (uint32_t)(p.slots - 1), sl::hash_record(me, r.n_key + Kind::EXTRA),
                                          sl::TAG_BIT | local, sd::SlotLoad{}, sd::SlotCas{}, same_as);
    if (slot >= 0) {
        p.win_slot[k] = (uint32_t)slot;
        if constexpr (Kind::EXTRA > 0) cand[k] = value;  // for the commit, a later launch; no lane of this launch reads it
    } else if (slot == sl::INSERT_FULL) {
        atomicMax(&counters[fl::CNT_OVERFLOW], 1ull);
    }
}

// Does lane k of the commit hold a slot of its map's table?  (Only then does a kernel read what it makes the map's kind from.)
__device__ __forceinline__ bool is_winner(const Params& p, int64_t k) { return k < p.n_lanes && p.valid[k] && p.win_slot[k] != sl::SLOT_EMPTY; }

template <class Kind>
__device__ __forceinline__ void commit(const Params& p, const Kind& kind, const typename Kind::Value* cand, int64_t k) {
    const uint32_t slot = p.win_slot[k];
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
    typename Kind::Value value{};
    if constexpr (Kind::EXTRA > 0) value = cand[k];
    sl::copy_record(p.b, r, k, seg, p.cap, idx);
    sl::store_pool_extra(seg, p.cap, r, idx, kind.words(value));
    const uint64_t item = p.piece * (uint64_t)p.E + (uint64_t)(k % p.E);
    p.parent[fl::state_index(map, p.cap, idx)] = p.desc[map].first_state + (uint32_t)(item / p.n_joint);
    p.action[fl::state_index(map, p.cap, idx)] = (uint16_t)(item % p.n_joint);
    p.table[fl::table_base(map, p.slots) + slot] = (uint32_t)idx;
    if (sl::is_goal(rec(r.w_bits), rec(r.w_gems), r, p.collect_gems != 0u, p.G) && kind.accepts(value, r.A)) atomicMin(&counters[fl::CNT_GOAL], idx);
}

// One lane per map; desc[m]: active = solved, first_state = the goal record, items = the plan's length (<= plan_rows).  Walks the
// parent links and fetches the goal's extra words.
template <class Kind>
__device__ __forceinline__ void plans(const Params& p, uint32_t* goal_extra) {
    const int64_t m = lane();
    if (m >= p.n_maps || !p.desc[m].active) return;
    const int A = p.lay.A;
    uint8_t* rows = p.plans + (uint64_t)m * (uint64_t)p.plan_rows * (uint64_t)A;
    uint8_t* flags = p.plans + (uint64_t)p.n_maps * (uint64_t)p.plan_rows * (uint64_t)A;
    uint64_t at = p.desc[m].first_state;
    if constexpr (Kind::EXTRA > 0) {
        const uint32_t* seg = pool_segment(p, m);
        for (int w = 0; w < Kind::EXTRA; w++) goal_extra[(int64_t)p.extra_stride * m + w] = at < p.cap ? seg[(uint64_t)(p.lay.n_words + w) * p.cap + at] : 0u;
    }
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

// ================================================================================================ host side
// What a library's texts and statuses differ by.
struct Library {
    const char* prefix;   // of its kernels' names: "forest", "hf", "cf"
    const char* options;  // the name of its options struct
    const char* search;   // "the search", "the help forest"
    const char* record;   // what it calls a pool entry: "state", "record"
    int extra;            // word arrays of a map's pool segment behind the record's, and words per map of root_extra and goal_extra: 0; 2
                          // whichever kind of the help forest runs; 3 or 21 by the agent class of the cycle forest's maps
    int capacity_status, dense_status;  // LLE_*_CAPACITY, LLE_TRAILS_DENSE / LLE_CYCLES_DENSE (0: the kind has no walk)
    size_t cand_bytes;    // bytes per lane of the winner buffer between insert and commit: the largest sizeof(Kind::Value) (no extra words: 0)
};

struct Options {  // a library's options struct, judged
    int64_t E, cap;
    int device;
    hipStream_t stream;
    lle_map_info info;  // of map 0: the maps agree on everything the search reads from it
};

struct Table {  // a static table of the library's, all maps' behind each other: uploaded once at creation
    const void* data;
    size_t bytes;
};

struct MapRun {  // one map in the last run
    fl::MapProgress progress{};
    std::vector<int64_t> frontier, expanded;
    std::vector<uint8_t> plan;
    uint32_t extra[sl::MAX_EXTRA] = {};  // of the plan's last state (no extra words: unused)
};

struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    lle_batch* batch = nullptr;
    lle_map_info info{};
    int64_t n_maps = 0, E = 0, cap = 0;
    std::vector<uint32_t> roots;  // [n_maps][n_words]
    uint32_t *d_pool = nullptr, *d_parent = nullptr, *d_table = nullptr, *d_win = nullptr, *d_roots = nullptr;
    uint16_t* d_action = nullptr;
    uint8_t *d_valid = nullptr, *d_plans = nullptr;
    unsigned long long* d_counters = nullptr;
    fl::MapDescriptor* d_desc = nullptr;
    void* d_static[2] = {nullptr, nullptr};  // the library's static tables
    size_t plans_bytes = 0;
    // a library with extra words
    void* d_cand = nullptr;  // [n_lanes] of the library's cand_bytes: the value of winner k as its kind keeps it, for the commit
    uint32_t *d_root_extra = nullptr, *d_goal_extra = nullptr;  // [n_maps][extra]: of every map's reset state in this run, of every solved map's goal
    // pinned: what the host reads and writes once per level, and once per run
    fl::MapDescriptor* h_desc = nullptr;
    uint64_t* h_counters = nullptr;
    uint32_t* h_extra = nullptr;  // [n_maps][extra]: up, the reset states' extra words; down, the goals'
    int extra = 0;                // the library's extra words
    // the last run
    std::vector<MapRun> maps;
    int64_t valid_items = 0, launched_lanes = 0;
};

// The kernels of one run (insert: the instantiation it launches, with `insert_lds` bytes of dynamic LDS) and their bits in the library's
// kernel name table.
template <class P>
struct Launch {
    void (*seed)(P);
    void (*expand)(P);
    void (*insert)(P);
    void (*commit)(P);
    void (*plans)(P);
    uint32_t seed_bit, piece_bits, plans_bit;
    size_t insert_lds = 0;
};

dim3 grid_for(int64_t lanes) { return dim3((unsigned)((lanes + THREADS - 1) / THREADS)); }

// create, first half: the maps and the options.  `opt` may be NULL.
template <class O>
bool read_options(const lle_map* const* maps, int n_maps, const O* opt, const Library& lib, Options* o) {
    if (!maps) return fail(LLE_ERR_NULL, "NULL maps"), false;
    if (n_maps < 1) return fail(LLE_ERR_ARG, "n_maps must be at least 1"), false;
    for (int m = 0; m < n_maps; m++)
        if (!maps[m]) return fail(LLE_ERR_NULL, "NULL map (entry " + std::to_string(m) + ")"), false;
    if (opt && opt->struct_bytes != sizeof(O)) return fail(LLE_ERR_ARG, std::string(lib.options) + ".struct_bytes is not sizeof(" + lib.options + ")"), false;
    o->E = opt && opt->envs_per_map ? opt->envs_per_map : 256;
    o->cap = opt && opt->max_states_per_map ? opt->max_states_per_map : 65536;
    o->device = opt ? opt->device : -1;
    o->stream = reinterpret_cast<hipStream_t>(opt ? opt->stream : nullptr);
    if (o->E < 1 || o->E > fl::MAX_ENVS_PER_MAP) return fail(LLE_ERR_ARG, "envs_per_map must be 1 .. 2^30"), false;
    if (o->cap < 1 || o->cap > fl::MAX_STATES_PER_MAP) return fail(LLE_ERR_ARG, "max_states_per_map must be 1 .. 2^30"), false;
    if ((int64_t)n_maps * o->E > fl::MAX_LANES) return fail(LLE_ERR_ARG, "n_maps * envs_per_map must be at most 2^30"), false;
    if (fl::table_slots((uint64_t)o->cap, (uint64_t)o->E) > fl::MAX_TABLE_SLOTS)
        return fail(LLE_ERR_ARG, "max_states_per_map + envs_per_map must be below 2^31 (a table segment has at most 2^31 slots)"), false;
    if (lle_map_get_info(maps[0], &o->info) != LLE_OK) return fail(LLE_ERR_ARG, "lle_map_get_info failed"), false;
    const std::string agents = std::string("more than 6 agents: a state has 5^A joint actions, ") + lib.search + " serves maps of at most 6 agents (these maps have ";
    if (!sd::record_limits_ok(o->info, agents.c_str())) return false;
    // the shapes, judged by the step library itself without a device: its refusal is the one lle_batch_create_multi would give
    if (lle_batch_arena_bytes_multi(maps, n_maps, o->E) < 0) return fail(LLE_ERR_ARG, std::string("lle_batch_create_multi: ") + lle_last_error()), false;
    return true;
}

// Everything of the handle on the device and in pinned memory; the handle itself stays the caller's.
void close(Handle* f) {
    sd::DeviceGuard g(f->device);
    (void)hipStreamSynchronize(f->stream);
    if (f->batch) lle_batch_free(f->batch);
    void* const buffers[] = {f->d_pool, f->d_parent, f->d_action, f->d_table,     f->d_valid,     f->d_win,  f->d_counters,   f->d_roots,
                             f->d_desc, f->d_plans,  f->d_static[0], f->d_static[1], f->d_cand, f->d_root_extra, f->d_goal_extra};
    for (void* b : buffers) (void)hipFree(b);
    void* const pinned[] = {f->h_desc, f->h_counters, f->h_extra};
    for (void* b : pinned)
        if (b) (void)hipHostFree(b);
}

// create, second half: the device, the batch of n_maps * E environments bound to p->b, the buffers (the library's static tables
// copied up into d_static, from memory that outlives the copy), the handle's part of *p, every map's reset state by the library's
// `roots_kernel`.  On failure nothing is left on the device.
template <class P>
int open(Handle* f, const lle_map* const* maps, int n_maps, const Options& o, const Library& lib, const Table (&tables)[2], P* p, void (*roots_kernel)(P)) {
    const std::string no_device = std::string("no HIP device: ") + lib.search + " runs on the GPU only (there is no CPU fallback)";
    if (const int rc = sd::choose_device(o.device, no_device.c_str(), &f->device)) return rc;
    f->stream = o.stream;
    f->info = o.info;
    f->n_maps = n_maps;
    f->E = o.E;
    f->cap = o.cap;
    f->maps.assign((size_t)n_maps, MapRun{});
    for (auto& mr : f->maps) mr.progress = fl::fresh_progress(false);
    sd::DeviceGuard g(f->device);
    auto give_up = [&](int rc) {  // (the error text stays: nothing in close fails into it)
        close(f);
        return rc;
    };
    f->batch = lle_batch_create_multi(maps, n_maps, o.E, f->device, nullptr, 0, f->stream);
    if (!f->batch) return give_up(fail(LLE_ERR_HIP, std::string("lle_batch_create_multi: ") + lle_last_error()));
    if (const int rc = sd::bind_batch(f->batch, o.info, (int64_t)n_maps * o.E, &p->b)) return give_up(rc);
    const sl::RecordLayout lay = sl::make_layout(o.info.n_agents, o.info.n_beam_words, false);
    const uint64_t slots = fl::table_slots((uint64_t)o.cap, (uint64_t)o.E);
    const size_t M = (size_t)n_maps, lanes = M * (size_t)o.E, cap = (size_t)o.cap, words = (size_t)(lay.n_words + lib.extra);
    const size_t pool_bytes = M * words * cap * 4;
    bool ok = hipMalloc(&f->d_pool, pool_bytes) == hipSuccess && hipMalloc(&f->d_parent, M * cap * 4) == hipSuccess &&
              hipMalloc(&f->d_action, M * cap * 2) == hipSuccess && hipMalloc(&f->d_table, M * (size_t)slots * 4) == hipSuccess &&
              hipMalloc(&f->d_valid, lanes) == hipSuccess && hipMalloc(&f->d_win, lanes * 4) == hipSuccess &&
              hipMalloc(&f->d_counters, M * fl::N_COUNTERS * 8) == hipSuccess && hipMalloc(&f->d_roots, M * (size_t)lay.n_words * 4) == hipSuccess &&
              hipMalloc(&f->d_desc, M * sizeof(fl::MapDescriptor)) == hipSuccess && hipHostMalloc(&f->h_desc, M * sizeof(fl::MapDescriptor)) == hipSuccess &&
              hipHostMalloc(&f->h_counters, M * fl::N_COUNTERS * 8) == hipSuccess;
    f->extra = lib.extra;
    const size_t extra_bytes = M * (size_t)lib.extra * 4;
    if (lib.extra > 0)
        ok = ok && hipMalloc(&f->d_cand, lanes * lib.cand_bytes) == hipSuccess && hipMalloc(&f->d_root_extra, extra_bytes) == hipSuccess &&
             hipMalloc(&f->d_goal_extra, extra_bytes) == hipSuccess && hipHostMalloc(&f->h_extra, extra_bytes) == hipSuccess;
    for (int t = 0; t < 2; t++)
        if (tables[t].bytes > 0)
            ok = ok && hipMalloc(&f->d_static[t], tables[t].bytes) == hipSuccess &&
                 hipMemcpyAsync(f->d_static[t], tables[t].data, tables[t].bytes, hipMemcpyHostToDevice, f->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return give_up(fail(LLE_ERR_HIP, std::string("allocating the ") + lib.record + " pools failed (" + std::to_string(pool_bytes) + " bytes for " +
                                             std::to_string(n_maps) + " maps of " + std::to_string(o.cap) + " " + lib.record + "s of " + std::to_string(words) +
                                             " words)"));
    }
    p->pool = f->d_pool;
    p->parent = f->d_parent;
    p->action = f->d_action;
    p->table = f->d_table;
    p->counters = f->d_counters;
    p->roots = f->d_roots;
    p->desc = f->d_desc;
    p->valid = f->d_valid;
    p->win_slot = f->d_win;
    p->plans = nullptr;
    p->lay = lay;
    p->cap = (uint64_t)o.cap;
    p->slots = slots;
    p->n_maps = n_maps;
    p->E = o.E;
    p->n_lanes = (int64_t)n_maps * o.E;
    p->G = o.info.n_gems;
    p->seg_words = (int32_t)words;
    p->extra_stride = lib.extra;
    p->n_joint = sl::pow5(o.info.n_agents);
    // ---- every map's reset state (the batch is freshly reset: World::new calls reset)
    f->roots.assign(M * (size_t)lay.n_words, 0u);
    hipLaunchKernelGGL(roots_kernel, grid_for(n_maps), dim3(THREADS), 0, f->stream, *p);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(f->roots.data(), f->d_roots, f->roots.size() * 4, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
        hipStreamSynchronize(f->stream) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(fail(LLE_ERR_HIP, "reading the reset states failed"));
    }
    sd::g_error.clear();
    return LLE_OK;
}

// A run begins: the layout of this run's identity in *p; no plan, no extra words and a frontier of the reset state alone for every map.
template <class P>
void begin_run(Handle* f, P* p, bool collect_gems) {
    p->lay = sl::make_layout(f->info.n_agents, f->info.n_beam_words, collect_gems);
    p->collect_gems = collect_gems ? 1u : 0u;
    f->valid_items = f->launched_lanes = 0;
    for (MapRun& mr : f->maps) {
        mr.frontier.assign(1, 1);
        mr.expanded.clear();
        mr.plan.clear();
        std::fill(mr.extra, mr.extra + sl::MAX_EXTRA, 0u);
    }
    if (f->h_extra) std::fill(f->h_extra, f->h_extra + (size_t)f->extra * f->maps.size(), 0u);
}

template <class P>
int launch_piece(Handle* f, const P& p, const Launch<P>& l, const Library& lib, std::atomic<uint32_t>& launched) {
    const dim3 grid = grid_for(p.n_lanes), block(THREADS);
    hipLaunchKernelGGL(l.expand, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, std::string(lib.prefix) + "_expand launch failed");
    // (actions in LLE_BUF_ACTIONS; no auto-reset, no sampling, no observation)
    if (lle_batch_step(f->batch, nullptr, LLE_STEP_NO_OBS, 0, 0, 0, f->stream) != LLE_OK) return fail(LLE_ERR_HIP, std::string("lle_batch_step: ") + lle_last_error());
    hipLaunchKernelGGL(l.insert, grid, block, l.insert_lds, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, std::string(lib.prefix) + "_insert launch failed");
    hipLaunchKernelGGL(l.commit, grid, block, 0, f->stream, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, std::string(lib.prefix) + "_commit launch failed");
    launched.fetch_or(l.piece_bits);
    return LLE_OK;
}

// h_desc to the device (the pinned buffer is not written again before the stream has been synchronised).
bool upload_descriptors(Handle* f) {
    return hipMemcpyAsync(f->d_desc, f->h_desc, (size_t)f->n_maps * sizeof(fl::MapDescriptor), hipMemcpyHostToDevice, f->stream) == hipSuccess;
}

// A HIP call of a run failed: the stream is drained, so that nothing still reads or writes the pinned buffers when the caller returns.
int hip_failed(Handle* f, const char* what) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(f->stream);
    return fail(LLE_ERR_HIP, what);
}

// The search of every map from its reset state, which the library has judged: maps[m].progress says whether map m searches, h_extra
// holds the reset states' extra words (lib.extra > 0).  Record 0 of every searching map, then level by level to depth t_max, all
// maps in lock-step, then the plans of the solved maps.  `report` fills the library's result structs from maps[]: called on success,
// and where a map's own counters or parent links end the run.
template <class P, class Report>
int run(Handle* f, P& p, int t_max, const Launch<P>& l, const Library& lib, std::atomic<uint32_t>& launched, const Report& report) {
    const size_t M = (size_t)f->n_maps, A = (size_t)p.lay.A;
    bool any_active = false;
    for (size_t m = 0; m < M; m++) {
        uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
        std::fill(c, c + fl::N_COUNTERS, 0ull);
        c[fl::CNT_STATES] = 1;
        c[fl::CNT_GOAL] = fl::NO_GOAL;
        f->h_desc[m] = fl::level_descriptor(f->maps[m].progress, p.n_joint);
        any_active = any_active || f->maps[m].progress.active;
    }
    if (!any_active || t_max == 0) return report(), LLE_OK;

    // ---- tables, counters and record 0 of every searching map
    bool ok = hipMemsetAsync(p.table, 0xFF, M * (size_t)p.slots * 4, f->stream) == hipSuccess &&
              hipMemcpyAsync(p.counters, f->h_counters, M * fl::N_COUNTERS * 8, hipMemcpyHostToDevice, f->stream) == hipSuccess &&
              (lib.extra == 0 || hipMemcpyAsync(f->d_root_extra, f->h_extra, M * (size_t)lib.extra * 4, hipMemcpyHostToDevice, f->stream) == hipSuccess) &&
              upload_descriptors(f);
    if (ok) {
        hipLaunchKernelGGL(l.seed, grid_for(f->n_maps), dim3(THREADS), 0, f->stream, p);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) return hip_failed(f, "preparing the pools failed");
    launched.fetch_or(l.seed_bit);

    // ---- level by level, all maps in lock-step (the first level's descriptors are on their way already)
    int depth = 0;
    while (depth < t_max && any_active) {
        if (depth > 0) {
            for (size_t m = 0; m < M; m++) f->h_desc[m] = fl::level_descriptor(f->maps[m].progress, p.n_joint);
            if (!upload_descriptors(f)) return hip_failed(f, "writing the level's descriptors failed");
        }
        const uint64_t pieces = fl::piece_count(f->h_desc, f->n_maps, f->E);
        f->valid_items += (int64_t)fl::level_items(f->h_desc, f->n_maps);
        f->launched_lanes += (int64_t)pieces * p.n_lanes;
        for (uint64_t q = 0; q < pieces; q++) {
            p.piece = q;
            if (const int rc = launch_piece(f, p, l, lib, launched)) {
                (void)hipStreamSynchronize(f->stream);
                return rc;
            }
        }
        if (hipMemcpyAsync(f->h_counters, p.counters, M * fl::N_COUNTERS * 8, hipMemcpyDeviceToHost, f->stream) != hipSuccess ||
            hipStreamSynchronize(f->stream) != hipSuccess)
            return hip_failed(f, "reading the level's counters failed");
        depth++;
        any_active = false;
        for (size_t m = 0; m < M; m++) {
            MapRun& mr = f->maps[m];
            if (!mr.progress.active) continue;
            const uint64_t* c = f->h_counters + fl::counter_index((int64_t)m, 0);
            int64_t frontier_new = 0, expanded_new = 0;
            const int fate = fl::advance(mr.progress, c, p.cap, depth, lib.capacity_status, lib.dense_status, &frontier_new, &expanded_new);
            if (fate == fl::FATE_STEP_ERROR) {
                report();
                return fail(LLE_ERR_HIP, "the step refused " + std::to_string(c[fl::CNT_STEP_ERRORS]) + " joint actions their availability masks allow (map " +
                                             std::to_string(m) + ")");
            }
            if (fate == fl::FATE_CAPACITY || fate == fl::FATE_DENSE) {  // this map alone has no answer
                mr.frontier.assign(1, 1);
                mr.expanded.clear();
                continue;
            }
            mr.frontier.push_back(frontier_new);
            mr.expanded.push_back(expanded_new);
            any_active = any_active || mr.progress.active;
        }
    }

    // ---- the plans of the solved maps: one launch walks the parent links and fetches the goals' extra words, one copy of each brings them back
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
        const size_t bytes = M * (size_t)rows * A + M;
        if (bytes > f->plans_bytes) {
            (void)hipFree(f->d_plans);
            f->d_plans = nullptr;
            f->plans_bytes = 0;
            if (hipMalloc(&f->d_plans, bytes) != hipSuccess) return hip_failed(f, "allocating the plan buffer failed");
            f->plans_bytes = bytes;
        }
        p.plans = f->d_plans;
        p.plan_rows = rows;
        std::vector<uint8_t> host(bytes, 0);
        ok = upload_descriptors(f);
        if (ok) {
            hipLaunchKernelGGL(l.plans, grid_for(f->n_maps), dim3(THREADS), 0, f->stream, p);
            ok = hipGetLastError() == hipSuccess;
        }
        ok = ok && hipMemcpyAsync(host.data(), f->d_plans, bytes, hipMemcpyDeviceToHost, f->stream) == hipSuccess &&
             (lib.extra == 0 || hipMemcpyAsync(f->h_extra, f->d_goal_extra, M * (size_t)lib.extra * 4, hipMemcpyDeviceToHost, f->stream) == hipSuccess);
        if (hipStreamSynchronize(f->stream) != hipSuccess || !ok) return hip_failed(f, "reading the plans back failed");
        launched.fetch_or(l.plans_bit);
        for (size_t m = 0; m < M; m++) {
            MapRun& mr = f->maps[m];
            if (mr.progress.length <= 0) continue;
            if (!host[M * (size_t)rows * A + m]) {
                report();
                return fail(LLE_ERR_HIP, "the parent links of map " + std::to_string(m) + " do not lead back to the reset state");
            }
            const uint8_t* first = host.data() + m * (size_t)rows * A;
            mr.plan.assign(first, first + (size_t)mr.progress.length * A);
            for (int w = 0; w < lib.extra; w++) mr.extra[w] = f->h_extra[(size_t)lib.extra * m + w];
        }
    }
    return report(), LLE_OK;
}

int plan(const Handle* f, int map_index, uint8_t* out, int64_t cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const MapRun& mr = f->maps[(size_t)map_index];
    if (mr.progress.length < 0) return fail(LLE_ERR_ARG, "the last run found no plan for this map");
    if (mr.progress.length > 0 && (!out || cap < (int64_t)mr.plan.size())) return fail(LLE_ERR_ARG, "the plan needs length * n_agents bytes");
    if (!mr.plan.empty()) std::memcpy(out, mr.plan.data(), mr.plan.size());
    return mr.progress.length;
}

int stats(const Handle* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const MapRun& mr = f->maps[(size_t)map_index];
    for (int d = 0; frontier && d < std::min(cap, (int)mr.frontier.size()); d++) frontier[d] = mr.frontier[(size_t)d];
    for (int d = 0; expanded && d < std::min(cap, (int)mr.expanded.size()); d++) expanded[d] = mr.expanded[(size_t)d];
    return (int)mr.frontier.size();
}

int occupancy(const Handle* f, int64_t* valid_items, int64_t* launched_lanes) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (valid_items) *valid_items = f->valid_items;
    if (launched_lanes) *launched_lanes = f->launched_lanes;
    return LLE_OK;
}

}  // namespace
}  // namespace lle_forest_core
#endif  // LLE_FOREST_CORE_HPP
