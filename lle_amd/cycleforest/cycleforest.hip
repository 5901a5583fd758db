// cycleforest.hip -- liblle_cycleforest.so: the solve mode no-interdependence-N (no closed trail of help events over exactly N distinct
// agents) for many equally shaped maps at once, one breadth-first tree per map, every tree walked depth by depth in the same launches
// (C ABI: include/lle_cycleforest.h; DESIGN.md "Cycle forest").
//
// The forest of ../forest/forest_core.hpp (kernel bodies, handle, create, level loop, plan read-back: shared with ../forest/forest.hip
// and ../helpforest/helpforest.hip) over the records of ../cycles/cycles.hip (cycle kind, ../cycles/cycles_logic.hpp: W more words, the
// packed set of (anchor, current, support) triples -- W = 3 for maps of up to 4 agents, 21 for 5 or 6; the maps of a batch agree on
// their agents, so one W holds for the forest).  Per map a segment of the pool (n_words + W arrays of `cap` words), parent, action, a
// table segment, eight counters -- and the map's OWN static data: its cell table (H * W words) and its edge rule, read from global
// memory by k / E, exactly as hf_insert reads them.
//
// cf_insert<W> works R' out in the lane's own slab of dynamic LDS: word i of the lane at i * 256 + threadIdx.x, indexed by the lane
// inside the WORKGROUP, not inside the map -- a workgroup straddles maps whenever E is no multiple of 256.  No cell table is staged, so
// there is no barrier and an idle lane returns at once.  Nothing is handed from lane to lane inside the launch: a lane's own value is
// in registers before the probe, and a tag it meets is worked out again in its own slab, from that candidate's parent in the map's own
// segment (sl::occupant_is): no lane waits, nothing needs a fence.
//
// Here are the kernels under their names, the C ABI with its argument checks and the judgement of the reset states with their values.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lle_cycleforest.h"
#include "../cycles/cycles_logic.hpp"
#include "../forest/forest_core.hpp"
#include "../helpforest/helpforest_logic.hpp"
#include "../search/search_core.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
namespace fl = lle_forest_logic;
namespace fc = lle_forest_core;
namespace hl = lle_helpgraph_logic;
namespace cl = lle_cycles_logic;
namespace hfl = lle_helpforest_logic;
using sd::fail;

namespace lle {

struct CfParams : fc::Params {
    const uint32_t* cells;       // [n_maps][H * W]: the sources that own a laser tile on the cell (bit laser_id), per map
    const hl::EdgeRule* rules;   // [n_maps]
    const uint32_t* root_extra;  // [n_maps][W]: the value words of every map's reset state in this run
    void* cand;                  // [n_lanes] CycleKind<W>::Value: the value of winner k, written by cf_insert for cf_commit
    uint32_t* goal_extra;        // [n_maps][W]: the value words of every solved map's goal record
    cl::Order order;             // N of the run
    int32_t H, W;
};

__device__ inline sc::Cells map_cells(const CfParams& p, int64_t map) { return sc::Cells{p.cells + (uint64_t)map * (uint64_t)p.H * (uint64_t)p.W}; }
// The kind a map searches with in this run: its own edge rule, the run's N, and the W words `work` (`stride` apart) its walk may write.
template <int W>
__device__ inline cl::CycleKind<W> map_kind(const CfParams& p, int64_t map, uint32_t* work, int32_t stride) {
    return cl::CycleKind<W>(cl::CycleRule{p.rules[map], p.order, work, stride});
}

__global__ __launch_bounds__(fc::THREADS) void cf_roots(CfParams p) { fc::roots(p); }
template <int W>
__global__ __launch_bounds__(fc::THREADS) void cf_seed(CfParams p) { fc::seed<cl::CycleKind<W>>(p, p.root_extra); }
__global__ __launch_bounds__(fc::THREADS) void cf_expand(CfParams p) { fc::expand(p); }

// Dynamic LDS: W * fc::THREADS words of slabs, word i of lane l at i * fc::THREADS + l.
template <int W>
__global__ __launch_bounds__(fc::THREADS) void cf_insert(CfParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t slabs[];
    const int64_t k = fc::lane();
    if (!fc::insert_front(p, k)) return;  // (no barrier in this kernel: an idle lane may leave)
    const int64_t map = k / p.E;
    fc::insert_back(p, map_kind<W>(p, map, slabs + threadIdx.x, fc::THREADS), map_cells(p, map), static_cast<typename cl::CycleKind<W>::Value*>(p.cand), k);
}

template <int W>
__global__ __launch_bounds__(fc::THREADS) void cf_commit(CfParams p) {
    const int64_t k = fc::lane();  // (the commit walks nothing: no work words)
    if (fc::is_winner(p, k)) fc::commit(p, map_kind<W>(p, k / p.E, nullptr, 0), static_cast<const typename cl::CycleKind<W>::Value*>(p.cand), k);
}

template <int W>
__global__ __launch_bounds__(fc::THREADS) void cf_plans(CfParams p) { fc::plans<cl::CycleKind<W>>(p, p.goal_extra); }

template __global__ void cf_seed<cl::SMALL_WORDS>(CfParams);
template __global__ void cf_insert<cl::SMALL_WORDS>(CfParams);
template __global__ void cf_commit<cl::SMALL_WORDS>(CfParams);
template __global__ void cf_plans<cl::SMALL_WORDS>(CfParams);
template __global__ void cf_seed<cl::LARGE_WORDS>(CfParams);
template __global__ void cf_insert<cl::LARGE_WORDS>(CfParams);
template __global__ void cf_commit<cl::LARGE_WORDS>(CfParams);
template __global__ void cf_plans<cl::LARGE_WORDS>(CfParams);

}  // namespace lle

// ================================================================================================ host side
using lle::CfParams;

namespace {

std::atomic<uint32_t> g_launched{0};
// (the four kernels of an agent class behind each other, the larger class behind the smaller)
enum { K_ROOTS = 0, K_EXPAND, K_SEED, K_INSERT, K_COMMIT, K_PLANS, K_CLASS = 4, K_COUNT = K_SEED + 2 * K_CLASS };
const char* const KERNEL_NAMES[K_COUNT] = {"cf_roots",      "cf_expand",    "cf_seed<3>",    "cf_insert<3>", "cf_commit<3>",
                                           "cf_plans<3>",   "cf_seed<21>",  "cf_insert<21>", "cf_commit<21>", "cf_plans<21>"};
const fc::Library LIBRARY[2] = {
    {"cf", "lle_cycleforest_options", "the cycle forest", "record", cl::SMALL_WORDS, LLE_CYCLES_CAPACITY, LLE_CYCLES_DENSE, sizeof(cl::CycleKind<cl::SMALL_WORDS>::Value)},
    {"cf", "lle_cycleforest_options", "the cycle forest", "record", cl::LARGE_WORDS, LLE_CYCLES_CAPACITY, LLE_CYCLES_DENSE, sizeof(cl::CycleKind<cl::LARGE_WORDS>::Value)}};

// The kernels of a run of the agent class whose values have W words; cf_insert<W> with its lanes' slabs.
template <int W>
fc::Launch<CfParams> launch_of() {
    constexpr int at = W == cl::SMALL_WORDS ? 0 : K_CLASS;
    return {lle::cf_seed<W>, lle::cf_expand, lle::cf_insert<W>, lle::cf_commit<W>, lle::cf_plans<W>, 1u << (K_SEED + at),
            1u << K_EXPAND | 1u << (K_INSERT + at) | 1u << (K_COMMIT + at), 1u << (K_PLANS + at), (size_t)W * fc::THREADS * 4};
}

static_assert(LLE_CYCLES_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_cycles.h and search_logic.hpp disagree");
static_assert(LLE_CYCLES_MAX_SOURCES == hl::MAX_SOURCES, "include/lle_cycles.h and helpgraph_logic.hpp disagree");
static_assert(LLE_CYCLES_MIN_ORDER == cl::MIN_ORDER && LLE_CYCLES_MAX_ORDER == cl::MAX_ORDER && LLE_CYCLES_WALK_BUDGET == cl::WALK_BUDGET,
              "include/lle_cycles.h and cycles_logic.hpp disagree");
static_assert(LLE_CYCLES_VALUE_WORDS == cl::LARGE_WORDS && LLE_CYCLES_VALUE_WORDS <= sl::MAX_EXTRA, "include/lle_cycles.h, cycles_logic.hpp and search_logic.hpp disagree");
static_assert((size_t)cl::LARGE_WORDS * fc::THREADS * 4 <= 65536, "the lanes' slabs fit 64 KB of LDS");

}  // namespace

struct lle_cycleforest : fc::Handle {
    std::vector<uint32_t> cells;      // [n_maps][H * W]: host copies of the static tables, for the reset states
    std::vector<hl::EdgeRule> rules;  // [n_maps]
    int words = 0;                    // of a value: the maps' agent class
    CfParams p{};
};

namespace {

template <int W>
int run(lle_cycleforest* f, const lle_cycleforest_args* args, const uint8_t* search, lle_cycleforest_result* per_map) {
    using Kind = cl::CycleKind<W>;
    CfParams p = f->p;
    fc::begin_run(f, &p, args->collect_gems != 0);
    p.order = cl::make_order(args->order_n);
    const sl::RecordLayout& r = p.lay;
    const size_t M = (size_t)f->n_maps, HW = (size_t)p.H * p.W;
    auto report = [&]() {
        for (size_t m = 0; m < M; m++) {
            const fl::MapProgress& pr = f->maps[m].progress;
            per_map[m].status = pr.status;
            per_map[m].length = pr.length;
            per_map[m].n_states = pr.n_states;
            per_map[m].depth_reached = pr.depth_reached;
            per_map[m].value_words = W;
        }
    };

    // ---- every reset state (t = 0: its edges count), judged on the host with the kernels' own functions
    for (size_t m = 0; m < M; m++) {
        fc::MapRun& mr = f->maps[m];
        uint32_t* extra = f->h_extra + (size_t)W * m;
        if (search && !search[m]) {  // not asked for: idle from the first level
            mr.frontier.clear();
            mr.progress = hfl::skipped_progress();
            continue;
        }
        const uint32_t* root = f->roots.data() + m * (size_t)r.n_words;
        const uint32_t* cells = f->cells.data() + m * HW;
        uint32_t work[W] = {};
        const Kind kind(cl::CycleRule{f->rules[m], p.order, work, 1});
        const uint64_t root_edges = kind.state([&](int w) { return root[w]; }, r, [&](int c) { return cells[c]; });
        typename Kind::Value root_value;
        const bool dense = !kind.update(cl::NoWords{}, root_edges, r.A, &root_value);
        const bool root_ok = !dense && !sl::anybody_dead(root[r.w_bits], r.A) && !kind.violates(root_value, r.A);  // a closed root: no plan starts here
        for (int i = 0; i < W; i++) extra[i] = root_ok ? root_value.w[i] : 0u;
        const bool solved = root_ok && sl::is_goal(root[r.w_bits], root[r.w_gems], r, p.collect_gems != 0u, p.G);
        mr.progress = fl::fresh_progress(root_ok && !solved);
        if (dense) mr.progress.status = LLE_CYCLES_DENSE;
        if (solved) {
            mr.progress.length = 0;
            for (int i = 0; i < W; i++) mr.extra[i] = extra[i];
        }
    }
    return fc::run(f, p, args->t_max, launch_of<W>(), LIBRARY[W == cl::SMALL_WORDS ? 0 : 1], g_launched, report);
}

}  // namespace

extern "C" {

const char* lle_cycleforest_last_error(void) { return sd::g_error.c_str(); }

void lle_cycleforest_free(lle_cycleforest* f) {
    if (!f) return;
    fc::close(f);
    delete f;
}

lle_cycleforest* lle_cycleforest_create(const lle_map* const* maps, int n_maps, const lle_cycleforest_options* opt) {
    fc::Options o;
    if (!fc::read_options(maps, n_maps, opt, LIBRARY[0], &o)) return nullptr;
    auto* f = new lle_cycleforest();
    f->words = cl::words_of(o.info.n_agents);
    f->rules.resize((size_t)n_maps);
    bool ok = true;
    for (int m = 0; ok && m < n_maps; m++) {
        std::string why;
        if (!sc::build_rule(maps[m], o.info, f->cells, f->rules[(size_t)m], why)) ok = (fail(LLE_ERR_UNSUPPORTED, why + " (map " + std::to_string(m) + ")"), false);
    }
    const fc::Table tables[2] = {{f->cells.data(), f->cells.size() * 4}, {f->rules.data(), f->rules.size() * sizeof(hl::EdgeRule)}};
    if (ok && fc::open(f, maps, n_maps, o, LIBRARY[f->words == cl::SMALL_WORDS ? 0 : 1], tables, &f->p, lle::cf_roots) == LLE_OK) {
        CfParams& p = f->p;
        p.cells = static_cast<const uint32_t*>(f->d_static[0]);
        p.rules = static_cast<const hl::EdgeRule*>(f->d_static[1]);
        p.root_extra = f->d_root_extra;
        p.cand = f->d_cand;
        p.goal_extra = f->d_goal_extra;
        p.H = o.info.height;
        p.W = o.info.width;
        g_launched.fetch_or(1u << K_ROOTS);
        return f;
    }
    delete f;
    return nullptr;
}

int lle_cycleforest_run(lle_cycleforest* f, const lle_cycleforest_args* args, const uint8_t* search, lle_cycleforest_result* per_map) {
    if (!args || !per_map) return fail(LLE_ERR_NULL, "NULL arguments or results");
    // (the arguments are judged before the handle is looked at: what they refuse they refuse on a machine without a device too)
    if (args->struct_bytes != sizeof(lle_cycleforest_args)) return fail(LLE_ERR_ARG, "lle_cycleforest_args.struct_bytes is not sizeof(lle_cycleforest_args)");
    if (args->order_n < cl::MIN_ORDER || args->order_n > cl::MAX_ORDER)
        return fail(LLE_ERR_ARG, "order_n must be 2 .. 6: a closed trail visits at least two agents, and a map has at most six");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (args->order_n > f->info.n_agents)
        return fail(LLE_ERR_ARG, "order_n = " + std::to_string(args->order_n) + " exceeds the maps' " + std::to_string(f->info.n_agents) +
                                     " agents: no closed trail of that order is possible, the plain forest of include/lle_forest.h is the answer");
    sd::DeviceGuard g(f->device);
    return f->words == cl::SMALL_WORDS ? run<cl::SMALL_WORDS>(f, args, search, per_map) : run<cl::LARGE_WORDS>(f, args, search, per_map);
}

int lle_cycleforest_plan(const lle_cycleforest* f, int map_index, uint8_t* out, int64_t cap) { return fc::plan(f, map_index, out, cap); }

int lle_cycleforest_value(const lle_cycleforest* f, int map_index, uint32_t* out) {
    if (!f) return fail(LLE_ERR_NULL, "NULL handle");
    if (!out) return fail(LLE_ERR_NULL, "NULL value words");
    if (map_index < 0 || map_index >= f->n_maps) return fail(LLE_ERR_ARG, "no such map");
    const fc::MapRun& mr = f->maps[(size_t)map_index];
    for (int i = 0; i < LLE_CYCLES_VALUE_WORDS; i++) out[i] = mr.progress.length >= 0 && i < f->words ? mr.extra[i] : 0u;
    return f->words;
}

int lle_cycleforest_stats(const lle_cycleforest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) {
    return fc::stats(f, map_index, frontier, expanded, cap);
}
int lle_cycleforest_occupancy(const lle_cycleforest* f, int64_t* valid_items, int64_t* launched_lanes) { return fc::occupancy(f, valid_items, launched_lanes); }
size_t lle_cycleforest_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, g_launched.load(), buf, cap); }
size_t lle_cycleforest_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, (1u << K_COUNT) - 1u, buf, cap); }

}  // extern "C"
