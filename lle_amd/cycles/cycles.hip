// cycles.hip -- liblle_cycles.so: the exact shortest joint plan of a map that holds no closed trail of help events over exactly N
// distinct agents (no-interdependence-N), by breadth-first search over (world state, trail triples) through the step kernel of
// liblle_hip.so (C ABI: include/lle_cycles.h; DESIGN.md "Closed-trail search").
//
// The single-tree search of ../search/search_core.hpp over the cycle kind (cycles_logic.hpp: CycleKind<W>): W more words per record,
// the packed set R of (anchor, current, support) triples of the trajectory that reached the state -- W = 3 for maps of up to 4
// agents, 21 for 5 or 6.  The words are part of a record's identity and live only in the pool.  cy_insert works out
// R' = layer_update(R(parent), state_edges(successor)) with the accumulating R' in the lane's own slab of LDS (word i of lane l at
// i * 256 + l: indexed by (anchor, current) at run time, which registers cannot be), counts the item in CNT_DENSE when the walk runs
// out of budget and drops it when a closed trail of order N appears.  The pieces, the four launches and why nothing is handed from
// lane to lane inside the insert launch: search_core.hpp -- a lane that meets another candidate's tag works that candidate's R' out
// again in its own slab, after its own has gone to registers.  Here are the kernels under their names, the C ABI with its argument
// checks, the judgement of the reset state and the texts of a dense run.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lle_cycles.h"
#include "../search/search_core.hpp"
#include "../search/search_device.hpp"
#include "../search/search_logic.hpp"
#include "cycles_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
namespace hl = lle_helpgraph_logic;
namespace cl = lle_cycles_logic;
using sd::fail;

namespace lle {

constexpr int CY_THREADS = 256;
static_assert(CY_THREADS == sc::THREADS, "search_core.hpp counts lanes in workgroups of sc::THREADS");
// H * W * 4 up to here: the cell table is staged in LDS, as tr_insert<true> does.  Half as much beside the 21.5 KB of slabs of the larger
// agent class -- whose maps the step kernel's own tables keep below 16 KB of cells anyway, so that a limit of 16 KB would never be passed.
constexpr size_t LDS_TABLE_MAX_BYTES = 16384, LDS_TABLE_MAX_BYTES_LARGE = 8192;
static_assert(LDS_TABLE_MAX_BYTES + (size_t)cl::LARGE_WORDS * CY_THREADS * 4 <= 65536, "the staged table and the lanes' slabs fit 64 KB of LDS");

struct CyParams : sc::Params {
    void* cand;             // [chunk] CycleKind<W>::Value: the value of winner k, written by cy_insert for cy_commit
    const uint32_t* cells;  // [H * W]: the sources that own a laser tile on the cell (bit laser_id)
    cl::CycleRule kind;     // the map's edge rule; N of the run (`work` is every lane's own: set in the kernel)
    uint32_t slab_at;       // the word of the dynamic LDS at which the lanes' slabs begin: behind the staged cell table
};

__global__ __launch_bounds__(CY_THREADS) void cy_expand(CyParams p) { sc::expand(p); }

// LDS_TABLE: the cell table (H * W words <= LDS_TABLE_MAX_BYTES, _LARGE for W = 21) staged in LDS; otherwise every read goes to global memory.
// Dynamic LDS: [0, slab_at) the table, then W * CY_THREADS words of slabs.
template <bool LDS_TABLE, int W>
__global__ __launch_bounds__(CY_THREADS) void cy_insert(CyParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_words[];
    if constexpr (LDS_TABLE) {  // (every lane of the workgroup gets here: no exit before the barrier)
        const int HW = p.kind.rule.H * p.kind.rule.W;
        for (int c = threadIdx.x; c < HW; c += CY_THREADS) lds_words[c] = p.cells[c];
        __syncthreads();
    }
    const uint32_t k = sc::lane();
    if (k >= p.n_items || !sc::insert_front(p, k)) return;
    cl::CycleRule mine = p.kind;
    mine.work = lds_words + p.slab_at + threadIdx.x;  // words slab_at + i * CY_THREADS + lane, i < W: inside the launch's LDS
    mine.work_stride = CY_THREADS;
    const cl::CycleKind<W> kind(mine);
    auto* cand = static_cast<typename cl::CycleKind<W>::Value*>(p.cand);
    if constexpr (LDS_TABLE) sc::insert_back(p, kind, sc::Cells{lds_words}, cand, k);
    else sc::insert_back(p, kind, sc::Cells{p.cells}, cand, k);
}

template <int W>
__global__ __launch_bounds__(CY_THREADS) void cy_commit(CyParams p) {
    sc::commit(p, cl::CycleKind<W>(p.kind), static_cast<const typename cl::CycleKind<W>::Value*>(p.cand), sc::lane());
}

template __global__ void cy_insert<false, cl::SMALL_WORDS>(CyParams);
template __global__ void cy_insert<true, cl::SMALL_WORDS>(CyParams);
template __global__ void cy_commit<cl::SMALL_WORDS>(CyParams);
template __global__ void cy_insert<false, cl::LARGE_WORDS>(CyParams);
template __global__ void cy_insert<true, cl::LARGE_WORDS>(CyParams);
template __global__ void cy_commit<cl::LARGE_WORDS>(CyParams);

}  // namespace lle

// ================================================================================================ host side
namespace {

// (per agent class the four bits search_core.hpp's launch_piece sets: expand, insert<false>, insert<true>, commit)
std::atomic<uint32_t> g_launched[2];
const char* const KERNEL_NAMES[2][4] = {{"cy_expand", "cy_insert<false, 3>", "cy_insert<true, 3>", "cy_commit<3>"},
                                        {"cy_expand", "cy_insert<false, 21>", "cy_insert<true, 21>", "cy_commit<21>"}};
const sc::Library LIBRARY[2] = {
    {"cy", "lle_cycles_options", "the closed-trail search", "record", "value words", cl::SMALL_WORDS, sizeof(cl::CycleKind<cl::SMALL_WORDS>::Value), LLE_CYCLES_CAPACITY, LLE_CYCLES_DENSE},
    {"cy", "lle_cycles_options", "the closed-trail search", "record", "value words", cl::LARGE_WORDS, sizeof(cl::CycleKind<cl::LARGE_WORDS>::Value), LLE_CYCLES_CAPACITY, LLE_CYCLES_DENSE}};
static_assert(LLE_CYCLES_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_cycles.h and search_logic.hpp disagree");
static_assert(LLE_CYCLES_MAX_SOURCES == hl::MAX_SOURCES, "include/lle_cycles.h and helpgraph_logic.hpp disagree");
static_assert(LLE_CYCLES_MIN_ORDER == cl::MIN_ORDER && LLE_CYCLES_MAX_ORDER == cl::MAX_ORDER && LLE_CYCLES_WALK_BUDGET == cl::WALK_BUDGET,
              "include/lle_cycles.h and cycles_logic.hpp disagree");
static_assert(LLE_CYCLES_VALUE_WORDS == cl::LARGE_WORDS && LLE_CYCLES_VALUE_WORDS <= sl::MAX_EXTRA && LLE_CYCLES_MAX_ORDER <= LLE_CYCLES_MAX_AGENTS,
              "include/lle_cycles.h, cycles_logic.hpp and search_logic.hpp disagree");
static_assert(sizeof(((lle_cycles_result*)nullptr)->value) == 4 * LLE_CYCLES_VALUE_WORDS, "lle_cycles_result.value holds the larger class");

size_t names(uint32_t small_bits, uint32_t large_bits, char* buf, size_t cap) {
    const char* list[7];
    int n = 0;
    for (int k = 0; k < 4; k++)
        if ((small_bits >> k) & 1u) list[n++] = KERNEL_NAMES[0][k];
    for (int k = 0; k < 4; k++)  // (cy_expand is one kernel: named once)
        if (((large_bits >> k) & 1u) && !(k == 0 && (small_bits & 1u))) list[n++] = KERNEL_NAMES[1][k];
    return sd::names_out(list, n, (1u << n) - 1u, buf, cap);
}

}  // namespace

struct lle_cycles : sc::Handle {
    std::vector<uint32_t> cells;  // [H * W]: host copy of the cell table, for the reset state
    int words = 0;                // of a value: the map's agent class
    lle::CyParams p{};
};

namespace {

template <int W>
int run(lle_cycles* s, const lle_cycles_args* args, lle_cycles_result* result) {
    using Kind = cl::CycleKind<W>;
    constexpr int cls = W == cl::SMALL_WORDS ? 0 : 1;
    lle::CyParams p = s->p;
    sc::begin_run(s, &p, args->collect_gems != 0);
    p.kind.order = cl::make_order(args->order_n);
    const sl::RecordLayout& r = p.lay;
    sc::Outcome out;
    auto report = [&](int rc) {
        result->length = out.length;
        result->n_states = out.n_states;
        result->depth_reached = out.depth_reached;
        result->value_words = W;
        for (int i = 0; i < LLE_CYCLES_VALUE_WORDS; i++) result->value[i] = out.length >= 0 && i < W ? out.goal_extra[i] : 0u;
        result->step_errors = out.step_errors;
        return rc;
    };

    // ---- the reset state (t = 0: its edges count), judged on the host with the kernels' own functions
    uint32_t work[W] = {};
    cl::CycleRule mine = p.kind;
    mine.work = work;
    mine.work_stride = 1;
    const Kind kind(mine);
    const std::vector<uint32_t>& root = s->root;
    const uint64_t root_edges = kind.state([&](int w) { return root[(size_t)w]; }, r, [&](int c) { return s->cells[(size_t)c]; });
    typename Kind::Value root_value;
    if (!kind.update(cl::NoWords{}, root_edges, r.A, &root_value))
        return report(fail(LLE_CYCLES_DENSE, "the arcs of the reset state allow more than " + std::to_string(cl::WALK_BUDGET) + " trail extensions: the search has no answer"));
    if (sl::anybody_dead(root[(size_t)r.w_bits], r.A) || kind.violates(root_value, r.A)) return report(LLE_OK);  // no plan starts here
    if (sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, p.collect_gems != 0u, p.G)) {
        s->length = out.length = 0;
        for (int i = 0; i < W; i++) out.goal_extra[i] = root_value.w[i];
        return report(LLE_OK);
    }
    const size_t table_bytes = s->cells.size() * 4, slab_bytes = (size_t)W * lle::CY_THREADS * 4;
    const bool in_lds = table_bytes <= (W == cl::SMALL_WORDS ? lle::LDS_TABLE_MAX_BYTES : lle::LDS_TABLE_MAX_BYTES_LARGE);
    const size_t staged_bytes = in_lds ? (table_bytes + 15) / 16 * 16 : 0;
    p.slab_at = (uint32_t)(staged_bytes / 4);
    const sc::Launch<lle::CyParams> launch = {lle::cy_expand, in_lds ? lle::cy_insert<true, W> : lle::cy_insert<false, W>, lle::cy_commit<W>, staged_bytes + slab_bytes, in_lds};
    const int rc = sc::search_tree(s, p, args->t_max, root_value.w, launch, LIBRARY[cls], g_launched[cls], &out);
    if (rc == LLE_CYCLES_DENSE)  // (n_states = 1: no answer, never a partial one)
        return report(fail(rc, "the arcs of one state allow more than " + std::to_string(cl::WALK_BUDGET) + " trail extensions (" + std::to_string(out.dense) + " work items at depth " +
                                   std::to_string(out.depth_reached) + "): the search has no answer"));
    return report(rc);
}

}  // namespace

extern "C" {

const char* lle_cycles_last_error(void) { return sd::g_error.c_str(); }

void lle_cycles_free(lle_cycles* s) {
    if (!s) return;
    sc::close(s);
    delete s;
}

lle_cycles* lle_cycles_create(const lle_map* map, const lle_cycles_options* opt) {
    sc::Options o;
    if (!sc::read_options(map, opt, LIBRARY[0], &o) || !sc::limits_ok(o.info, LIBRARY[0])) return nullptr;
    auto* s = new lle_cycles();
    s->words = cl::words_of(o.info.n_agents);
    std::string why;
    if (!sc::build_rule(map, o.info, s->cells, s->p.kind.rule, why)) {
        fail(LLE_ERR_UNSUPPORTED, why);
    } else if (sc::open(s, map, o, LIBRARY[s->words == cl::SMALL_WORDS ? 0 : 1], s->cells.data(), s->cells.size() * 4, &s->p) == LLE_OK) {
        s->p.cand = s->d_cand;
        s->p.cells = static_cast<const uint32_t*>(s->d_static);
        return s;
    }
    delete s;
    return nullptr;
}

int lle_cycles_run(lle_cycles* s, const lle_cycles_args* args, lle_cycles_result* result) {
    if (!args || !result) return fail(LLE_ERR_NULL, "NULL arguments or result");
    // (the arguments are judged before the handle is looked at: what they refuse they refuse on a machine without a device too)
    if (args->struct_bytes != sizeof(lle_cycles_args)) return fail(LLE_ERR_ARG, "lle_cycles_args.struct_bytes is not sizeof(lle_cycles_args)");
    if (result->struct_bytes != sizeof(lle_cycles_result)) return fail(LLE_ERR_ARG, "lle_cycles_result.struct_bytes is not sizeof(lle_cycles_result)");
    if (args->order_n < cl::MIN_ORDER || args->order_n > cl::MAX_ORDER)
        return fail(LLE_ERR_ARG, "order_n must be 2 .. 6: a closed trail visits at least two agents, and a map has at most six");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    if (!s) return fail(LLE_ERR_NULL, "NULL handle");
    if (args->order_n > s->info.n_agents)
        return fail(LLE_ERR_ARG, "order_n = " + std::to_string(args->order_n) + " exceeds the map's " + std::to_string(s->info.n_agents) +
                                     " agents: no closed trail of that order is possible, the plain search of include/lle_search.h is the answer");
    sd::DeviceGuard g(s->device);
    return s->words == cl::SMALL_WORDS ? run<cl::SMALL_WORDS>(s, args, result) : run<cl::LARGE_WORDS>(s, args, result);
}

int lle_cycles_plan(const lle_cycles* s, uint8_t* out, int64_t cap) { return sc::plan(s, out, cap); }
int lle_cycles_stats(const lle_cycles* s, int64_t* frontier, int64_t* expanded, int cap) { return sc::stats(s, frontier, expanded, cap); }
size_t lle_cycles_debug_launched(char* buf, size_t cap) { return names(g_launched[0].load(), g_launched[1].load(), buf, cap); }
size_t lle_cycles_debug_compiled(char* buf, size_t cap) { return names(0xFu, 0xFu, buf, cap); }

}  // extern "C"
