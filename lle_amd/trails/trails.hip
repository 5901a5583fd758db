// trails.hip -- liblle_trails.so: the exact shortest joint plan of a map that holds no sequence of N help events (no-sequence-N), by
// breadth-first search over (world state, trail lengths) through the step kernel of liblle_hip.so (C ABI: include/lle_trails.h;
// INTEGRATION.md section 18; DESIGN.md "Trail search").
//
// The single-tree search of ../search/search_core.hpp over the trail kind (trails_logic.hpp: TrailKind): ONE more word per record, the
// TRAIL VALUE of the trajectory that reached the state (4 bits per agent: the length of the longest trail of help edges that ends at
// the agent).  The trail word is part of a record's identity and lives only in the pool.  tr_insert works out
// L' = layer_update(L(parent), state_edges(successor)) in registers, counts the item in CNT_DENSE when the walk runs out of budget and
// drops it when some trail has N edges.  The pieces, the four launches and why nothing is handed from lane to lane inside the insert
// launch: search_core.hpp; the edge rule is ../helpgraph/helpgraph_logic.hpp's state_edges.  Here are the kernels under their names,
// the C ABI with its argument checks, the judgement of the reset state and the texts of a dense run.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lle_trails.h"
#include "../search/search_core.hpp"
#include "../search/search_device.hpp"
#include "../search/search_logic.hpp"
#include "trails_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;
using sd::fail;

namespace lle {

constexpr int TR_THREADS = 256;
static_assert(TR_THREADS == sc::THREADS, "search_core.hpp counts lanes in workgroups of sc::THREADS");
constexpr size_t LDS_TABLE_MAX_BYTES = 16384;  // H * W * 4 up to here: the cell table is staged in LDS, as hg_insert<true> does

struct TrParams : sc::Params {
    uint32_t* cand_trail;  // [chunk]: the trail value of winner k, written by tr_insert for tr_commit
    const uint32_t* cells; // [H * W]: the sources that own a laser tile on the cell (bit laser_id)
    tl::TrailKind kind;    // the map's edge rule; N of the run
};

__global__ __launch_bounds__(TR_THREADS) void tr_expand(TrParams p) { sc::expand(p); }

// LDS_TABLE: the cell table (H * W words <= LDS_TABLE_MAX_BYTES) staged in LDS; otherwise every read goes to global memory.
template <bool LDS_TABLE>
__global__ __launch_bounds__(TR_THREADS) void tr_insert(TrParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cells[];
    if constexpr (LDS_TABLE) {  // (every lane of the workgroup gets here: no exit before the barrier)
        const int HW = p.kind.rule.H * p.kind.rule.W;
        for (int c = threadIdx.x; c < HW; c += TR_THREADS) lds_cells[c] = p.cells[c];
        __syncthreads();
    }
    const uint32_t k = sc::lane();
    if (k >= p.n_items || !sc::insert_front(p, k)) return;
    if constexpr (LDS_TABLE) sc::insert_back(p, p.kind, sc::Cells{lds_cells}, p.cand_trail, k);
    else sc::insert_back(p, p.kind, sc::Cells{p.cells}, p.cand_trail, k);
}

__global__ __launch_bounds__(TR_THREADS) void tr_commit(TrParams p) { sc::commit(p, p.kind, p.cand_trail, sc::lane()); }

template __global__ void tr_insert<false>(TrParams);
template __global__ void tr_insert<true>(TrParams);

}  // namespace lle

// ================================================================================================ host side
namespace {

std::atomic<uint32_t> g_launched{0};
const char* const KERNEL_NAMES[4] = {"tr_expand", "tr_insert<false>", "tr_insert<true>", "tr_commit"};
// (one extra word, and one word per candidate: the pool is n_words + 1 arrays)
const sc::Library LIBRARY = {"tr", "lle_trails_options", "the trail search", "record", "trail word", tl::TrailKind::EXTRA, sizeof(tl::TrailKind::Value),
                            LLE_TRAILS_CAPACITY, LLE_TRAILS_DENSE};
static_assert(LLE_TRAILS_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_trails.h and search_logic.hpp disagree");
static_assert(LLE_TRAILS_MAX_SOURCES == hl::MAX_SOURCES, "include/lle_trails.h and helpgraph_logic.hpp disagree");
static_assert(LLE_TRAILS_MIN_LENGTH == tl::MIN_LENGTH && LLE_TRAILS_MAX_LENGTH == tl::MAX_LENGTH && LLE_TRAILS_WALK_BUDGET == tl::WALK_BUDGET,
              "include/lle_trails.h and trails_logic.hpp disagree");
static_assert(4 * LLE_TRAILS_MAX_AGENTS <= 31 && LLE_TRAILS_MAX_LENGTH - 1 <= 15, "a trail value is 4 bits per agent below the REACHED bit");

}  // namespace

struct lle_trails : sc::Handle {
    std::vector<uint32_t> cells;  // [H * W]: host copy of the cell table, for the reset state
    lle::TrParams p{};
};

extern "C" {

const char* lle_trails_last_error(void) { return sd::g_error.c_str(); }

void lle_trails_free(lle_trails* s) {
    if (!s) return;
    sc::close(s);
    delete s;
}

lle_trails* lle_trails_create(const lle_map* map, const lle_trails_options* opt) {
    sc::Options o;
    if (!sc::read_options(map, opt, LIBRARY, &o) || !sc::limits_ok(o.info, LIBRARY)) return nullptr;
    auto* s = new lle_trails();
    std::string why;
    if (!sc::build_rule(map, o.info, s->cells, s->p.kind.rule, why)) {
        fail(LLE_ERR_UNSUPPORTED, why);
    } else if (sc::open(s, map, o, LIBRARY, s->cells.data(), s->cells.size() * 4, &s->p) == LLE_OK) {
        s->p.cand_trail = static_cast<uint32_t*>(s->d_cand);
        s->p.cells = static_cast<const uint32_t*>(s->d_static);
        return s;
    }
    delete s;
    return nullptr;
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
    sd::DeviceGuard g(s->device);
    lle::TrParams p = s->p;
    sc::begin_run(s, &p, args->collect_gems != 0);
    p.kind.N = args->length_n;
    const sl::RecordLayout& r = p.lay;
    sc::Outcome out;
    auto report = [&](int rc) {
        result->length = out.length;
        result->n_states = out.n_states;
        result->depth_reached = out.depth_reached;
        result->trail = out.length >= 0 ? out.goal_extra[0] : 0u;
        result->step_errors = out.step_errors;
        return rc;
    };

    // ---- the reset state (t = 0: its edges count), judged on the host with the kernels' own functions
    const std::vector<uint32_t>& root = s->root;
    const uint64_t root_edges = p.kind.state([&](int w) { return root[(size_t)w]; }, r, [&](int c) { return s->cells[(size_t)c]; });
    int budget = tl::WALK_BUDGET;
    const uint32_t root_trail = tl::layer_update(0u, root_edges, p.kind.N, r.A, budget);
    if (budget < 0)
        return report(fail(LLE_TRAILS_DENSE, "the arcs of the reset state allow more than " + std::to_string(tl::WALK_BUDGET) + " trail extensions: the search has no answer"));
    if (sl::anybody_dead(root[(size_t)r.w_bits], r.A) || p.kind.violates(root_trail, r.A)) return report(LLE_OK);  // no plan starts here
    if (sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, p.collect_gems != 0u, p.G)) {
        s->length = out.length = 0;
        out.goal_extra[0] = root_trail;
        return report(LLE_OK);
    }
    const size_t table_bytes = s->cells.size() * 4;
    const bool in_lds = table_bytes <= lle::LDS_TABLE_MAX_BYTES;
    const sc::Launch<lle::TrParams> launch = {lle::tr_expand, in_lds ? lle::tr_insert<true> : lle::tr_insert<false>, lle::tr_commit, in_lds ? (table_bytes + 15) / 16 * 16 : 0, in_lds};
    const int rc = sc::search_tree(s, p, args->t_max, &root_trail, launch, LIBRARY, g_launched, &out);
    if (rc == LLE_TRAILS_DENSE)  // (n_states = 1: no answer, never a partial one)
        return report(fail(rc, "the arcs of one state allow more than " + std::to_string(tl::WALK_BUDGET) + " trail extensions (" + std::to_string(out.dense) + " work items at depth " +
                                   std::to_string(out.depth_reached) + "): the search has no answer"));
    return report(rc);
}

int lle_trails_plan(const lle_trails* s, uint8_t* out, int64_t cap) { return sc::plan(s, out, cap); }
int lle_trails_stats(const lle_trails* s, int64_t* frontier, int64_t* expanded, int cap) { return sc::stats(s, frontier, expanded, cap); }
size_t lle_trails_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, g_launched.load(), buf, cap); }
size_t lle_trails_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, 0xFu, buf, cap); }

}  // extern "C"
