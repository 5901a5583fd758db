// helpgraph.hip -- liblle_helpgraph.so: the exact shortest joint plan of a map under a restriction on who may help whom, by breadth-first
// search over (world state, help relation) through the step kernel of liblle_hip.so (C ABI: include/lle_helpgraph.h; INTEGRATION.md
// section 17; DESIGN.md "Help-graph search").
//
// The single-tree search of ../search/search_core.hpp over the help kind (helpgraph_logic.hpp: HelpKind): two more words per record,
// the HELP VALUE of the trajectory that reached the state (48 bits: bit 8 h + b = h has helped b in some state so far, the reset state
// included).  The help words are part of a record's identity and live only in the pool.  hg_insert works out
// help' = help(parent) | state_edges(successor) in registers and drops the item when the mode rejects help'; hg_commit reports a goal the
// mode accepts.  The pieces, the four launches and why nothing is handed from lane to lane inside the insert launch: search_core.hpp.
// Here are the kernels under their names, the C ABI with its argument checks, and the judgement of the reset state.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lle_helpgraph.h"
#include "../search/search_core.hpp"
#include "../search/search_device.hpp"
#include "../search/search_logic.hpp"
#include "helpgraph_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
namespace hl = lle_helpgraph_logic;
using sd::fail;

namespace lle {

constexpr int HG_THREADS = 256;
static_assert(HG_THREADS == sc::THREADS, "search_core.hpp counts lanes in workgroups of sc::THREADS");
constexpr size_t LDS_TABLE_MAX_BYTES = 16384;  // H * W * 4 up to here: the cell table is staged in LDS, as the coop kernel does

struct HgParams : sc::Params {
    uint64_t* cand_help;   // [chunk]: the help value of winner k, written by hg_insert for hg_commit
    const uint32_t* cells; // [H * W]: the sources that own a laser tile on the cell (bit laser_id)
    hl::HelpKind kind;     // the map's edge rule; mode and param of the run
};

__global__ __launch_bounds__(HG_THREADS) void hg_expand(HgParams p) { sc::expand(p); }

// LDS_TABLE: the cell table (H * W words <= LDS_TABLE_MAX_BYTES) staged in LDS; otherwise every read goes to global memory.
template <bool LDS_TABLE>
__global__ __launch_bounds__(HG_THREADS) void hg_insert(HgParams p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cells[];
    if constexpr (LDS_TABLE) {  // (every lane of the workgroup gets here: no exit before the barrier)
        const int HW = p.kind.rule.H * p.kind.rule.W;
        for (int c = threadIdx.x; c < HW; c += HG_THREADS) lds_cells[c] = p.cells[c];
        __syncthreads();
    }
    const uint32_t k = sc::lane();
    if (k >= p.n_items || !sc::insert_front(p, k)) return;
    if constexpr (LDS_TABLE) sc::insert_back(p, p.kind, sc::Cells{lds_cells}, p.cand_help, k);
    else sc::insert_back(p, p.kind, sc::Cells{p.cells}, p.cand_help, k);
}

__global__ __launch_bounds__(HG_THREADS) void hg_commit(HgParams p) { sc::commit(p, p.kind, p.cand_help, sc::lane()); }

template __global__ void hg_insert<false>(HgParams);
template __global__ void hg_insert<true>(HgParams);

}  // namespace lle

// ================================================================================================ host side
namespace {

std::atomic<uint32_t> g_launched{0};
const char* const KERNEL_NAMES[4] = {"hg_expand", "hg_insert<false>", "hg_insert<true>", "hg_commit"};
const sc::Library LIBRARY = {"hg", "lle_helpgraph_options", "the help-graph search", "record", "help words", hl::HelpKind::EXTRA, sizeof(hl::HelpKind::Value),
                            LLE_HELPGRAPH_CAPACITY, 0};
static_assert(LLE_HELPGRAPH_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_helpgraph.h and search_logic.hpp disagree");
static_assert(LLE_HELPGRAPH_MAX_SOURCES == hl::MAX_SOURCES, "include/lle_helpgraph.h and helpgraph_logic.hpp disagree");
static_assert(LLE_HELPGRAPH_STANDARD == hl::STANDARD && LLE_HELPGRAPH_NO_ASYMMETRIC == hl::NO_ASYMMETRIC && LLE_HELPGRAPH_NO_MUTUAL == hl::NO_MUTUAL &&
                  LLE_HELPGRAPH_NO_FULLY_COUPLED == hl::NO_FULLY_COUPLED && LLE_HELPGRAPH_NO_CONVERGENCE == hl::NO_CONVERGENCE &&
                  LLE_HELPGRAPH_NO_DIVERGENCE == hl::NO_DIVERGENCE,
              "include/lle_helpgraph.h and helpgraph_logic.hpp disagree");

}  // namespace

struct lle_helpgraph : sc::Handle {
    std::vector<uint32_t> cells;  // [H * W]: host copy of the cell table, for the reset state
    lle::HgParams p{};
};

extern "C" {

const char* lle_helpgraph_last_error(void) { return sd::g_error.c_str(); }

void lle_helpgraph_free(lle_helpgraph* s) {
    if (!s) return;
    sc::close(s);
    delete s;
}

lle_helpgraph* lle_helpgraph_create(const lle_map* map, const lle_helpgraph_options* opt) {
    sc::Options o;
    if (!sc::read_options(map, opt, LIBRARY, &o) || !sc::limits_ok(o.info, LIBRARY)) return nullptr;
    auto* s = new lle_helpgraph();
    std::string why;
    if (!sc::build_rule(map, o.info, s->cells, s->p.kind.rule, why)) {
        fail(LLE_ERR_UNSUPPORTED, why);
    } else if (sc::open(s, map, o, LIBRARY, s->cells.data(), s->cells.size() * 4, &s->p) == LLE_OK) {
        s->p.cand_help = static_cast<uint64_t*>(s->d_cand);
        s->p.cells = static_cast<const uint32_t*>(s->d_static);
        return s;
    }
    delete s;
    return nullptr;
}

int lle_helpgraph_run(lle_helpgraph* s, const lle_helpgraph_args* args, lle_helpgraph_result* result) {
    if (!s || !args || !result) return fail(LLE_ERR_NULL, "NULL handle, arguments or result");
    if (args->struct_bytes != sizeof(lle_helpgraph_args)) return fail(LLE_ERR_ARG, "lle_helpgraph_args.struct_bytes is not sizeof(lle_helpgraph_args)");
    if (result->struct_bytes != sizeof(lle_helpgraph_result)) return fail(LLE_ERR_ARG, "lle_helpgraph_result.struct_bytes is not sizeof(lle_helpgraph_result)");
    if (args->mode < 0 || args->mode >= hl::N_MODES) return fail(LLE_ERR_ARG, "unknown mode");
    if ((args->mode == LLE_HELPGRAPH_NO_CONVERGENCE || args->mode == LLE_HELPGRAPH_NO_DIVERGENCE) && args->param < 2)
        return fail(LLE_ERR_ARG, "param must be at least 2: a convergence or divergence has at least two helpers or beneficiaries");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    sd::DeviceGuard g(s->device);
    lle::HgParams p = s->p;
    sc::begin_run(s, &p, args->collect_gems != 0);
    p.kind.mode = args->mode;
    p.kind.param = args->param;
    const sl::RecordLayout& r = p.lay;
    sc::Outcome out;
    auto report = [&](int rc) {
        result->length = out.length;
        result->n_states = out.n_states;
        result->depth_reached = out.depth_reached;
        result->pad = 0;
        result->step_errors = out.step_errors;
        result->help_lo = out.length >= 0 ? out.goal_extra[0] : 0u;
        result->help_hi = out.length >= 0 ? out.goal_extra[1] : 0u;
        return rc;
    };

    // ---- the reset state, judged on the host with the kernels' own functions
    const std::vector<uint32_t>& root = s->root;
    const uint64_t root_help = p.kind.state([&](int w) { return root[(size_t)w]; }, r, [&](int c) { return s->cells[(size_t)c]; });
    const sl::ExtraWords<2> root_words = p.kind.words(root_help);
    if (sl::anybody_dead(root[(size_t)r.w_bits], r.A) || p.kind.violates(root_help, r.A)) return report(LLE_OK);  // no plan starts here
    if (sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, p.collect_gems != 0u, p.G) && p.kind.accepts(root_help, r.A)) {
        s->length = out.length = 0;
        out.goal_extra[0] = root_words.w[0];
        out.goal_extra[1] = root_words.w[1];
        return report(LLE_OK);
    }
    const size_t table_bytes = s->cells.size() * 4;
    const bool in_lds = table_bytes <= lle::LDS_TABLE_MAX_BYTES;
    const sc::Launch<lle::HgParams> launch = {lle::hg_expand, in_lds ? lle::hg_insert<true> : lle::hg_insert<false>, lle::hg_commit, in_lds ? (table_bytes + 15) / 16 * 16 : 0, in_lds};
    return report(sc::search_tree(s, p, args->t_max, root_words.w, launch, LIBRARY, g_launched, &out));
}

int lle_helpgraph_plan(const lle_helpgraph* s, uint8_t* out, int64_t cap) { return sc::plan(s, out, cap); }
int lle_helpgraph_stats(const lle_helpgraph* s, int64_t* frontier, int64_t* expanded, int cap) { return sc::stats(s, frontier, expanded, cap); }
size_t lle_helpgraph_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, g_launched.load(), buf, cap); }
size_t lle_helpgraph_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, 0xFu, buf, cap); }

}  // extern "C"
