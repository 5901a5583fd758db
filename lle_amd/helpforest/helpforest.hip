// helpforest.hip -- liblle_helpforest.so: the solve modes over the help graph and no-sequence-N for many equally shaped maps at once, one
// breadth-first tree per map, every tree walked depth by depth in the same launches (C ABI: include/lle_helpforest.h; INTEGRATION.md
// section 19; DESIGN.md "Help forest").
//
// The forest of ../forest/forest_core.hpp (kernel bodies, handle, create, level loop, plan read-back: shared with ../forest/forest.hip)
// over the records of ../helpgraph/helpgraph.hip (help kind: two more words, the help value) or of ../trails/trails.hip (trail kind:
// one more word, the trail value).  Per map a segment of the pool (n_words + 2 arrays of `cap` words, whichever kind runs), parent,
// action, a table segment, eight counters -- and the map's OWN static data: its cell table (H * W words) and its edge rule.  Lanes,
// segments and the fates of a map are ../forest/forest_logic.hpp's, the edge rule and the modes ../helpgraph/helpgraph_logic.hpp's,
// the walk ../trails/trails_logic.hpp's.  Both kinds (hl::HelpKind, tl::TrailKind) run through the same code of
// ../search/search_logic.hpp: a LOCAL tag (TAG_BIT | index inside the map's block) is taken apart by sl::Piece, sl::occupant_is compares.
//
// Here are the kernels under their names, which make the kind of a lane's map from the map's own rule and read its own cell table from
// memory (a workgroup spans several maps when E is no multiple of 256; a table is H * W words that every lane of the map reads: it
// stays in cache), the C ABI with its argument checks and the judgement of the reset states with their extra words.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/lle_helpforest.h"
#include "../forest/forest_core.hpp"
#include "../search/search_core.hpp"
#include "helpforest_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
namespace fl = lle_forest_logic;
namespace fc = lle_forest_core;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;
namespace hfl = lle_helpforest_logic;
using sd::fail;

namespace lle {

template <int KIND>
using KindOf = std::conditional_t<KIND == hfl::KIND_HELP, hl::HelpKind, tl::TrailKind>;

struct HfParams : fc::Params {
    const uint32_t* cells;       // [n_maps][H * W]: the sources that own a laser tile on the cell (bit laser_id), per map
    const hl::EdgeRule* rules;   // [n_maps]
    const uint32_t* root_extra;  // [n_maps][2]: the extra words of every map's reset state in this run
    void* cand_extra;            // [n_lanes] of 8 bytes: the value of winner k as its kind keeps it, for hf_commit
    uint32_t* goal_extra;        // [n_maps][2]: the extra words of every solved map's goal record
    int32_t H, W;
    int32_t mode, param;
};

__device__ inline sc::Cells map_cells(const HfParams& p, int64_t map) { return sc::Cells{p.cells + (uint64_t)map * (uint64_t)p.H * (uint64_t)p.W}; }
// The kind a map searches with in this run: its own edge rule, the run's mode and param (k of a help mode, or N).
template <int KIND>
__device__ inline KindOf<KIND> map_kind(const HfParams& p, int64_t map) {
    if constexpr (KIND == hfl::KIND_HELP) return hl::HelpKind{p.rules[map], p.mode, p.param};
    else return tl::TrailKind{p.rules[map], p.param};
}

__global__ __launch_bounds__(fc::THREADS) void hf_roots(HfParams p) { fc::roots(p); }
template <int KIND>
__global__ __launch_bounds__(fc::THREADS) void hf_seed(HfParams p) { fc::seed<KindOf<KIND>>(p, p.root_extra); }
__global__ __launch_bounds__(fc::THREADS) void hf_expand(HfParams p) { fc::expand(p); }

template <int KIND>
__global__ __launch_bounds__(fc::THREADS) void hf_insert(HfParams p) {
    const int64_t k = fc::lane();
    if (fc::insert_front(p, k)) fc::insert_back(p, map_kind<KIND>(p, k / p.E), map_cells(p, k / p.E), static_cast<typename KindOf<KIND>::Value*>(p.cand_extra), k);
}

template <int KIND>
__global__ __launch_bounds__(fc::THREADS) void hf_commit(HfParams p) {
    const int64_t k = fc::lane();
    if (fc::is_winner(p, k)) fc::commit(p, map_kind<KIND>(p, k / p.E), static_cast<const typename KindOf<KIND>::Value*>(p.cand_extra), k);
}

// (both words of a segment's extra arrays, whichever kind ran: the host knows which of them the kind has)
__global__ __launch_bounds__(fc::THREADS) void hf_plans(HfParams p) { fc::plans<hl::HelpKind>(p, p.goal_extra); }

template __global__ void hf_seed<hfl::KIND_HELP>(HfParams);
template __global__ void hf_seed<hfl::KIND_TRAIL>(HfParams);
template __global__ void hf_insert<hfl::KIND_HELP>(HfParams);
template __global__ void hf_insert<hfl::KIND_TRAIL>(HfParams);
template __global__ void hf_commit<hfl::KIND_HELP>(HfParams);
template __global__ void hf_commit<hfl::KIND_TRAIL>(HfParams);

}  // namespace lle

// ================================================================================================ host side
using lle::HfParams;

namespace {

std::atomic<uint32_t> g_launched{0};
enum { K_ROOTS = 0, K_SEED_HELP, K_SEED_TRAIL, K_EXPAND, K_INSERT_HELP, K_INSERT_TRAIL, K_COMMIT_HELP, K_COMMIT_TRAIL, K_PLANS, K_COUNT };
const char* const KERNEL_NAMES[K_COUNT] = {"hf_roots",         "hf_seed<help>",   "hf_seed<trail>",   "hf_expand", "hf_insert<help>",
                                           "hf_insert<trail>", "hf_commit<help>", "hf_commit<trail>", "hf_plans"};
const fc::Library LIBRARY = {"hf", "lle_helpforest_options", "the help forest", "record", hfl::EXTRA_WORDS, LLE_HELPGRAPH_CAPACITY, LLE_TRAILS_DENSE,
                             sizeof(hl::HelpKind::Value)};

// The kernels of a run of kind KIND (in the name table a trail kernel follows its help twin).
template <int KIND>
fc::Launch<HfParams> launch_of() {
    return {lle::hf_seed<KIND>, lle::hf_expand, lle::hf_insert<KIND>, lle::hf_commit<KIND>, lle::hf_plans, 1u << (K_SEED_HELP + KIND),
            1u << K_EXPAND | 1u << (K_INSERT_HELP + KIND) | 1u << (K_COMMIT_HELP + KIND), 1u << K_PLANS};
}

static_assert(hfl::KIND_HELP == 0 && hfl::KIND_TRAIL == 1 && hl::HelpKind::EXTRA == hfl::EXTRA_WORDS && tl::TrailKind::EXTRA <= hfl::EXTRA_WORDS &&
                  sizeof(tl::TrailKind::Value) <= sizeof(hl::HelpKind::Value),
              "launch_of counts kinds from help = 0; hf_plans fetches a segment's extra arrays as the help kind's words");
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

}  // namespace

struct lle_helpforest : fc::Handle {
    std::vector<uint32_t> cells;      // [n_maps][H * W]: host copies of the static tables, for the reset states
    std::vector<hl::EdgeRule> rules;  // [n_maps]
    HfParams p{};
};

extern "C" {

const char* lle_helpforest_last_error(void) { return sd::g_error.c_str(); }

void lle_helpforest_free(lle_helpforest* f) {
    if (!f) return;
    fc::close(f);
    delete f;
}

lle_helpforest* lle_helpforest_create(const lle_map* const* maps, int n_maps, const lle_helpforest_options* opt) {
    fc::Options o;
    if (!fc::read_options(maps, n_maps, opt, LIBRARY, &o)) return nullptr;
    auto* f = new lle_helpforest();
    f->rules.resize((size_t)n_maps);
    bool ok = true;
    for (int m = 0; ok && m < n_maps; m++) {
        std::string why;
        if (!sc::build_rule(maps[m], o.info, f->cells, f->rules[(size_t)m], why)) ok = (fail(LLE_ERR_UNSUPPORTED, why + " (map " + std::to_string(m) + ")"), false);
    }
    const fc::Table tables[2] = {{f->cells.data(), f->cells.size() * 4}, {f->rules.data(), f->rules.size() * sizeof(hl::EdgeRule)}};
    if (ok && fc::open(f, maps, n_maps, o, LIBRARY, tables, &f->p, lle::hf_roots) == LLE_OK) {
        HfParams& p = f->p;
        p.cells = static_cast<const uint32_t*>(f->d_static[0]);
        p.rules = static_cast<const hl::EdgeRule*>(f->d_static[1]);
        p.root_extra = f->d_root_extra;
        p.cand_extra = f->d_cand;
        p.goal_extra = f->d_goal_extra;
        p.H = o.info.height;
        p.W = o.info.width;
        g_launched.fetch_or(1u << K_ROOTS);
        return f;
    }
    delete f;
    return nullptr;
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
    sd::DeviceGuard g(f->device);
    const bool help = hfl::kind_of(args->mode) == hfl::KIND_HELP;
    HfParams p = f->p;
    fc::begin_run(f, &p, args->collect_gems != 0);
    p.mode = args->mode;
    p.param = args->param;
    const sl::RecordLayout& r = p.lay;
    const int A = r.A;
    const size_t M = (size_t)f->n_maps, HW = (size_t)p.H * p.W;
    auto report = [&]() {
        for (size_t m = 0; m < M; m++) {
            const fc::MapRun& mr = f->maps[m];
            const bool plan = mr.progress.length >= 0;
            per_map[m].status = mr.progress.status;
            per_map[m].length = mr.progress.length;
            per_map[m].n_states = mr.progress.n_states;
            per_map[m].depth_reached = mr.progress.depth_reached;
            per_map[m].help_lo = plan && help ? mr.extra[0] : 0u;
            per_map[m].help_hi = plan && help ? mr.extra[1] : 0u;
            per_map[m].trail = plan && !help ? mr.extra[0] : 0u;
        }
    };

    // ---- every reset state (t = 0: its edges count), judged on the host with the kernels' own functions
    for (size_t m = 0; m < M; m++) {
        fc::MapRun& mr = f->maps[m];
        uint32_t* extra = f->h_extra + hfl::EXTRA_WORDS * m;
        if (search && !search[m]) {  // not asked for: idle from the first level
            mr.frontier.clear();
            mr.progress = hfl::skipped_progress();
            continue;
        }
        const uint32_t* root = f->roots.data() + m * (size_t)r.n_words;
        const uint32_t* cells = f->cells.data() + m * HW;
        const uint64_t root_edges = hl::state_edges([&](int w) { return root[w]; }, r, f->rules[m], [&](int c_) { return cells[c_]; });
        bool root_ok = !sl::anybody_dead(root[r.w_bits], A), accepted = true, dense = false;
        if (help) {
            root_ok = root_ok && !hl::violates(root_edges, p.mode, p.param, A);
            accepted = hl::accepts(root_edges, p.mode, A);
            extra[0] = hl::help_lo(root_edges);
            extra[1] = hl::help_hi(root_edges);
        } else {
            int budget = tl::WALK_BUDGET;
            const uint32_t root_trail = tl::layer_update(0u, root_edges, p.param, A, budget);
            dense = budget < 0;
            root_ok = root_ok && !dense && !tl::violates_sequence(root_trail, p.param, A);  // a reset state that holds a trail of N: no plan
            extra[0] = dense ? 0u : root_trail;
        }
        const bool solved = root_ok && accepted && sl::is_goal(root[r.w_bits], root[r.w_gems], r, p.collect_gems != 0u, p.G);
        mr.progress = fl::fresh_progress(root_ok && !solved);  // (not ok: no plan starts here)
        if (dense) mr.progress.status = LLE_TRAILS_DENSE;
        if (solved) {
            mr.progress.length = 0;
            mr.extra[0] = extra[0];
            mr.extra[1] = extra[1];
        }
    }
    return fc::run(f, p, args->t_max, help ? launch_of<hfl::KIND_HELP>() : launch_of<hfl::KIND_TRAIL>(), LIBRARY, g_launched, report);
}

int lle_helpforest_plan(const lle_helpforest* f, int map_index, uint8_t* out, int64_t cap) { return fc::plan(f, map_index, out, cap); }
int lle_helpforest_stats(const lle_helpforest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) {
    return fc::stats(f, map_index, frontier, expanded, cap);
}
int lle_helpforest_occupancy(const lle_helpforest* f, int64_t* valid_items, int64_t* launched_lanes) { return fc::occupancy(f, valid_items, launched_lanes); }
size_t lle_helpforest_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, g_launched.load(), buf, cap); }
size_t lle_helpforest_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, (1u << K_COUNT) - 1u, buf, cap); }

}  // extern "C"
