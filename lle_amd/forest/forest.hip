// forest.hip -- liblle_forest.so: the exact shortest joint plans of many equally shaped maps at once, one breadth-first tree per map,
// every tree walked depth by depth in the same launches (C ABI: include/lle_forest.h; DESIGN.md "Forest search").
//
// The library touches its batch only through include/lle_hip.h, like search.hip: ONE lle_batch of n_maps * E environments made with
// lle_batch_create_multi, in which map m owns the environments [m * E, (m + 1) * E).  Per map a segment of everything search.hip
// keeps: `cap` pool records (structure of arrays inside the segment), parent (u32, local index) and action (u16) per state, a table
// segment of a power of two >= max(2 cap, cap + E + 1) slots, eight u64 counters and the foreign-beam table (H * W bytes).  Which lane
// serves which map, the descriptors, the per-map counters and fates are forest_logic.hpp's; the kernel bodies, the handle, the two
// halves of a create, the level loop and the plan read-back are forest_core.hpp's, shared with ../helpforest/helpforest.hip: this is the
// forest over the plain kind (sl::PlainKind), no extra words, so every map's search is exactly search.hip's.
//
// Here are the kernels under their names, the C ABI with its argument checks, the judgement of the reset states and the no-cooperation
// filter: its table is read from memory (a workgroup spans several maps when E is no multiple of 256), H * W bytes that stay in cache.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lle_forest.h"
#include "forest_core.hpp"
#include "forest_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace fl = lle_forest_logic;
namespace fc = lle_forest_core;
using sd::fail;

namespace lle {

struct ForestParams : fc::Params {
    const uint8_t* foreign;  // [n_maps][H * W]
    int32_t H, W;
};

__global__ __launch_bounds__(fc::THREADS) void forest_roots(ForestParams p) { fc::roots(p); }
__global__ __launch_bounds__(fc::THREADS) void forest_seed(ForestParams p) { fc::seed<sl::PlainKind>(p, nullptr); }
__global__ __launch_bounds__(fc::THREADS) void forest_expand(ForestParams p) { fc::expand(p); }

// NO_COOP: mode no-cooperation.
template <bool NO_COOP>
__global__ __launch_bounds__(fc::THREADS) void forest_insert(ForestParams p) {
    const int64_t k = fc::lane();
    if (!fc::insert_front(p, k)) return;
    if constexpr (NO_COOP) {
        const uint8_t* foreign = p.foreign + fl::foreign_base(k / p.E, p.H, p.W);
        for (int a = 0; a < p.lay.A; a++) {
            const uint8_t* q = p.b.pos + k * p.b.pos_stride + a * p.b.pos_agent_stride;
            const int i = q[0], j = q[1];
            if (i < p.H && j < p.W && sl::on_foreign_beam(foreign[i * p.W + j], a)) return;
        }
    }
    fc::insert_back(p, sl::PlainKind{}, nullptr, nullptr, k);
}

__global__ __launch_bounds__(fc::THREADS) void forest_commit(ForestParams p) {
    const int64_t k = fc::lane();
    if (fc::is_winner(p, k)) fc::commit(p, sl::PlainKind{}, nullptr, k);
}

__global__ __launch_bounds__(fc::THREADS) void forest_plans(ForestParams p) { fc::plans<sl::PlainKind>(p, nullptr); }

template __global__ void forest_insert<false>(ForestParams);
template __global__ void forest_insert<true>(ForestParams);

}  // namespace lle

// ================================================================================================ host side
using lle::ForestParams;

namespace {

std::atomic<uint32_t> g_launched{0};
enum { K_ROOTS = 0, K_SEED, K_EXPAND, K_INSERT, K_INSERT_NO_COOP, K_COMMIT, K_PLANS, K_COUNT };
const char* const KERNEL_NAMES[K_COUNT] = {"forest_roots", "forest_seed", "forest_expand", "forest_insert<false>", "forest_insert<true>", "forest_commit",
                                           "forest_plans"};
const fc::Library LIBRARY = {"forest", "lle_forest_options", "the search", "state", sl::PlainKind::EXTRA, LLE_SEARCH_CAPACITY, 0};

static_assert(LLE_SEARCH_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_search.h and search_logic.hpp disagree");

}  // namespace

struct lle_forest : fc::Handle {
    std::vector<uint8_t> foreign;  // [n_maps][H * W]: host copy of the foreign-beam tables, for the reset states
    ForestParams p{};
};

extern "C" {

const char* lle_forest_last_error(void) { return sd::g_error.c_str(); }

void lle_forest_free(lle_forest* f) {
    if (!f) return;
    fc::close(f);
    delete f;
}

lle_forest* lle_forest_create(const lle_map* const* maps, int n_maps, const lle_forest_options* opt) {
    fc::Options o;
    if (!fc::read_options(maps, n_maps, opt, LIBRARY, &o)) return nullptr;
    auto* f = new lle_forest();
    const int H = o.info.height, W = o.info.width;
    bool ok = true;
    for (int m = 0; ok && m < n_maps; m++)
        if (!sd::build_foreign(maps[m], H, W, f->foreign)) ok = (fail(LLE_ERR_ARG, "laser tile out of range (map " + std::to_string(m) + ")"), false);
    const fc::Table tables[2] = {{f->foreign.data(), f->foreign.size()}, {nullptr, 0}};
    if (ok && fc::open(f, maps, n_maps, o, LIBRARY, tables, &f->p, lle::forest_roots) == LLE_OK) {
        f->p.foreign = static_cast<const uint8_t*>(f->d_static[0]);
        f->p.H = H;
        f->p.W = W;
        g_launched.fetch_or(1u << K_ROOTS);
        return f;
    }
    delete f;
    return nullptr;
}

int lle_forest_run(lle_forest* f, const lle_search_args* args, lle_forest_result* per_map) {
    if (!f || !args || !per_map) return fail(LLE_ERR_NULL, "NULL handle, arguments or results");
    if (args->struct_bytes != sizeof(lle_search_args)) return fail(LLE_ERR_ARG, "lle_search_args.struct_bytes is not sizeof(lle_search_args)");
    if (args->mode != LLE_SEARCH_STANDARD && args->mode != LLE_SEARCH_NO_COOPERATION) return fail(LLE_ERR_ARG, "unknown mode");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    sd::DeviceGuard g(f->device);
    const bool no_coop = args->mode == LLE_SEARCH_NO_COOPERATION;
    ForestParams p = f->p;
    fc::begin_run(f, &p, args->collect_gems != 0);
    const sl::RecordLayout& r = p.lay;
    const size_t M = (size_t)f->n_maps, HW = (size_t)p.H * p.W;
    auto report = [&]() {
        for (size_t m = 0; m < M; m++) {
            const fl::MapProgress& pr = f->maps[m].progress;
            per_map[m].status = pr.status;
            per_map[m].length = pr.length;
            per_map[m].n_states = pr.n_states;
            per_map[m].depth_reached = pr.depth_reached;
            per_map[m].pad = 0;
        }
    };

    // ---- every reset state, judged on the host with the kernels' own functions
    for (size_t m = 0; m < M; m++) {
        const uint32_t* root = f->roots.data() + m * (size_t)r.n_words;
        const bool root_ok = !sl::anybody_dead(root[r.w_bits], r.A) && !(no_coop && sl::root_on_foreign_beam(root, r, f->foreign.data() + m * HW, p.H, p.W));
        const bool solved = root_ok && sl::is_goal(root[r.w_bits], root[r.w_gems], r, p.collect_gems != 0u, p.G);
        fl::MapProgress& pr = f->maps[m].progress;
        pr = fl::fresh_progress(root_ok && !solved);  // (not ok: no plan starts here)
        if (solved) pr.length = 0;
    }
    const fc::Launch<ForestParams> launch = {lle::forest_seed, lle::forest_expand, no_coop ? lle::forest_insert<true> : lle::forest_insert<false>, lle::forest_commit,
                                             lle::forest_plans, 1u << K_SEED, 1u << K_EXPAND | 1u << (no_coop ? K_INSERT_NO_COOP : K_INSERT) | 1u << K_COMMIT,
                                             1u << K_PLANS};
    return fc::run(f, p, args->t_max, launch, LIBRARY, g_launched, report);
}

int lle_forest_plan(const lle_forest* f, int map_index, uint8_t* out, int64_t cap) { return fc::plan(f, map_index, out, cap); }
int lle_forest_stats(const lle_forest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap) { return fc::stats(f, map_index, frontier, expanded, cap); }
int lle_forest_occupancy(const lle_forest* f, int64_t* valid_items, int64_t* launched_lanes) { return fc::occupancy(f, valid_items, launched_lanes); }
size_t lle_forest_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, g_launched.load(), buf, cap); }
size_t lle_forest_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, K_COUNT, (1u << K_COUNT) - 1u, buf, cap); }

}  // extern "C"
