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
// in pieces of at most `chunk` items, four launches each: search_expand, lle_batch_step, search_insert, search_commit.  What they do,
// the handle, the level loop and the plan walk are search_core.hpp's, shared with ../helpgraph/helpgraph.hip and ../trails/trails.hip:
// this is the search over the plain kind, no extra words.  What all searches share with ../forest/forest.hip and the steps-to-go
// library lives in search_logic.hpp (host and device: record layout, hash, table, record I/O) and search_device.hpp (HIP: error
// string, device guard, batch binding, reset state, foreign-beam table).  Here are the kernels under their names, the no-cooperation
// filter with its LDS foreign table, the C ABI with its argument checks, the judgement of the reset state and the lower bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <deque>
#include <vector>

#include "../../include/lle_search.h"
#include "search_core.hpp"
#include "search_device.hpp"
#include "search_logic.hpp"

namespace sl = lle_search_logic;
namespace sd = lle_search_device;
namespace sc = lle_search_core;
using sd::fail;

namespace lle {

constexpr int SEARCH_THREADS = 256;
static_assert(SEARCH_THREADS == sc::THREADS, "search_core.hpp counts lanes in workgroups of sc::THREADS");

struct SearchParams : sc::Params {
    const uint8_t* foreign;  // [H * W]: colours of the sources that own a laser tile on the cell (bit min(colour, 7))
    int32_t H, W;
};

__global__ __launch_bounds__(SEARCH_THREADS) void search_expand(SearchParams p) { sc::expand(p); }

// NO_COOP: mode no-cooperation, the foreign-beam table staged in LDS (one byte per cell: at most 255 x 255 bytes).
template <bool NO_COOP>
__global__ __launch_bounds__(SEARCH_THREADS) void search_insert(SearchParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_foreign[];
    if constexpr (NO_COOP) {  // (every lane of the workgroup gets here: no exit before the barrier)
        const int HW = p.H * p.W;
        for (int c = threadIdx.x; c < HW; c += SEARCH_THREADS) lds_foreign[c] = p.foreign[c];
        __syncthreads();
    }
    const uint32_t k = sc::lane();
    if (k >= p.n_items || !sc::insert_front(p, k)) return;
    if constexpr (NO_COOP) {
        for (int a = 0; a < p.lay.A; a++) {
            const uint8_t* q = p.b.pos + (int64_t)k * p.b.pos_stride + a * p.b.pos_agent_stride;
            const int i = q[0], j = q[1];
            if (i < p.H && j < p.W && sl::on_foreign_beam(lds_foreign[i * p.W + j], a)) return;
        }
    }
    sc::insert_back(p, sl::PlainKind{}, sc::Cells{nullptr}, nullptr, k);
}

__global__ __launch_bounds__(SEARCH_THREADS) void search_commit(SearchParams p) { sc::commit(p, sl::PlainKind{}, nullptr, sc::lane()); }

template __global__ void search_insert<false>(SearchParams);
template __global__ void search_insert<true>(SearchParams);

}  // namespace lle

// ================================================================================================ host side
namespace {

std::atomic<uint32_t> g_launched{0};
const char* const KERNEL_NAMES[4] = {"search_expand", "search_insert<false>", "search_insert<true>", "search_commit"};
const sc::Library LIBRARY = {"search", "lle_search_options", "the search", "state", "", sl::PlainKind::EXTRA, 0, LLE_SEARCH_CAPACITY, 0};
static_assert(LLE_SEARCH_MAX_AGENTS == sl::MAX_AGENTS, "include/lle_search.h and search_logic.hpp disagree");

}  // namespace

struct lle_search : sc::Handle {
    std::vector<uint8_t> foreign;  // [H * W]: host copy of the foreign-beam table, for the reset state
    lle::SearchParams p{};
};

extern "C" {

const char* lle_search_last_error(void) { return sd::g_error.c_str(); }

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
    sc::close(s);
    delete s;
}

lle_search* lle_search_create(const lle_map* map, const lle_search_options* opt) {
    sc::Options o;
    if (!sc::read_options(map, opt, LIBRARY, &o)) return nullptr;
    auto* s = new lle_search();
    if (!sd::build_foreign(map, o.info.height, o.info.width, s->foreign)) {
        fail(LLE_ERR_ARG, "laser tile out of range");
    } else if (sc::limits_ok(o.info, LIBRARY) && sc::open(s, map, o, LIBRARY, s->foreign.data(), s->foreign.size(), &s->p) == LLE_OK) {
        s->p.foreign = static_cast<const uint8_t*>(s->d_static);
        s->p.H = o.info.height;
        s->p.W = o.info.width;
        return s;
    }
    delete s;
    return nullptr;
}

int lle_search_run(lle_search* s, const lle_search_args* args, lle_search_result* result) {
    if (!s || !args || !result) return fail(LLE_ERR_NULL, "NULL handle, arguments or result");
    if (args->struct_bytes != sizeof(lle_search_args)) return fail(LLE_ERR_ARG, "lle_search_args.struct_bytes is not sizeof(lle_search_args)");
    if (result->struct_bytes != sizeof(lle_search_result)) return fail(LLE_ERR_ARG, "lle_search_result.struct_bytes is not sizeof(lle_search_result)");
    if (args->mode != LLE_SEARCH_STANDARD && args->mode != LLE_SEARCH_NO_COOPERATION) return fail(LLE_ERR_ARG, "unknown mode");
    if (args->t_max < 0) return fail(LLE_ERR_ARG, "t_max must not be negative");
    sd::DeviceGuard g(s->device);
    const bool no_coop = args->mode == LLE_SEARCH_NO_COOPERATION;
    lle::SearchParams p = s->p;
    sc::begin_run(s, &p, args->collect_gems != 0);
    const sl::RecordLayout& r = p.lay;
    sc::Outcome out;
    auto report = [&](int rc) {
        result->length = out.length;
        result->n_states = out.n_states;
        result->depth_reached = out.depth_reached;
        result->pad = 0;
        result->step_errors = out.step_errors;
        return rc;
    };

    // ---- the reset state, judged on the host with the kernels' own functions
    const std::vector<uint32_t>& root = s->root;
    if (sl::anybody_dead(root[(size_t)r.w_bits], r.A) || (no_coop && sl::root_on_foreign_beam(root.data(), r, s->foreign.data(), p.H, p.W)))
        return report(LLE_OK);  // no plan starts here
    if (sl::is_goal(root[(size_t)r.w_bits], root[(size_t)r.w_gems], r, p.collect_gems != 0u, p.G)) {
        s->length = out.length = 0;
        return report(LLE_OK);
    }
    // (the byte table is staged only where it is read: in no-cooperation mode)
    const sc::Launch<lle::SearchParams> launch = {lle::search_expand, no_coop ? lle::search_insert<true> : lle::search_insert<false>, lle::search_commit,
                                                  no_coop ? ((size_t)p.H * p.W + 15) / 16 * 16 : 0, no_coop};
    return report(sc::search_tree(s, p, args->t_max, nullptr, launch, LIBRARY, g_launched, &out));
}

int lle_search_plan(const lle_search* s, uint8_t* out, int64_t cap) { return sc::plan(s, out, cap); }
int lle_search_stats(const lle_search* s, int64_t* frontier, int64_t* expanded, int cap) { return sc::stats(s, frontier, expanded, cap); }
size_t lle_search_debug_launched(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, g_launched.load(), buf, cap); }
size_t lle_search_debug_compiled(char* buf, size_t cap) { return sd::names_out(KERNEL_NAMES, 4, 0xFu, buf, cap); }

}  // extern "C"
