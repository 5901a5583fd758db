// coopcycles.hip -- liblle_coopcycles.so: the closed help trails of every environment's episode (C ABI: include/lle_coopcycles.h;
// DESIGN.md section 4.18).
//
// The reference's PlanProfile.is_interdependent(n_agents) (profile.py) for many environments in one launch behind the coop and the
// cooptrails launches.  The library reads a batch only through lle_batch_get_buffer and a coop handle only through lle_coop_buffer and
// lle_coop_start_edges, so the other libraries keep their kernels.
//
// State: two packed sets of (anchor, current, support) triples u32 [W][n] (../cycles/cycles_logic.hpp: THE VALUE and THE BITS; word-major,
// so the loads of one word by a wavefront coalesce; the running episode's and the last finished one's) and two profiles u8 [n][4].
// Kernel: ONE lane per environment.  A lane loads its A rows of the state's edges, packs them into the 48-bit arc word of the search
// (bit 8 h + b) and -- only where the state has an arc -- runs cl::layer_update<W>, the function the closed-trail search runs per
// record, byte for byte, with an order that never prunes and never closes.  The new value of a layer is built in the lane's own words
// (W = 3: a private array; W = 21: a slab of LDS, word i of lane l at i * 256 + l, no barrier) and goes to the lane's own global words
// only when the walk stayed within its budget; a further layer of the same launch reads it back from there.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#include "../../include/lle_coopcycles.h"
#include "../coop/tracker_core.hpp"
#include "../cycles/cycles_logic.hpp"

namespace cl = lle_cycles_logic;
namespace eo = lle_episode_ops;

namespace lle {

constexpr int COOPCYCLES_THREADS = 256;
using lle_tracker_core::START_PITCH;  // per map: the start edges of every agent

static_assert(LLE_COOPCYCLES_MAX_AGENTS == cl::sl::MAX_AGENTS && LLE_COOPCYCLES_WALK_BUDGET == cl::WALK_BUDGET, "the header's constants");
static_assert(LLE_COOPCYCLES_SMALL_WORDS == cl::SMALL_WORDS && LLE_COOPCYCLES_LARGE_WORDS == cl::LARGE_WORDS, "the header's constants");

struct CoopCyclesParams {
    const uint32_t* step_edges;  // LLE_COOP_STEP_EDGES [n][A]
    const uint32_t* starts;      // [n_maps][START_PITCH]
    const uint8_t* evcount;      // LLE_BUF_EVCOUNT
    const uint8_t* err;          // LLE_BUF_ERR
    uint32_t* episode_closed;    // [W][n]
    uint32_t* last_closed;       // [W][n]
    uint32_t* episode_cprofile;  // [n] (4 bytes each)
    uint32_t* last_cprofile;     // [n]
    const uint8_t* env_mask;
    int64_t n_envs, envs_per_map;
    cl::Order order;             // {A, every mask, none}: the walk stores every triple and never stops on a closed one
    uint64_t of_size[cl::MAX_ORDER + 1];  // cl::masks_of_size(k), worked out on the host
    int32_t A;
    uint32_t ops, flags;
};

// The running episode's words of one environment as layer_update reads them: global memory, or nothing after a CLEAR.
struct EpisodeWords {
    const uint32_t* base;  // word 0 of the environment
    int64_t stride;        // n_envs
    bool empty;
    __host__ __device__ uint32_t operator()(int i) const { return empty ? 0u : base[(int64_t)i * stride]; }
};

// The closed orders of a value as a bit set: bit k = some (a, a, S) with |S| = k.
template <int W, class Read>
__device__ uint32_t closed_orders(const Read& words, int A, const uint64_t* of_size) {
    uint64_t closed = 0ull;
    for (int a = 0; a < A; a++) closed |= cl::supports<W>(words, a, a);
    uint32_t orders = 0u;
    for (int k = cl::MIN_ORDER; k <= cl::MAX_ORDER; k++)
        if (closed & of_size[k]) orders |= 1u << k;
    return orders;
}

// Lane l of workgroup b serves environment b * 256 + l.
template <int W>
__global__ __launch_bounds__(COOPCYCLES_THREADS) void coopcycles_kernel(CoopCyclesParams p) {
    const int64_t env = (int64_t)blockIdx.x * COOPCYCLES_THREADS + (int64_t)threadIdx.x;
    // (no barrier and no cross-lane read in this kernel: a lane may leave at any point)
    if (env >= p.n_envs) return;
    if (p.env_mask && p.env_mask[env] == 0) return;
    const uint32_t reset_ops = eo::reset_ops(p.flags, p.evcount + env);
    if ((p.ops | reset_ops) == 0u) return;
    const uint32_t own_ops = eo::own_ops(p.ops, p.flags, p.err + env);
    const int A = p.A;

    // ---- the arc words of both layers: bit 8 h + b = h helps b
    uint64_t step = 0ull, start = 0ull;
    if (own_ops & LLE_COOPCYCLES_MARK_POS)
        for (int h = 0; h < A; h++) step |= (uint64_t)eo::clean_row(p.step_edges[env * A + h], h, A) << (8 * h);
    if ((own_ops | reset_ops) & LLE_COOPCYCLES_MARK_STARTS)
        for (int h = 0; h < A; h++) start |= (uint64_t)eo::clean_row(p.starts[(env / p.envs_per_map) * START_PITCH + h], h, A) << (8 * h);

    // ---- the lane's own words for the value a layer builds
    cl::Words out;
    [[maybe_unused]] uint32_t mine[cl::SMALL_WORDS];
    if constexpr (W == cl::SMALL_WORDS) {
        out = cl::Words{mine, 1};
    } else {
        __shared__ uint32_t slabs[W * COOPCYCLES_THREADS];  // word i of lane l at i * 256 + l: a wavefront's accesses of one word fall into 64 banks
        out = cl::Words{slabs + threadIdx.x, COOPCYCLES_THREADS};
    }

    uint32_t* const episode = p.episode_closed + env;  // word i at episode[i * n_envs]
    uint32_t* const last = p.last_closed + env;
    const uint32_t prof = p.episode_cprofile[env];
    uint32_t orders = prof & 255u, count = (prof >> 8) & 255u, dense = (prof >> 16) & 1u;
    const uint32_t valid = 1u << 24;
    bool cleared = false;  // the episode's value is empty, its global words not yet

    // ---- the operations: the auto-reset's, then the caller's; stage 2 is the caller's MARK_POS (one walk in the code, not three)
#pragma unroll 1
    for (int stage = 0; stage < eo::STAGES; stage++) {
        const uint32_t ops = eo::stage_ops(reset_ops, own_ops, stage);
        if (ops & LLE_COOPCYCLES_FINISH) {
            for (int i = 0; i < W; i++) last[(int64_t)i * p.n_envs] = cleared ? 0u : episode[(int64_t)i * p.n_envs];
            p.last_cprofile[env] = orders | count << 8 | dense << 16 | valid;
        }
        if (ops & LLE_COOPCYCLES_CLEAR) { cleared = true; orders = 0u; count = 0u; dense = 0u; }
        if (ops & (LLE_COOPCYCLES_MARK_STARTS | LLE_COOPCYCLES_MARK_POS)) {
            const uint64_t edges = stage == 2 ? step : start;
            if (edges != 0ull) {  // (most states have no arc: nothing but the operations above)
                count = min(255u, count + 1u);
                int budget = cl::WALK_BUDGET;
                bool closed = false;  // (never set under p.order)
                cl::layer_update<W>(EpisodeWords{episode, p.n_envs, cleared}, out, edges, p.order, A, budget, closed);
                if (budget >= 0) {
                    for (int i = 0; i < W; i++) episode[(int64_t)i * p.n_envs] = out(i);
                    orders = closed_orders<W>(out, A, p.of_size);
                    cleared = false;
                } else {
                    dense = 1u;  // the layer is dropped whole: the value stays as it was
                }
            }
        }
    }

    if (cleared)
        for (int i = 0; i < W; i++) episode[(int64_t)i * p.n_envs] = 0u;
    const uint32_t now = orders | count << 8 | dense << 16 | valid;
    if (now != prof) p.episode_cprofile[env] = now;
}

template __global__ void coopcycles_kernel<cl::SMALL_WORDS>(CoopCyclesParams);
template __global__ void coopcycles_kernel<cl::LARGE_WORDS>(CoopCyclesParams);

}  // namespace lle

// ================================================================================================ host side (../coop/tracker_core.hpp)
using lle::CoopCyclesParams;
using namespace lle_abi_host;
namespace tc = lle_tracker_core;

static_assert(LLE_COOPCYCLES_FINISH == eo::FINISH && LLE_COOPCYCLES_CLEAR == eo::CLEAR && LLE_COOPCYCLES_MARK_STARTS == eo::MARK_STARTS &&
                  LLE_COOPCYCLES_MARK_POS == eo::MARK_POS && LLE_COOPCYCLES_HONOUR_AUTO_RESET == eo::HONOUR_AUTO_RESET &&
                  LLE_COOPCYCLES_SKIP_REFUSED == eo::SKIP_REFUSED && LLE_COOPCYCLES_BUF_COUNT == tc::N_ARRAYS,
              "the shared decode and the shared handle read this header's values");

struct lle_coopcycles : tc::Tracker<CoopCyclesParams> {
    int words = 0;
};

namespace {

std::atomic<uint32_t> g_launched{0};
// bit 0: W = 3, bit 1: W = 21
const char* const KERNEL_NAMES[2] = {"coopcycles_kernel<3>", "coopcycles_kernel<21>"};

// One launch of coopcycles_kernel<words> over p.n_envs environments.
int launch(const CoopCyclesParams& p, int words, hipStream_t st) {
    const int64_t blocks = (p.n_envs + lle::COOPCYCLES_THREADS - 1) / lle::COOPCYCLES_THREADS;
    if (blocks <= 0 || blocks > 0x7FFFFFFF) return fail(LLE_ERR_ARG, "too many environments for one launch");
    const dim3 grid((uint32_t)blocks), block(lle::COOPCYCLES_THREADS);
    if (words == cl::SMALL_WORDS) hipLaunchKernelGGL((lle::coopcycles_kernel<cl::SMALL_WORDS>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((lle::coopcycles_kernel<cl::LARGE_WORDS>), grid, block, 0, st, p);
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "coopcycles launch failed");
    g_launched.fetch_or(words == cl::SMALL_WORDS ? 1u : 2u);
    return LLE_OK;
}

// The refusal of a map with more agents than a value holds.  [[clang::noinline]] here and on masks_of_size below: the calls stay out
// of line, so that the library's dynamic symbols (those weak instantiations among them) are the ones it had when create was one function.
std::string too_many_agents(int A) {
    [[clang::noinline]] return "the closed-trail tracker serves maps of at most " + std::to_string(LLE_COOPCYCLES_MAX_AGENTS) +
                               " agents, this one has " + std::to_string(A) + ": a packed set of agent masks is one 64-bit word";
}

}  // namespace

extern "C" {

const char* lle_coopcycles_last_error(void) { return g_error.c_str(); }

void lle_coopcycles_free(lle_coopcycles* t) { tc::destroy(t); }

lle_coopcycles* lle_coopcycles_create(lle_batch* batch, lle_coop* coop, void* stream) {
    auto* t = tc::bind<lle_coopcycles>(batch, coop, "no HIP device: the closed-trail cooperation tracker runs on the GPU only (there is no CPU fallback)",
                                       tc::AgentLimit{LLE_COOPCYCLES_MAX_AGENTS, too_many_agents});
    if (!t) return nullptr;
    const int A = t->p.A;
    const size_t value_bytes = 4 * (size_t)cl::words_of(A);
    if (!tc::allocate(t, {value_bytes, value_bytes, 4, 4}, "allocating the coopcycles arrays failed", stream)) return nullptr;
    t->words = cl::words_of(A);
    CoopCyclesParams& p = t->p;
    p.episode_closed = reinterpret_cast<uint32_t*>(t->arrays[LLE_COOPCYCLES_EPISODE_CLOSED]);
    p.last_closed = reinterpret_cast<uint32_t*>(t->arrays[LLE_COOPCYCLES_LAST_CLOSED]);
    p.episode_cprofile = reinterpret_cast<uint32_t*>(t->arrays[LLE_COOPCYCLES_EPISODE_CPROFILE]);
    p.last_cprofile = reinterpret_cast<uint32_t*>(t->arrays[LLE_COOPCYCLES_LAST_CPROFILE]);
    p.order = cl::Order{A, ~0ull, 0ull};  // N = the map's agents, every mask allowed, none "exact": no pruning, no closing
    for (int k = 0; k <= cl::MAX_ORDER; k++) [[clang::noinline]] p.of_size[k] = cl::masks_of_size(k);
    return t;
}

int lle_coopcycles_update_map(lle_coopcycles* t, int map_index, void* stream) { return tc::update_map(t, map_index, stream); }

void* lle_coopcycles_buffer(lle_coopcycles* t, int which) {
    return tc::buffer(t, which, "NULL handle or `which` not one of LLE_COOPCYCLES_EPISODE_CLOSED ... LLE_COOPCYCLES_LAST_CPROFILE");
}

int lle_coopcycles_update(lle_coopcycles* t, const lle_coopcycles_update_args* args, void* stream) {
    return tc::update(t, args, "lle_coopcycles_update_args", stream, [t](const CoopCyclesParams& p, hipStream_t st) { return launch(p, t->words, st); });
}

size_t lle_coopcycles_debug_launched(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 2, g_launched.load(), buf, cap); }
size_t lle_coopcycles_debug_compiled(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 2, 0x3u, buf, cap); }

}  // extern "C"
