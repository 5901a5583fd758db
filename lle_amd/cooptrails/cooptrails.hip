// cooptrails.hip -- liblle_cooptrails.so: the longest help trail of every environment's episode (C ABI: include/lle_cooptrails.h;
// DESIGN.md section 4.15).
//
// The temporal half of the reference's PlanProfile (is_sequential, profile.py) for many environments in one launch behind the coop
// launch.  The library reads a batch only through lle_batch_get_buffer and a coop handle only through lle_coop_buffer and
// lle_coop_start_edges, so liblle_hip.so and liblle_coop.so keep their kernels.
//
// State: two trail values u64 [n] (4 bits per agent: the longest trail that ends there, saturating at 15; the running episode's and
// the last finished one's) and two profiles u8 [n][4].
// Kernel: the coop kernel's shape, one lane per (environment, agent) in groups of G = next power of two >= A lanes.  Lane a loads row a
// of the state's edges, the group gathers all rows into every lane, and -- only where the state has an edge -- lane x walks the trails
// that start at agent x (cooptrails_logic.hpp: registers only); a field-wise max butterfly combines the walks; the group's first lane
// stores.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "../../include/lle_cooptrails.h"
#include "../coop/tracker_core.hpp"
#include "cooptrails_logic.hpp"

namespace ct = lle_cooptrails_logic;
namespace eo = lle_episode_ops;

namespace lle {

constexpr int COOPTRAILS_THREADS = 256;
using lle_tracker_core::START_PITCH;  // per map: the start edges of every agent

struct CoopTrailsParams {
    const uint32_t* step_edges;  // LLE_COOP_STEP_EDGES [n][A]
    const uint32_t* starts;      // [n_maps][START_PITCH]
    const uint8_t* evcount;      // LLE_BUF_EVCOUNT
    const uint8_t* err;          // LLE_BUF_ERR
    uint64_t* episode_trails;    // [n]
    uint64_t* last_trails;       // [n]
    uint32_t* episode_tprofile;  // [n] (4 bytes each)
    uint32_t* last_tprofile;     // [n]
    const uint8_t* env_mask;
    int64_t n_envs, envs_per_map;
    int32_t A;
    uint32_t ops, flags;
};

template <int G>
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
#pragma unroll
    for (int off = G >> 1; off >= 1; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, G);
    return v;
}
// The field-wise maximum of the trail values of the G lanes of the group, in every lane.
template <int G>
__device__ __forceinline__ uint64_t group_field_max(uint64_t v) {
#pragma unroll
    for (int off = G >> 1; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, G), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, G);
        v = ct::field_max(v, (uint64_t)hi << 32 | lo);
    }
    return v;
}

// Lane a of group g of workgroup b serves agent a of environment b * (256 / G) + g.
template <int G>
__global__ __launch_bounds__(COOPTRAILS_THREADS) void cooptrails_kernel(CoopTrailsParams p) {
    static_assert(G >= 1 && G <= 16 && (G & (G - 1)) == 0, "a power of two that divides the wave64");
    constexpr int ENVS_PER_BLOCK = COOPTRAILS_THREADS / G;
    const int a = (int)(threadIdx.x % G);
    const int64_t env = (int64_t)blockIdx.x * ENVS_PER_BLOCK + (int64_t)(threadIdx.x / G);
    // (every exit and every branch on operations, flags and arcs below is uniform over a lane group: the cross-lane reads only touch
    // lanes of the own group, and none of them sits inside a walk)
    if (env >= p.n_envs) return;
    if (p.env_mask && p.env_mask[env] == 0) return;
    const uint32_t reset_ops = eo::reset_ops(p.flags, p.evcount + env);
    if ((p.ops | reset_ops) == 0u) return;
    const uint32_t own_ops = eo::own_ops(p.ops, p.flags, p.err + env);
    const bool agent = a < p.A;  // lanes A .. G-1 of a group carry no agent: their rows are zero and they walk nothing

    // ---- lane a loads row a of both layers; the group gathers every row into every lane
    uint32_t mine = 0u;  // bits 0-15: the state's row, bits 16-31: the start row
    if (agent) {
        if (own_ops & LLE_COOPTRAILS_MARK_POS) mine = ct::clean_row(p.step_edges[env * p.A + a], a, p.A);
        if ((own_ops | reset_ops) & LLE_COOPTRAILS_MARK_STARTS) mine |= ct::clean_row(p.starts[(env / p.envs_per_map) * START_PITCH + a], a, p.A) << 16;
    }
    uint64_t sw[4] = {0ull, 0ull, 0ull, 0ull}, tw[4] = {0ull, 0ull, 0ull, 0ull};  // (indexed by constants after unrolling: registers)
#pragma unroll
    for (int h = 0; h < G; h++) {
        const uint32_t r = (uint32_t)__shfl((int)mine, h, G);
        sw[h >> 2] |= (uint64_t)(r & 0xFFFFu) << (16 * (h & 3));
        tw[h >> 2] |= (uint64_t)(r >> 16) << (16 * (h & 3));
    }
    const ct::Arcs step{sw[0], sw[1], sw[2], sw[3]}, start{tw[0], tw[1], tw[2], tw[3]};

    uint64_t L = p.episode_trails[env], last = 0ull;
    const uint32_t prof = p.episode_tprofile[env];
    uint32_t count = (prof >> 8) & 255u, dense = (prof >> 16) & 1u;
    uint32_t last_prof = 0u;
    bool finished = false;
    const uint32_t valid = 1u << 24;

    // ---- the operations: the auto-reset's, then the caller's; stage 2 is the caller's MARK_POS (one walk in the code, not three)
#pragma unroll 1
    for (int stage = 0; stage < eo::STAGES; stage++) {
        const uint32_t ops = eo::stage_ops(reset_ops, own_ops, stage);
        if (ops & LLE_COOPTRAILS_FINISH) {
            last = L;
            last_prof = ct::longest(L) | count << 8 | dense << 16 | valid;
            finished = true;
        }
        if (ops & LLE_COOPTRAILS_CLEAR) { L = 0ull; count = 0u; dense = 0u; }
        if (ops & (LLE_COOPTRAILS_MARK_STARTS | LLE_COOPTRAILS_MARK_POS)) {
            const ct::Arcs e = stage == 2 ? step : start;
            if (ct::any_arc(e)) {  // (most states have no edge: nothing but the operations above)
                count = min(255u, count + 1u);
                bool gave_up = false;
                const uint64_t walked = agent ? ct::walk_from(L, e, a, &gave_up) : L;
                L = group_field_max<G>(walked);
                dense |= group_or<G>(gave_up ? 1u : 0u);
            }
        }
    }

    if (a == 0) {
        p.episode_trails[env] = L;
        p.episode_tprofile[env] = ct::longest(L) | count << 8 | dense << 16 | valid;
        if (finished) {
            p.last_trails[env] = last;
            p.last_tprofile[env] = last_prof;
        }
    }
}

template __global__ void cooptrails_kernel<1>(CoopTrailsParams);
template __global__ void cooptrails_kernel<2>(CoopTrailsParams);
template __global__ void cooptrails_kernel<4>(CoopTrailsParams);
template __global__ void cooptrails_kernel<8>(CoopTrailsParams);
template __global__ void cooptrails_kernel<16>(CoopTrailsParams);

}  // namespace lle

// ================================================================================================ host side (../coop/tracker_core.hpp)
using lle::CoopTrailsParams;
using namespace lle_abi_host;
namespace tc = lle_tracker_core;

static_assert(LLE_COOPTRAILS_FINISH == eo::FINISH && LLE_COOPTRAILS_CLEAR == eo::CLEAR && LLE_COOPTRAILS_MARK_STARTS == eo::MARK_STARTS &&
                  LLE_COOPTRAILS_MARK_POS == eo::MARK_POS && LLE_COOPTRAILS_HONOUR_AUTO_RESET == eo::HONOUR_AUTO_RESET &&
                  LLE_COOPTRAILS_SKIP_REFUSED == eo::SKIP_REFUSED && LLE_COOPTRAILS_BUF_COUNT == tc::N_ARRAYS,
              "the shared decode and the shared handle read this header's values");

struct lle_cooptrails : tc::Tracker<CoopTrailsParams> {
    int log2_g = 0;
};

namespace {

std::atomic<uint32_t> g_launched{0};
// bit log2(G)
const char* const KERNEL_NAMES[5] = {"cooptrails_kernel<1>", "cooptrails_kernel<2>", "cooptrails_kernel<4>", "cooptrails_kernel<8>", "cooptrails_kernel<16>"};

// One launch of cooptrails_kernel<1 << log2_g> over p.n_envs environments.
int launch(const CoopTrailsParams& p, int log2_g, hipStream_t st) {
    const int G = 1 << log2_g;
    const int64_t envs_per_block = lle::COOPTRAILS_THREADS / G;
    const int64_t blocks = (p.n_envs + envs_per_block - 1) / envs_per_block;
    if (blocks <= 0 || blocks > 0x7FFFFFFF) return fail(LLE_ERR_ARG, "too many environments for one launch");
    const dim3 grid((uint32_t)blocks), block(lle::COOPTRAILS_THREADS);
    switch (G) {
        case 1: hipLaunchKernelGGL((lle::cooptrails_kernel<1>), grid, block, 0, st, p); break;
        case 2: hipLaunchKernelGGL((lle::cooptrails_kernel<2>), grid, block, 0, st, p); break;
        case 4: hipLaunchKernelGGL((lle::cooptrails_kernel<4>), grid, block, 0, st, p); break;
        case 8: hipLaunchKernelGGL((lle::cooptrails_kernel<8>), grid, block, 0, st, p); break;
        case 16: hipLaunchKernelGGL((lle::cooptrails_kernel<16>), grid, block, 0, st, p); break;
        default: return fail(LLE_ERR_UNSUPPORTED, "more agents than the cooptrails kernel serves");
    }
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "cooptrails launch failed");
    g_launched.fetch_or(1u << log2_g);
    return LLE_OK;
}

}  // namespace

extern "C" {

const char* lle_cooptrails_last_error(void) { return g_error.c_str(); }

void lle_cooptrails_free(lle_cooptrails* t) { tc::destroy(t); }

lle_cooptrails* lle_cooptrails_create(lle_batch* batch, lle_coop* coop, void* stream) {
    auto* t = tc::bind<lle_cooptrails>(batch, coop, "no HIP device: the temporal cooperation tracker runs on the GPU only (there is no CPU fallback)",
                                       tc::AgentLimit{ct::MAX_AGENTS, nullptr});
    if (!t || !tc::allocate(t, {8, 8, 4, 4}, "allocating the cooptrails arrays failed", stream)) return nullptr;
    CoopTrailsParams& p = t->p;
    p.episode_trails = reinterpret_cast<uint64_t*>(t->arrays[LLE_COOPTRAILS_EPISODE_TRAILS]);
    p.last_trails = reinterpret_cast<uint64_t*>(t->arrays[LLE_COOPTRAILS_LAST_TRAILS]);
    p.episode_tprofile = reinterpret_cast<uint32_t*>(t->arrays[LLE_COOPTRAILS_EPISODE_TPROFILE]);
    p.last_tprofile = reinterpret_cast<uint32_t*>(t->arrays[LLE_COOPTRAILS_LAST_TPROFILE]);
    int G = 1;
    while (G < p.A) G <<= 1, t->log2_g++;
    return t;
}

int lle_cooptrails_update_map(lle_cooptrails* t, int map_index, void* stream) { return tc::update_map(t, map_index, stream); }

void* lle_cooptrails_buffer(lle_cooptrails* t, int which) {
    return tc::buffer(t, which, "NULL handle or `which` not one of LLE_COOPTRAILS_EPISODE_TRAILS ... LLE_COOPTRAILS_LAST_TPROFILE");
}

int lle_cooptrails_update(lle_cooptrails* t, const lle_cooptrails_update_args* args, void* stream) {
    return tc::update(t, args, "lle_cooptrails_update_args", stream, [t](const CoopTrailsParams& p, hipStream_t st) { return launch(p, t->log2_g, st); });
}

size_t lle_cooptrails_debug_launched(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 5, g_launched.load(), buf, cap); }
size_t lle_cooptrails_debug_compiled(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 5, 0x1Fu, buf, cap); }

}  // extern "C"
