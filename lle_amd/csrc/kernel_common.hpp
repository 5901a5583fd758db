// kernel_common.hpp -- pieces shared by world_kernel (kernels.hip) and step_kernel (step_kernel.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "kernels.h"
#include "obs_stream.hpp"
#include "step_logic.hpp"
#include "tables.h"

namespace lle {

enum Mode : int { MODE_STEP = 0, MODE_RESET = 1, MODE_SET_STATE = 2, MODE_OBSERVE = 3, MODE_SOURCES = 4, MODE_ENV_SOURCES = 5 };

// Wavefront sums without LDS: DPP row operations inside every row of 16 lanes (xor 1, xor 2 as quad permutes, then the mirrors of the
// half row and of the row -- after them every lane holds its row's sum), and the four rows through v_readlane: the result is a SCALAR.
// (__shfl_xor is ds_bpermute_b32: six dependent LDS round trips per sum.)  Compiler builtins, not inline asm: the compiler places the DPP
// hazard waits.  Call in wave-uniform control flow with every lane active; a lane that has nothing to add passes zero.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_row_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += dpp_row_u32<DPP_QUAD_XOR1>(v);
    v += dpp_row_u32<DPP_QUAD_XOR2>(v);
    v += dpp_row_u32<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_row_u32<DPP_ROW_MIRROR>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_row_u64(uint64_t v) {
    return ((uint64_t)dpp_row_u32<CTRL>((uint32_t)(v >> 32)) << 32) | dpp_row_u32<CTRL>((uint32_t)v);
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    v += dpp_row_u64<DPP_QUAD_XOR1>(v);
    v += dpp_row_u64<DPP_QUAD_XOR2>(v);
    v += dpp_row_u64<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_row_u64<DPP_ROW_MIRROR>(v);
    uint64_t s = 0;
#pragma unroll
    for (int r = 0; r < 64; r += 16)
        s += ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), r) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, r);
    return s;
}

// per-wave partial counters (step_logic.hpp StepCounts); the slot of a wave is private, so no atomics.
// The wavefront's row of the counters: lane k < 8 holds counter k.  `preloaded`: the old values were read at the top of
// the kernel (stats_preload) -- a load HERE is answered only after every observation store the wavefront has in flight
// (the vmcnt counter is in order), which keeps the wavefront alive for one more memory round trip after its last
// store.  (Atomic adds without return need no load either, but 8 atomics per wavefront measured 0.6 us slower per launch.)
__device__ __forceinline__ int64_t stats_preload(const int64_t* __restrict__ stats, uint32_t wave_id, uint32_t lane) {
    return lane < 8 ? stats[(int64_t)wave_id * 8 + lane] : 0;
}
// (`c`: the wavefront's sums -- wave-uniform)
__device__ __forceinline__ void store_stats(int64_t* __restrict__ stats, uint32_t wave_id, const StepCounts& c, int A, uint32_t lane, bool preloaded, int64_t old) {
    const int64_t steps = c.steps, gems = c.gems, exits = c.exits, died = c.died, invalid = c.invalid, resets = c.resets, bonus = c.bonus;
    const int64_t v = lane == 0 ? steps : lane == 1 ? steps * A : lane == 2 ? gems : lane == 3 ? exits : lane == 4 ? died
                    : lane == 5 ? invalid : lane == 6 ? resets : gems + exits - died + bonus;
    if (preloaded) {
        if (lane < 8) stats[(int64_t)wave_id * 8 + lane] = old + v;
    } else if (lane == 0) {
        int64_t* out = stats + (int64_t)wave_id * 8;
        out[0] += steps; out[1] += steps * A; out[2] += gems; out[3] += exits; out[4] += died;
        out[5] += invalid; out[6] += resets; out[7] += gems + exits - died + bonus;
    }
}
__device__ __forceinline__ void flush_stats(int64_t* __restrict__ stats, uint32_t wave_id, const StepCounts& c, int A, uint32_t lane,
                                            bool preloaded = false, int64_t old = 0) {
    const StepCounts sums = {wave_sum_u32(c.steps), wave_sum_u32(c.gems), wave_sum_u32(c.exits), wave_sum_u32(c.died),
                             wave_sum_u32(c.invalid), wave_sum_u32(c.resets), wave_sum_u32(c.bonus)};
    store_stats(stats, wave_id, sums, A, lane, preloaded, old);
}
// One step: the seven counters as the two packed words of step_logic.hpp (stat_pack_reward / stat_pack_flags; zero in a lane that leads
// no environment) -- two sums instead of seven.  The caller asserts stat_fields_fit for its wavefront.
__device__ __forceinline__ void flush_stats_packed(int64_t* __restrict__ stats, uint32_t wave_id, uint32_t reward_word, uint32_t flags_word, int A, uint32_t lane,
                                                   bool preloaded, int64_t old) {
    store_stats(stats, wave_id, stat_unpack(wave_sum_u32(reward_word), wave_sum_u32(flags_word)), A, lane, preloaded, old);
}

// ---- per-env record I/O.  The per-agent buffers (pos, avail, actions, events) are laid out with a stride of AM
// agents per env (AM = the kernel instantiation's bound, >= the map's A), so a record is a whole number of dwords
// whatever A is, and moves as dwords (the compiler merges neighbours into dwordx2/x4).
template <int AM>
__device__ __forceinline__ void store_u16_record(uint16_t* __restrict__ base, int64_t env, const uint32_t (&v)[AM]) {
    uint32_t* __restrict__ w = reinterpret_cast<uint32_t*>(base) + env * (AM / 2);
#pragma unroll
    for (int k = 0; k < AM / 2; k++) w[k] = (v[2 * k] & 0xFFFFu) | (v[2 * k + 1] << 16);
}
template <int AM>
__device__ __forceinline__ void load_u8_record(const uint8_t* __restrict__ base, int64_t env, uint32_t (&out)[AM]) {
    const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(base) + env * (AM / 4);
#pragma unroll
    for (int k = 0; k < AM / 4; k++) {
        const uint32_t v = w[k];
#pragma unroll
        for (int q = 0; q < 4; q++) out[4 * k + q] = (v >> (8 * q)) & 0xFFu;
    }
}
template <int AM>
__device__ __forceinline__ void store_u8_record(uint8_t* __restrict__ base, int64_t env, const uint32_t (&v)[AM]) {
    uint32_t* __restrict__ w = reinterpret_cast<uint32_t*>(base) + env * (AM / 4);
#pragma unroll
    for (int k = 0; k < AM / 4; k++)
        w[k] = (v[4 * k] & 0xFFu) | ((v[4 * k + 1] & 0xFFu) << 8) | ((v[4 * k + 2] & 0xFFu) << 16) | (v[4 * k + 3] << 24);
}

}  // namespace lle
