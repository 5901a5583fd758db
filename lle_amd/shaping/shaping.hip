// shaping.hip -- liblle_shaping.so: potential-based reward shaping and the LaserSubgoal extras of an lle_batch
// (C ABI: include/lle_shaping.h).
//
// PotentialShapedLLE (python/lle/env/reward_strategy.py:112-181) and LaserSubgoal (python/lle/env/extras_generators.py:75-101) of the
// reference for many environments in one launch.  The library reads a batch only through the public ABI of include/lle_hip.h
// (lle_batch_get_buffer: LLE_BUF_POS, LLE_BUF_EVCOUNT; lle_map_*), so liblle_hip.so keeps its kernels.
//
// State: two arrays u32 [n][A], bit l = agent a of the environment has stood on a beam tile of source laser_id l since the last
// clear -- one for the reward strategy, one for the extras generator.  A cell -> u32 table per map says which sources own a tile
// on the cell (World.lasers: the outer two layers only); marking an agent is one table lookup and an OR.
// Kernel: one lane per (environment, agent) in groups of G = next power of two >= A lanes, the lane-group shape of the step
// kernels; the per-environment count of reached entries is summed across the group with cross-lane reads inside the wave64 (no
// LDS, no atomics); the group's first lane writes the reward, every lane its own E extras.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_shaping.h"
#include "../common/abi_host.hpp"

// `gamma * prev - cur` must round the product before the subtraction, like numpy on Python floats: no FMA (also -ffp-contract=off).
#pragma clang fp contract(off)

namespace lle {

constexpr int SHAPING_THREADS = 256;
constexpr int START_PITCH = LLE_MAX_AGENTS;  // start masks per map
constexpr int LDS_TABLE_MAX_BYTES = 16384;   // a cell table up to 64 x 64 lives in LDS; larger ones stay in global memory (read-only, L2-resident)

struct ShapingParams {
    const uint32_t* tables;    // [n_maps][H * W] cell masks
    const uint32_t* starts;    // [n_maps][START_PITCH] cell mask of every agent's start cell
    const uint8_t* ecols;      // [E] laser_id of every extras column
    const uint8_t* pos;        // LLE_BUF_POS
    const uint8_t* evcount;    // LLE_BUF_EVCOUNT
    uint32_t* reached_s;       // [n][A] reward strategy
    uint32_t* reached_e;       // [n][A] extras generator
    const uint8_t* env_mask;
    const float* base_reward;
    float* reward_out;
    float* extras_out;
    int64_t pos_stride, pos_agent_stride;  // elements
    int64_t n_envs, envs_per_map;
    double gamma, reward_value;
    int32_t H, W, A, E;
    int32_t n_pbrs;            // entries of pbrs_cols (duplicates counted)
    int32_t n_mult;            // mult[k] = the sources listed more than k times
    uint32_t mult[LLE_SHAPING_MAX_REPEATS];
    uint32_t strategy_ops, extras_ops, flags;
    int32_t reward_kind;
};

__device__ __forceinline__ uint32_t apply_ops(uint32_t bits, uint32_t ops, uint32_t start, uint32_t here, uint32_t& before_pos) {
    if (ops & LLE_SHAPING_CLEAR) bits = 0u;
    if (ops & LLE_SHAPING_MARK_STARTS) bits |= start;
    before_pos = bits;
    if (ops & LLE_SHAPING_MARK_POS) bits |= here;
    return bits;
}

// Lane a of group g of workgroup b serves agent a of environment b * (256 / G) + g.  LDS_TABLE: the workgroup's environments
// share one map and its cell table fits LDS_TABLE_MAX_BYTES.
template <int G, bool LDS_TABLE>
__global__ __launch_bounds__(SHAPING_THREADS) void shaping_kernel(ShapingParams p) {
    extern __shared__ uint32_t lds_table[];
    static_assert(G >= 1 && G <= 16 && (G & (G - 1)) == 0, "a power of two that divides the wave64");
    constexpr int ENVS_PER_BLOCK = SHAPING_THREADS / G;
    const int HW = p.H * p.W;
    const int64_t env0 = (int64_t)blockIdx.x * ENVS_PER_BLOCK;  // < n_envs: the grid is ceil(n_envs / ENVS_PER_BLOCK)
    if constexpr (LDS_TABLE) {
        const uint32_t* src = p.tables + (env0 / p.envs_per_map) * HW;
        for (int k = threadIdx.x; k < HW; k += SHAPING_THREADS) lds_table[k] = src[k];
        __syncthreads();
    }
    const int a = (int)(threadIdx.x % G);
    const int64_t env = env0 + (int64_t)(threadIdx.x / G);
    // (both exits are uniform over a lane group: the cross-lane sums below only read lanes of the own group)
    if (env >= p.n_envs) return;
    if (p.env_mask && p.env_mask[env] == 0) return;
    const int64_t map = env / p.envs_per_map;
    const bool agent = a < p.A;  // lanes A .. G-1 of a group carry no agent: they count as zero
    const bool has_s = p.n_pbrs > 0, has_e = p.E > 0;
    const bool was_reset = (p.flags & LLE_SHAPING_HONOUR_AUTO_RESET) && (p.evcount[env] & 0x80u);
    const uint32_t reset_ops = was_reset ? (uint32_t)(LLE_SHAPING_CLEAR | LLE_SHAPING_MARK_STARTS) : 0u;
    const uint32_t s_ops = has_s ? (p.strategy_ops | reset_ops) : 0u;
    const uint32_t e_ops = has_e ? (p.extras_ops | reset_ops) : 0u;

    uint32_t s = 0u, e = 0u, s_before = 0u, e_before = 0u;
    if (agent) {
        const int64_t idx = env * p.A + a;
        uint32_t start = 0u, here = 0u;
        if ((s_ops | e_ops) & LLE_SHAPING_MARK_STARTS) start = p.starts[map * START_PITCH + a];
        if ((s_ops | e_ops) & LLE_SHAPING_MARK_POS) {
            const uint8_t* q = p.pos + env * p.pos_stride + a * p.pos_agent_stride;
            const int i = q[0], j = q[1];
            if (i < p.H && j < p.W) {
                const int cell = i * p.W + j;
                if constexpr (LDS_TABLE) here = lds_table[cell];
                else here = p.tables[map * HW + cell];
            }
        }
        if (has_s) {
            s = apply_ops(p.reached_s[idx], s_ops, start, here, s_before);
            if (s_ops) p.reached_s[idx] = s;
        }
        if (has_e) {
            e = apply_ops(p.reached_e[idx], e_ops, start, here, e_before);
            if (e_ops) p.reached_e[idx] = e;
        }
    }

    if (p.reward_out) {
        // reached entries of this agent before and after the position mark, duplicates of pbrs_cols counted as often as listed;
        // both counts (<= 16 * 64) travel in one word
        uint32_t cnt = 0u;
        for (int k = 0; k < p.n_mult; k++) cnt += (uint32_t)__popc(s_before & p.mult[k]) | (uint32_t)__popc(s & p.mult[k]) << 16;
#pragma unroll
        for (int off = G >> 1; off >= 1; off >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, off, G);
        if (a == 0) {
            const int size = p.A * p.n_pbrs;  // _agents_pos_reached.size (reward_strategy.py:145,175)
            const double prev = (double)(size - (int)(cnt & 0xFFFFu)) * p.reward_value;
            const double cur = (double)(size - (int)(cnt >> 16)) * p.reward_value;
            const double scaled = p.gamma * prev;
            const float shaped = (float)(scaled - cur);
            if (p.reward_kind == 0) {
                p.reward_out[env] = p.base_reward[env] + shaped;
            } else {
                const float4 b = *reinterpret_cast<const float4*>(p.base_reward + 4 * env);
                float* o = p.reward_out + 5 * env;
                o[0] = b.x; o[1] = b.y; o[2] = b.z; o[3] = b.w; o[4] = shaped;
            }
        }
    }
    if (p.extras_out && agent) {
        float* o = p.extras_out + (env * p.A + a) * p.E;
        for (int c = 0; c < p.E; c++) o[c] = ((e >> p.ecols[c]) & 1u) ? 1.0f : 0.0f;
    }
}

#define LLE_SHAPING_INSTANTIATE(G)                                    \
    template __global__ void shaping_kernel<G, false>(ShapingParams); \
    template __global__ void shaping_kernel<G, true>(ShapingParams);
LLE_SHAPING_INSTANTIATE(1)
LLE_SHAPING_INSTANTIATE(2)
LLE_SHAPING_INSTANTIATE(4)
LLE_SHAPING_INSTANTIATE(8)
LLE_SHAPING_INSTANTIATE(16)
#undef LLE_SHAPING_INSTANTIATE

}  // namespace lle

// ================================================================================================ host side
using lle::ShapingParams;
using namespace lle_abi_host;

namespace {

std::atomic<uint32_t> g_launched{0};
// bit 2 * log2(G) + LDS_TABLE
const char* const KERNEL_NAMES[10] = {"shaping_kernel<1,false>", "shaping_kernel<1,true>",  "shaping_kernel<2,false>",  "shaping_kernel<2,true>",
                                      "shaping_kernel<4,false>", "shaping_kernel<4,true>",  "shaping_kernel<8,false>",  "shaping_kernel<8,true>",
                                      "shaping_kernel<16,false>", "shaping_kernel<16,true>"};

struct MapTables {
    int32_t H = 0, W = 0, A = 0, n_sources = 0;
    std::vector<uint32_t> cells;   // [H * W]
    std::vector<uint32_t> starts;  // [START_PITCH]: the cell mask at every agent's start
};

// The cell table of `map` (lle_shaping_cell_masks) and the masks at its start cells; `err` set on failure.
bool build_map(const lle_map* map, MapTables& mt, std::string& err) {
    lle_map_info info{};
    if (lle_map_get_info(map, &info) != LLE_OK) { err = "lle_map_get_info failed"; return false; }
    mt.H = info.height; mt.W = info.width; mt.A = info.n_agents; mt.n_sources = info.n_sources;
    if (mt.A > LLE_MAX_AGENTS || mt.n_sources > 32) { err = "map beyond the limits of the shaping kernel"; return false; }
    mt.cells.assign((size_t)mt.H * mt.W, 0u);
    // World.lasers (world.rs:159-172): the outer layer of a cell and the one directly below it -- what lle_map_laser_tiles lists
    std::vector<lle_laser_tile> tiles((size_t)std::max(0, lle_map_laser_tiles(map, nullptr, 0)));
    lle_map_laser_tiles(map, tiles.data(), (int)tiles.size());
    for (const auto& t : tiles) {
        if (t.i < 0 || t.i >= mt.H || t.j < 0 || t.j >= mt.W || t.laser_id < 0 || t.laser_id >= 32) { err = "laser tile out of range"; return false; }
        mt.cells[(size_t)t.i * mt.W + t.j] |= 1u << t.laser_id;
    }
    std::vector<int32_t> ij((size_t)2 * std::max(0, lle_map_positions(map, LLE_POS_START, nullptr, 0)));
    lle_map_positions(map, LLE_POS_START, ij.data(), (int)ij.size() / 2);
    if ((int)ij.size() != 2 * mt.A) { err = "one start cell per agent is required"; return false; }
    mt.starts.assign(lle::START_PITCH, 0u);
    for (int a = 0; a < mt.A; a++) {
        const int i = ij[(size_t)2 * a], j = ij[(size_t)2 * a + 1];
        if (i < 0 || i >= mt.H || j < 0 || j >= mt.W) { err = "start cell out of range"; return false; }
        mt.starts[(size_t)a] = mt.cells[(size_t)i * mt.W + j];
    }
    return true;
}

}  // namespace

struct lle_shaping {
    int device = 0;
    int n_maps = 0;
    int64_t n_envs = 0;
    std::vector<MapTables> maps;
    uint32_t* d_tables = nullptr;
    uint32_t* d_starts = nullptr;
    uint8_t* d_ecols = nullptr;
    uint32_t* d_reached = nullptr;  // both arrays: [2][n][A]
    bool lds_table = false;
    int log2_g = 0;
    ShapingParams p{};
};

extern "C" {

const char* lle_shaping_last_error(void) { return g_error.c_str(); }

int lle_shaping_cell_masks(const lle_map* map, uint32_t* out, int cap) {
    if (!map) return fail(LLE_ERR_NULL, "NULL map");
    MapTables mt;
    std::string err;
    if (!build_map(map, mt, err)) return fail(LLE_ERR_ARG, err);
    if (out)
        for (int k = 0; k < std::min(cap, (int)mt.cells.size()); k++) out[k] = mt.cells[(size_t)k];
    return (int)mt.cells.size();
}

void lle_shaping_free(lle_shaping* s) {
    if (!s) return;
    DeviceGuard g(s->device);
    (void)hipFree(s->d_tables);
    (void)hipFree(s->d_starts);
    (void)hipFree(s->d_ecols);
    (void)hipFree(s->d_reached);
    delete s;
}

lle_shaping* lle_shaping_create(lle_batch* batch, const lle_map* const* maps, int n_maps, const lle_shaping_config* config, void* stream) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) {
        (void)hipGetLastError();
        fail(LLE_ERR_NO_DEVICE, "no HIP device: reward shaping runs on the GPU only (there is no CPU fallback)");
        return nullptr;
    }
    if (!batch || !maps || !config) {
        fail(LLE_ERR_NULL, "NULL batch, maps or config");
        return nullptr;
    }
    if (config->struct_bytes != sizeof(lle_shaping_config)) {
        fail(LLE_ERR_ARG, "lle_shaping_config.struct_bytes is not sizeof(lle_shaping_config)");
        return nullptr;
    }
    if (n_maps != lle_batch_n_maps(batch) || n_maps <= 0) {
        fail(LLE_ERR_ARG, "n_maps must be lle_batch_n_maps(batch)");
        return nullptr;
    }
    if (config->n_pbrs_cols < 0 || config->n_pbrs_cols > LLE_SHAPING_MAX_COLS || config->n_extras_cols < 0 ||
        config->n_extras_cols > LLE_SHAPING_MAX_COLS || (config->n_pbrs_cols > 0 && !config->pbrs_cols) ||
        (config->n_extras_cols > 0 && !config->extras_cols)) {
        fail(LLE_ERR_ARG, "pbrs_cols / extras_cols: 0 .. LLE_SHAPING_MAX_COLS entries each");
        return nullptr;
    }
    lle_buffer_desc pos{}, evcount{};
    if (lle_batch_get_buffer(batch, LLE_BUF_POS, &pos) || lle_batch_get_buffer(batch, LLE_BUF_EVCOUNT, &evcount)) {
        fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
        return nullptr;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, pos.ptr) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "the batch's buffers are not device memory");
        return nullptr;
    }
    auto* s = new lle_shaping();
    s->device = attr.device;
    s->n_maps = n_maps;
    s->n_envs = lle_batch_n_envs(batch);
    std::string err;
    s->maps.resize((size_t)n_maps);
    for (int m = 0; m < n_maps; m++) {
        if (!maps[m] || !build_map(maps[m], s->maps[(size_t)m], err)) {
            fail(LLE_ERR_ARG, maps[m] ? err : "NULL map");
            delete s;
            return nullptr;
        }
        const MapTables& a = s->maps[0], &b = s->maps[(size_t)m];
        if (a.H != b.H || a.W != b.W || a.A != b.A || a.n_sources != b.n_sources) {
            fail(LLE_ERR_ARG, "the maps of a batch share height, width, agents and sources");
            delete s;
            return nullptr;
        }
    }
    const MapTables& m0 = s->maps[0];
    if (s->n_envs <= 0 || s->n_envs % n_maps != 0 || m0.A < 1) {
        fail(LLE_ERR_ARG, "n_envs must be a positive multiple of n_maps");
        delete s;
        return nullptr;
    }
    ShapingParams& p = s->p;
    uint32_t times[32] = {0};
    for (int k = 0; k < config->n_pbrs_cols; k++) {
        const int l = config->pbrs_cols[k];
        if (l < 0 || l >= m0.n_sources) {
            fail(LLE_ERR_ARG, "pbrs_cols: not a laser_id of the map");
            delete s;
            return nullptr;
        }
        if (++times[l] > LLE_SHAPING_MAX_REPEATS) {
            fail(LLE_ERR_UNSUPPORTED, "pbrs_cols: a source listed more than LLE_SHAPING_MAX_REPEATS times");
            delete s;
            return nullptr;
        }
    }
    p.n_mult = 0;
    for (int k = 0; k < LLE_SHAPING_MAX_REPEATS; k++) {
        p.mult[k] = 0u;
        for (int l = 0; l < 32; l++)
            if (times[l] > (uint32_t)k) p.mult[k] |= 1u << l;
        if (p.mult[k]) p.n_mult = k + 1;
    }
    std::vector<uint8_t> ecols((size_t)std::max(1, config->n_extras_cols), 0);
    for (int k = 0; k < config->n_extras_cols; k++) {
        const int l = config->extras_cols[k];
        if (l < 0 || l >= m0.n_sources) {
            fail(LLE_ERR_ARG, "extras_cols: not a laser_id of the map");
            delete s;
            return nullptr;
        }
        ecols[(size_t)k] = (uint8_t)l;
    }

    DeviceGuard g(s->device);
    const size_t HW = (size_t)m0.H * m0.W;
    std::vector<uint32_t> tables, starts;
    for (const auto& m : s->maps) {
        tables.insert(tables.end(), m.cells.begin(), m.cells.end());
        starts.insert(starts.end(), m.starts.begin(), m.starts.end());
    }
    const size_t reached_bytes = (size_t)2 * (size_t)s->n_envs * (size_t)m0.A * 4;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMalloc(&s->d_tables, std::max<size_t>(4, tables.size() * 4)) != hipSuccess || hipMalloc(&s->d_starts, starts.size() * 4) != hipSuccess ||
        hipMalloc(&s->d_ecols, ecols.size()) != hipSuccess || hipMalloc(&s->d_reached, reached_bytes) != hipSuccess ||
        hipMemcpyAsync(s->d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s->d_starts, starts.data(), starts.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s->d_ecols, ecols.data(), ecols.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(s->d_reached, 0, reached_bytes, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating or uploading the shaping tables failed");
        lle_shaping_free(s);
        return nullptr;
    }
    p.tables = s->d_tables;
    p.starts = s->d_starts;
    p.ecols = s->d_ecols;
    p.pos = static_cast<const uint8_t*>(pos.ptr);
    p.pos_stride = pos.stride[0];
    p.pos_agent_stride = pos.ndim > 2 ? pos.stride[1] : 2;
    p.evcount = static_cast<const uint8_t*>(evcount.ptr);
    p.reached_s = s->d_reached;
    p.reached_e = s->d_reached + (size_t)s->n_envs * (size_t)m0.A;
    p.n_envs = s->n_envs;
    p.envs_per_map = s->n_envs / n_maps;
    p.gamma = config->gamma;
    p.reward_value = config->reward_value;
    p.H = m0.H;
    p.W = m0.W;
    p.A = m0.A;
    p.E = config->n_extras_cols;
    p.n_pbrs = config->n_pbrs_cols;
    int G = 1;
    while (G < m0.A) G <<= 1, s->log2_g++;
    // the table in LDS: it fits, and every workgroup's environments (256 / G consecutive ones) belong to one map
    const int64_t envs_per_block = lle::SHAPING_THREADS / G;
    s->lds_table = HW * 4 <= (size_t)lle::LDS_TABLE_MAX_BYTES && (n_maps == 1 || p.envs_per_map % envs_per_block == 0);
    g_error.clear();
    return s;
}

int lle_shaping_update_map(lle_shaping* s, int map_index, const lle_map* map, void* stream) {
    (void)stream;
    if (!s || !map) return fail(LLE_ERR_NULL, "NULL handle or map");
    if (map_index < 0 || map_index >= s->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    MapTables mt;
    std::string err;
    if (!build_map(map, mt, err)) return fail(LLE_ERR_ARG, err);
    const MapTables& old = s->maps[(size_t)map_index];
    if (mt.H != old.H || mt.W != old.W || mt.A != old.A || mt.n_sources != old.n_sources || mt.cells != old.cells || mt.starts != old.starts)
        return fail(LLE_ERR_ARG, "not a recompilation of the handle's map (the beams or the starts moved)");
    return LLE_OK;
}

void* lle_shaping_reached(lle_shaping* s, int which) {
    if (!s || which < 0 || which > 1) {
        fail(LLE_ERR_ARG, "NULL handle or `which` not 0 / 1");
        return nullptr;
    }
    return which == 0 ? s->p.reached_s : s->p.reached_e;
}

int lle_shaping_update(lle_shaping* s, const lle_shaping_update_args* args, void* stream) {
    if (!s || !args) return fail(LLE_ERR_NULL, "NULL handle or arguments");
    if (args->struct_bytes != sizeof(lle_shaping_update_args)) return fail(LLE_ERR_ARG, "lle_shaping_update_args.struct_bytes is not sizeof(lle_shaping_update_args)");
    const uint32_t all_ops = LLE_SHAPING_CLEAR | LLE_SHAPING_MARK_STARTS | LLE_SHAPING_MARK_POS;
    if ((args->strategy_ops & ~all_ops) || (args->extras_ops & ~all_ops) || (args->flags & ~(uint32_t)LLE_SHAPING_HONOUR_AUTO_RESET))
        return fail(LLE_ERR_ARG, "unknown operation or flag");
    if (args->reward_kind != 0 && args->reward_kind != 1) return fail(LLE_ERR_ARG, "reward_kind is 0 or 1");
    if (args->reward_out && !args->base_reward) return fail(LLE_ERR_NULL, "reward_out needs base_reward");
    if (args->reward_out && args->reward_kind == 1 && reinterpret_cast<uintptr_t>(args->base_reward) % 16 != 0)
        return fail(LLE_ERR_ARG, "base_reward [n][4] must be 16-byte aligned");
    if (args->extras_out && s->p.E == 0) return fail(LLE_ERR_ARG, "extras_out on a handle created without extras_cols");
    ShapingParams p = s->p;
    p.strategy_ops = args->strategy_ops;
    p.extras_ops = args->extras_ops;
    p.flags = args->flags;
    p.reward_kind = args->reward_kind;
    p.env_mask = args->env_mask;
    p.base_reward = args->base_reward;
    p.reward_out = args->reward_out;
    p.extras_out = args->extras_out;
    const int G = 1 << s->log2_g;
    const int64_t envs_per_block = lle::SHAPING_THREADS / G;
    const int64_t blocks = (p.n_envs + envs_per_block - 1) / envs_per_block;
    if (blocks > 0x7FFFFFFF) return fail(LLE_ERR_ARG, "too many environments for one launch");
    const size_t lds = s->lds_table ? (size_t)p.H * p.W * 4 : 0;
    DeviceGuard g(s->device);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((uint32_t)blocks), block(lle::SHAPING_THREADS);
#define LLE_SHAPING_LAUNCH(GG)                                                                                 \
    case GG:                                                                                                   \
        if (s->lds_table) hipLaunchKernelGGL((lle::shaping_kernel<GG, true>), grid, block, lds, st, p);        \
        else hipLaunchKernelGGL((lle::shaping_kernel<GG, false>), grid, block, 0, st, p);                      \
        break;
    switch (G) {
        LLE_SHAPING_LAUNCH(1)
        LLE_SHAPING_LAUNCH(2)
        LLE_SHAPING_LAUNCH(4)
        LLE_SHAPING_LAUNCH(8)
        LLE_SHAPING_LAUNCH(16)
        default: return fail(LLE_ERR_UNSUPPORTED, "more agents than the shaping kernel serves");
    }
#undef LLE_SHAPING_LAUNCH
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "shaping launch failed");
    g_launched.fetch_or(1u << (2 * s->log2_g + (s->lds_table ? 1 : 0)));
    return LLE_OK;
}

size_t lle_shaping_debug_launched(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 10, g_launched.load(), buf, cap); }
size_t lle_shaping_debug_compiled(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 10, 0x3FFu, buf, cap); }

}  // extern "C"
