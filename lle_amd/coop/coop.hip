// coop.hip -- liblle_coop.so: cooperation edges and episode profiles of an lle_batch (C ABI: include/lle_coop.h; INTEGRATION.md
// section 13).
//
// detect_dependencies (python/lle/characterization/plan/analyser.py:31-60) and the flattened degree profile of
// TemporalCooperationGraph (graph.py:92-151) of the reference for many environments in one launch.  The library reads a batch only
// through the public ABI of include/lle_hip.h (lle_batch_get_buffer, lle_map_*), so liblle_hip.so keeps its kernels.
//
// State: three arrays u32 [n][A] (row h = beneficiaries of helper h: this state's, the running episode's, the last finished
// episode's) and two profiles u8 [n][8].  A cell -> u32 table per map says which sources own a laser tile on the cell (World.lasers:
// the outer two layers only); an agent's word m_a is one table lookup, zero when it is not the cell's occupant.
// Kernel: one lane per (environment, agent) in groups of G = next power of two >= A lanes, the lane-group shape of the step
// kernels; lane a reads the other lanes' words with cross-lane reads inside the wave64 and sets bit b where lane b stands on a
// source lane a is blocking; the profile is bit counting over the group's rows, again by cross-lane reads (no LDS beyond the staged
// table, no atomics); the group's first lane writes the profiles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_coop.h"
#include "tracker_core.hpp"

namespace eo = lle_episode_ops;

namespace lle {

constexpr int COOP_THREADS = 256;
constexpr int START_PITCH = 32;              // per map: [0, 16) start edges of every agent, [16] non-zero when there is any
constexpr int COLOUR_PITCH = 32;             // per map: [0, 16) sources of every agent's colour, [16] the enabled sources
constexpr int LDS_TABLE_MAX_BYTES = 16384;   // a cell table up to 64 x 64 lives in LDS; larger ones stay in global memory

struct CoopParams {
    const uint32_t* tables;    // [n_maps][H * W] cell masks
    const uint32_t* starts;    // [n_maps][START_PITCH]
    const uint32_t* colours;   // [n_maps][COLOUR_PITCH]
    const uint8_t* pos;        // LLE_BUF_POS
    const uint64_t* bits;      // LLE_BUF_BITS
    const uint8_t* evcount;    // LLE_BUF_EVCOUNT
    const uint8_t* src_colour; // LLE_BUF_SRC_COLOUR
    const uint32_t* src_enabled;  // LLE_BUF_SRC_ENABLED
    uint32_t* step_edges;      // [n][A]
    uint32_t* episode_edges;   // [n][A]
    uint32_t* last_edges;      // [n][A]
    uint64_t* episode_profile; // [n] (8 bytes each)
    uint64_t* last_profile;    // [n]
    const uint8_t* env_mask;
    int64_t pos_stride, pos_agent_stride, colour_stride;  // elements
    int64_t n_envs, envs_per_map;
    int32_t H, W, A, L;
    uint32_t ops, flags;
    uint8_t first_word[LLE_MAX_SOURCES];  // first beam word of every source: its entry of an LLE_BUF_SRC_COLOUR record
};

// OR over the G lanes of the group.
template <int G>
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
#pragma unroll
    for (int off = G >> 1; off >= 1; off >>= 1) v |= (uint32_t)__shfl_xor((int)v, off, G);
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
#pragma unroll
    for (int off = G >> 1; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, G);
    return v;
}
template <int G>
__device__ __forceinline__ uint32_t group_max(uint32_t v) {
#pragma unroll
    for (int off = G >> 1; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, G));
    return v;
}

// Bytes 0-4 of the profile of the group's rows (`row` of lane a = beneficiaries of helper a, bits < G only), the same value in every lane.
template <int G>
__device__ __forceinline__ uint64_t profile_of(uint32_t row, int a) {
    const uint32_t n_edges = group_sum<G>((uint32_t)__popc(row));
    const uint32_t helped = group_or<G>(row);                    // the agents that are a beneficiary of any edge
    const uint32_t helpers = group_or<G>(row ? 1u << a : 0u);
    const uint32_t max_out = group_max<G>((uint32_t)__popc(row));
    uint32_t in = 0u;  // lane a as a beneficiary: the helpers that have its bit
#pragma unroll
    for (int h = 0; h < G; h++) in += ((uint32_t)__shfl((int)row, h, G) >> a) & 1u;
    const uint32_t max_in = group_max<G>(in);
    const uint32_t asym = group_sum<G>(((helped >> a) & 1u) ? 0u : (uint32_t)__popc(row));
    return (uint64_t)(n_edges & 255u) | (uint64_t)__popc(helped | helpers) << 8 | (uint64_t)max_in << 16 | (uint64_t)max_out << 24 | (uint64_t)(asym & 255u) << 32;
}

// Lane a of group g of workgroup b serves agent a of environment b * (256 / G) + g.  LDS_TABLE: the workgroup's environments
// share one map and its cell table fits LDS_TABLE_MAX_BYTES.
template <int G, bool LDS_TABLE>
__global__ __launch_bounds__(COOP_THREADS) void coop_kernel(CoopParams p) {
    extern __shared__ uint32_t lds_table[];
    static_assert(G >= 1 && G <= 16 && (G & (G - 1)) == 0, "a power of two that divides the wave64");
    constexpr int ENVS_PER_BLOCK = COOP_THREADS / G;
    const int HW = p.H * p.W;
    const int64_t env0 = (int64_t)blockIdx.x * ENVS_PER_BLOCK;  // < n_envs: the grid is ceil(n_envs / ENVS_PER_BLOCK)
    if constexpr (LDS_TABLE) {
        const uint32_t* src = p.tables + (env0 / p.envs_per_map) * HW;
        for (int k = threadIdx.x; k < HW; k += COOP_THREADS) lds_table[k] = src[k];
        __syncthreads();
    }
    const int a = (int)(threadIdx.x % G);
    const int64_t env = env0 + (int64_t)(threadIdx.x / G);
    // (every exit and every branch on `ops` below is uniform over a lane group: the cross-lane reads only touch lanes of the own group)
    if (env >= p.n_envs) return;
    if (p.env_mask && p.env_mask[env] == 0) return;
    const int64_t map = env / p.envs_per_map;
    const bool agent = a < p.A;  // lanes A .. G-1 of a group carry no agent: their words are zero
    const uint32_t reset_ops = eo::reset_ops(p.flags, p.evcount + env);
    if ((p.ops | reset_ops) == 0u) return;
    const int64_t idx = env * p.A + a;

    // ---- the edges of the state in the buffers
    uint32_t step = 0u;
    if (p.ops & LLE_COOP_MARK_POS) {
        uint32_t m = 0u, own = 0u;
        if (agent) {
            const uint64_t bits = p.bits[env];
            const uint8_t* q = p.pos + env * p.pos_stride + a * p.pos_agent_stride;
            const int i = q[0], j = q[1];
            if (((bits >> (32 + a)) & 1u) && i < p.H && j < p.W) {
                const int cell = i * p.W + j;
                if constexpr (LDS_TABLE) m = lds_table[cell];
                else m = p.tables[map * HW + cell];
            }
            if (m) {  // the sources of this agent's colour that are enabled: the ones it blocks where it stands on them
                uint32_t mine, enabled;
                if (p.flags & LLE_COOP_ENV_SOURCES) {
                    const uint8_t* col = p.src_colour + env * p.colour_stride;
                    mine = 0u;
                    for (int l = 0; l < p.L; l++) mine |= (col[p.first_word[l]] == a ? 1u : 0u) << l;
                    enabled = p.src_enabled[env];
                } else {
                    mine = p.colours[map * COLOUR_PITCH + a];
                    enabled = p.colours[map * COLOUR_PITCH + 16];
                }
                own = m & mine & enabled;
            }
        }
#pragma unroll
        for (int b = 0; b < G; b++) {
            const uint32_t mb = (uint32_t)__shfl((int)m, b, G);
            if ((mb & own) && b != a) step |= 1u << b;
        }
    }

    // ---- the operations: the auto-reset's first, then the caller's whole (no SKIP_REFUSED here: stages 1 and 2 of episode_ops.hpp as one)
    uint32_t episode = 0u, last = 0u;
    uint32_t count = 0u, last_count = 0u;
    bool finished = false;
    if (agent) episode = p.episode_edges[idx];
    count = (uint32_t)(p.episode_profile[env] >> 40) & 255u;
    uint32_t start = 0u, start_any = 0u;
    if ((p.ops | reset_ops) & LLE_COOP_MARK_STARTS) {
        if (agent) start = p.starts[map * START_PITCH + a];
        start_any = p.starts[map * START_PITCH + 16];
    }
    const uint32_t step_any = group_or<G>(step);
#pragma unroll
    for (int phase = 0; phase < 2; phase++) {
        const uint32_t ops = phase == 0 ? eo::stage_ops(reset_ops, p.ops, 0) : eo::stage_ops(reset_ops, p.ops, 1) | eo::stage_ops(reset_ops, p.ops, 2);
        if (ops & LLE_COOP_FINISH) { last = episode; last_count = count; finished = true; }
        if (ops & LLE_COOP_CLEAR) { episode = 0u; count = 0u; }
        if (ops & LLE_COOP_MARK_STARTS) { episode |= start; count = min(255u, count + (start_any ? 1u : 0u)); }
        if (ops & LLE_COOP_MARK_POS) { episode |= step; count = min(255u, count + (step_any ? 1u : 0u)); }
    }

    if (agent) {
        if (p.ops & LLE_COOP_MARK_POS) p.step_edges[idx] = step;
        p.episode_edges[idx] = episode;
        if (finished) p.last_edges[idx] = last;
    }
    const uint64_t valid = (uint64_t)1 << 56;
    const uint64_t prof = profile_of<G>(episode, a) | (uint64_t)count << 40 | valid;
    if (a == 0) p.episode_profile[env] = prof;
    if (finished) {
        const uint64_t lprof = profile_of<G>(last, a) | (uint64_t)last_count << 40 | valid;
        if (a == 0) p.last_profile[env] = lprof;
    }
}

#define LLE_COOP_INSTANTIATE(G)                                 \
    template __global__ void coop_kernel<G, false>(CoopParams); \
    template __global__ void coop_kernel<G, true>(CoopParams);
LLE_COOP_INSTANTIATE(1)
LLE_COOP_INSTANTIATE(2)
LLE_COOP_INSTANTIATE(4)
LLE_COOP_INSTANTIATE(8)
LLE_COOP_INSTANTIATE(16)
#undef LLE_COOP_INSTANTIATE

}  // namespace lle

// ================================================================================================ host side
using lle::CoopParams;
using namespace lle_abi_host;

static_assert(LLE_COOP_FINISH == eo::FINISH && LLE_COOP_CLEAR == eo::CLEAR && LLE_COOP_MARK_STARTS == eo::MARK_STARTS && LLE_COOP_MARK_POS == eo::MARK_POS &&
                  LLE_COOP_HONOUR_AUTO_RESET == eo::HONOUR_AUTO_RESET,
              "the shared decode reads this header's values");

namespace {

std::atomic<uint32_t> g_launched{0};
// bit 2 * log2(G) + LDS_TABLE
const char* const KERNEL_NAMES[10] = {"coop_kernel<1,false>", "coop_kernel<1,true>",  "coop_kernel<2,false>",  "coop_kernel<2,true>",
                                      "coop_kernel<4,false>", "coop_kernel<4,true>",  "coop_kernel<8,false>",  "coop_kernel<8,true>",
                                      "coop_kernel<16,false>", "coop_kernel<16,true>"};

struct MapTables {
    int32_t H = 0, W = 0, A = 0, n_sources = 0;
    std::vector<uint32_t> cells;     // [H * W]
    std::vector<int32_t> start_ij;   // [2 A]
    std::vector<uint32_t> colours;   // [COLOUR_PITCH]
    std::vector<uint32_t> starts;    // [START_PITCH]: filled by start_edges()
    std::vector<uint8_t> first_word; // [n_sources]
    bool start_on_beam = false;      // a start cell is a laser cell
};

// The static tables of `map`; `err` set on failure.
bool build_map(const lle_map* map, MapTables& mt, std::string& err) {
    lle_map_info info{};
    if (lle_map_get_info(map, &info) != LLE_OK) { err = "lle_map_get_info failed"; return false; }
    mt.H = info.height; mt.W = info.width; mt.A = info.n_agents; mt.n_sources = info.n_sources;
    if (mt.A > LLE_MAX_AGENTS || mt.A > 16) { err = "more than 16 agents: beyond the limits of the coop kernel"; return false; }
    if (mt.n_sources > 32) { err = "more than 32 sources: beyond the limits of the coop kernel"; return false; }
    mt.cells.assign((size_t)mt.H * mt.W, 0u);
    // World.lasers (world.rs:159-172): the outer layer of a cell and the one directly below it -- what lle_map_laser_tiles lists
    std::vector<lle_laser_tile> tiles((size_t)std::max(0, lle_map_laser_tiles(map, nullptr, 0)));
    lle_map_laser_tiles(map, tiles.data(), (int)tiles.size());
    for (const auto& t : tiles) {
        if (t.i < 0 || t.i >= mt.H || t.j < 0 || t.j >= mt.W || t.laser_id < 0 || t.laser_id >= 32) { err = "laser tile out of range"; return false; }
        mt.cells[(size_t)t.i * mt.W + t.j] |= 1u << t.laser_id;
    }
    mt.start_ij.assign((size_t)2 * std::max(0, lle_map_positions(map, LLE_POS_START, nullptr, 0)), 0);
    lle_map_positions(map, LLE_POS_START, mt.start_ij.data(), (int)mt.start_ij.size() / 2);
    if ((int)mt.start_ij.size() != 2 * mt.A) { err = "one start cell per agent is required"; return false; }
    mt.start_on_beam = false;
    for (int a = 0; a < mt.A; a++) {
        const int i = mt.start_ij[(size_t)2 * a], j = mt.start_ij[(size_t)2 * a + 1];
        if (i < 0 || i >= mt.H || j < 0 || j >= mt.W) { err = "start cell out of range"; return false; }
        if (mt.cells[(size_t)i * mt.W + j]) mt.start_on_beam = true;
    }
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    if ((int)src.size() != mt.n_sources) { err = "lle_map_sources disagrees with lle_map_info"; return false; }
    mt.colours.assign(lle::COLOUR_PITCH, 0u);
    mt.first_word.assign(src.size(), 0);
    size_t w = 0;
    for (size_t l = 0; l < src.size(); l++) {  // lle_map_info.n_beam_words: ceil(length / 32) words per source, at least one
        if (w > 255) { err = "beam words out of range"; return false; }
        mt.first_word[l] = (uint8_t)w;
        w += (size_t)std::max(1, (src[l].length + 31) / 32);
        if (src[l].agent_id >= 0 && src[l].agent_id < mt.A) mt.colours[(size_t)src[l].agent_id] |= 1u << l;  // a colour >= n_agents never blocks
        if (src[l].enabled) mt.colours[16] |= 1u << l;
    }
    mt.starts.assign(lle::START_PITCH, 0u);
    return true;
}

// One launch of coop_kernel<1 << log2_g, lds_table> over p.n_envs environments.
int launch(const CoopParams& p, int log2_g, bool lds_table, hipStream_t st) {
    const int G = 1 << log2_g;
    const int64_t envs_per_block = lle::COOP_THREADS / G;
    const int64_t blocks = (p.n_envs + envs_per_block - 1) / envs_per_block;
    if (blocks <= 0 || blocks > 0x7FFFFFFF) return fail(LLE_ERR_ARG, "too many environments for one launch");
    const size_t lds = lds_table ? (size_t)p.H * p.W * 4 : 0;
    const dim3 grid((uint32_t)blocks), block(lle::COOP_THREADS);
#define LLE_COOP_LAUNCH(GG)                                                                            \
    case GG:                                                                                           \
        if (lds_table) hipLaunchKernelGGL((lle::coop_kernel<GG, true>), grid, block, lds, st, p);      \
        else hipLaunchKernelGGL((lle::coop_kernel<GG, false>), grid, block, 0, st, p);                 \
        break;
    switch (G) {
        LLE_COOP_LAUNCH(1)
        LLE_COOP_LAUNCH(2)
        LLE_COOP_LAUNCH(4)
        LLE_COOP_LAUNCH(8)
        LLE_COOP_LAUNCH(16)
        default: return fail(LLE_ERR_UNSUPPORTED, "more agents than the coop kernel serves");
    }
#undef LLE_COOP_LAUNCH
    if (hipGetLastError() != hipSuccess) return fail(LLE_ERR_HIP, "coop launch failed");
    g_launched.fetch_or(1u << (2 * log2_g + (lds_table ? 1 : 0)));
    return LLE_OK;
}

}  // namespace

struct lle_coop {
    int device = 0;
    int n_maps = 0;
    int64_t n_envs = 0;
    std::vector<MapTables> maps;
    uint32_t* d_tables = nullptr;
    uint32_t* d_starts = nullptr;
    uint32_t* d_colours = nullptr;
    uint8_t* d_state = nullptr;   // the five arrays between guard bytes
    uint8_t* d_scratch = nullptr; // one environment's arrays, for the start edges
    bool lds_table = false;
    bool any_start_on_beam = false;
    int log2_g = 0;
    CoopParams p{};
};

namespace {

// The start edges of map `m`: the coop kernel on a freshly reset one-environment batch of it (synchronises `st`).
int start_edges(lle_coop* c, int m, const lle_map* map, hipStream_t st) {
    MapTables& mt = c->maps[(size_t)m];
    mt.starts.assign(lle::START_PITCH, 0u);
    if (!mt.start_on_beam) return LLE_OK;  // nobody stands on a laser tile after a reset: no edge whatever the colours
    lle_batch* tmp = lle_batch_create(map, 1, c->device, nullptr, 0, st);
    if (!tmp) return fail(LLE_ERR_HIP, std::string("the one-environment batch for the start edges: ") + lle_last_error());
    lle_buffer_desc pos{}, bits{}, evcount{};
    int rc = LLE_OK;
    if (lle_batch_get_buffer(tmp, LLE_BUF_POS, &pos) || lle_batch_get_buffer(tmp, LLE_BUF_BITS, &bits) || lle_batch_get_buffer(tmp, LLE_BUF_EVCOUNT, &evcount)) {
        rc = fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
    } else {
        const size_t HW = (size_t)mt.H * mt.W, A = (size_t)mt.A;
        CoopParams q = c->p;
        q.tables = c->d_tables + (size_t)m * HW;
        q.starts = c->d_starts + (size_t)m * lle::START_PITCH;
        q.colours = c->d_colours + (size_t)m * lle::COLOUR_PITCH;
        q.pos = static_cast<const uint8_t*>(pos.ptr);
        q.pos_stride = pos.stride[0];
        q.pos_agent_stride = pos.ndim > 2 ? pos.stride[1] : 2;
        q.bits = static_cast<const uint64_t*>(bits.ptr);
        q.evcount = static_cast<const uint8_t*>(evcount.ptr);
        q.src_colour = nullptr;
        q.src_enabled = nullptr;
        uint32_t* words = reinterpret_cast<uint32_t*>(c->d_scratch);
        q.step_edges = words;
        q.episode_edges = words + 16;
        q.last_edges = words + 32;
        q.episode_profile = reinterpret_cast<uint64_t*>(words + 48);
        q.last_profile = q.episode_profile + 1;
        q.env_mask = nullptr;
        q.n_envs = 1;
        q.envs_per_map = 1;
        q.ops = LLE_COOP_CLEAR | LLE_COOP_MARK_POS;
        q.flags = 0;
        // (the colour table of this map must be on the device already)
        rc = launch(q, c->log2_g, c->lds_table, st);
        if (rc == LLE_OK && (hipMemcpyAsync(mt.starts.data(), words, A * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) {
            (void)hipGetLastError();
            rc = fail(LLE_ERR_HIP, "reading the start edges back failed");
        }
        uint32_t any = 0u;
        for (size_t a = 0; a < A; a++) any |= mt.starts[a];
        mt.starts[16] = any;
    }
    (void)hipStreamSynchronize(st);
    lle_batch_free(tmp);
    return rc;
}

// Colour and start tables of map `m` to the device (synchronises `st`).
int upload_map(lle_coop* c, int m, const lle_map* map, hipStream_t st) {
    MapTables& mt = c->maps[(size_t)m];
    if (hipMemcpyAsync(c->d_colours + (size_t)m * lle::COLOUR_PITCH, mt.colours.data(), lle::COLOUR_PITCH * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "uploading the colour table failed");
    }
    const int rc = start_edges(c, m, map, st);
    if (rc != LLE_OK) return rc;
    if (hipMemcpyAsync(c->d_starts + (size_t)m * lle::START_PITCH, mt.starts.data(), lle::START_PITCH * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "uploading the start edges failed");
    }
    return LLE_OK;
}

}  // namespace

extern "C" {

const char* lle_coop_last_error(void) { return g_error.c_str(); }

int lle_coop_cell_masks(const lle_map* map, uint32_t* out, int cap) {
    if (!map) return fail(LLE_ERR_NULL, "NULL map");
    MapTables mt;
    std::string err;
    if (!build_map(map, mt, err)) return fail(LLE_ERR_ARG, err);
    if (out)
        for (int k = 0; k < std::min(cap, (int)mt.cells.size()); k++) out[k] = mt.cells[(size_t)k];
    return (int)mt.cells.size();
}

void lle_coop_free(lle_coop* c) {
    if (!c) return;
    DeviceGuard g(c->device);
    (void)hipFree(c->d_tables);
    (void)hipFree(c->d_starts);
    (void)hipFree(c->d_colours);
    (void)hipFree(c->d_state);
    (void)hipFree(c->d_scratch);
    delete c;
}

lle_coop* lle_coop_create(lle_batch* batch, const lle_map* const* maps, int n_maps, void* stream) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) {
        (void)hipGetLastError();
        fail(LLE_ERR_NO_DEVICE, "no HIP device: the cooperation tracker runs on the GPU only (there is no CPU fallback)");
        return nullptr;
    }
    if (!batch || !maps) {
        fail(LLE_ERR_NULL, "NULL batch or maps");
        return nullptr;
    }
    if (n_maps != lle_batch_n_maps(batch) || n_maps <= 0) {
        fail(LLE_ERR_ARG, "n_maps must be lle_batch_n_maps(batch)");
        return nullptr;
    }
    lle_buffer_desc pos{}, bits{}, evcount{}, colour{}, enabled{};
    if (lle_batch_get_buffer(batch, LLE_BUF_POS, &pos) || lle_batch_get_buffer(batch, LLE_BUF_BITS, &bits) ||
        lle_batch_get_buffer(batch, LLE_BUF_EVCOUNT, &evcount) || lle_batch_get_buffer(batch, LLE_BUF_SRC_COLOUR, &colour) ||
        lle_batch_get_buffer(batch, LLE_BUF_SRC_ENABLED, &enabled)) {
        fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
        return nullptr;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, pos.ptr) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "the batch's buffers are not device memory");
        return nullptr;
    }
    auto* c = new lle_coop();
    c->device = attr.device;
    c->n_maps = n_maps;
    c->n_envs = lle_batch_n_envs(batch);
    std::string err;
    c->maps.resize((size_t)n_maps);
    for (int m = 0; m < n_maps; m++) {
        if (!maps[m] || !build_map(maps[m], c->maps[(size_t)m], err)) {
            fail(LLE_ERR_ARG, maps[m] ? err : "NULL map");
            delete c;
            return nullptr;
        }
        const MapTables& a = c->maps[0], &b = c->maps[(size_t)m];
        if (a.H != b.H || a.W != b.W || a.A != b.A || a.n_sources != b.n_sources || a.first_word != b.first_word) {
            fail(LLE_ERR_ARG, "the maps of a batch share height, width, agents, sources and beam words");
            delete c;
            return nullptr;
        }
        c->any_start_on_beam = c->any_start_on_beam || b.start_on_beam;
    }
    const MapTables& m0 = c->maps[0];
    if (c->n_envs <= 0 || c->n_envs % n_maps != 0 || m0.A < 1) {
        fail(LLE_ERR_ARG, "n_envs must be a positive multiple of n_maps");
        delete c;
        return nullptr;
    }

    DeviceGuard g(c->device);
    const size_t HW = (size_t)m0.H * m0.W, nA = (size_t)c->n_envs * (size_t)m0.A, n = (size_t)c->n_envs;
    std::vector<uint32_t> tables;
    for (const auto& m : c->maps) tables.insert(tables.end(), m.cells.begin(), m.cells.end());
    // the five arrays, each starting on a 256-byte boundary between runs of LLE_COOP_GUARD_BYTES zero bytes that no launch writes
    const size_t sizes[LLE_COOP_BUF_COUNT] = {nA * 4, nA * 4, nA * 4, n * 8, n * 8};
    size_t offsets[LLE_COOP_BUF_COUNT];
    const size_t state_bytes = eo::guarded_layout(sizes, LLE_COOP_BUF_COUNT, LLE_COOP_GUARD_BYTES, offsets);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMalloc(&c->d_tables, std::max<size_t>(4, tables.size() * 4)) != hipSuccess ||
        hipMalloc(&c->d_starts, (size_t)n_maps * lle::START_PITCH * 4) != hipSuccess ||
        hipMalloc(&c->d_colours, (size_t)n_maps * lle::COLOUR_PITCH * 4) != hipSuccess || hipMalloc(&c->d_state, state_bytes) != hipSuccess ||
        hipMalloc(&c->d_scratch, 256) != hipSuccess ||
        hipMemcpyAsync(c->d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(c->d_starts, 0, (size_t)n_maps * lle::START_PITCH * 4, st) != hipSuccess ||
        hipMemsetAsync(c->d_state, 0, state_bytes, st) != hipSuccess || hipMemsetAsync(c->d_scratch, 0, 256, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating or uploading the coop tables failed");
        lle_coop_free(c);
        return nullptr;
    }
    CoopParams& p = c->p;
    p.tables = c->d_tables;
    p.starts = c->d_starts;
    p.colours = c->d_colours;
    p.pos = static_cast<const uint8_t*>(pos.ptr);
    p.pos_stride = pos.stride[0];
    p.pos_agent_stride = pos.ndim > 2 ? pos.stride[1] : 2;
    p.bits = static_cast<const uint64_t*>(bits.ptr);
    p.evcount = static_cast<const uint8_t*>(evcount.ptr);
    p.src_colour = static_cast<const uint8_t*>(colour.ptr);
    p.colour_stride = colour.ndim > 1 ? colour.stride[0] : 0;
    p.src_enabled = static_cast<const uint32_t*>(enabled.ptr);
    p.step_edges = reinterpret_cast<uint32_t*>(c->d_state + offsets[LLE_COOP_STEP_EDGES]);
    p.episode_edges = reinterpret_cast<uint32_t*>(c->d_state + offsets[LLE_COOP_EPISODE_EDGES]);
    p.last_edges = reinterpret_cast<uint32_t*>(c->d_state + offsets[LLE_COOP_LAST_EDGES]);
    p.episode_profile = reinterpret_cast<uint64_t*>(c->d_state + offsets[LLE_COOP_EPISODE_PROFILE]);
    p.last_profile = reinterpret_cast<uint64_t*>(c->d_state + offsets[LLE_COOP_LAST_PROFILE]);
    p.n_envs = c->n_envs;
    p.envs_per_map = c->n_envs / n_maps;
    p.H = m0.H;
    p.W = m0.W;
    p.A = m0.A;
    p.L = m0.n_sources;
    std::memset(p.first_word, 0, sizeof(p.first_word));
    for (size_t l = 0; l < m0.first_word.size(); l++) p.first_word[l] = m0.first_word[l];
    int G = 1;
    while (G < m0.A) G <<= 1, c->log2_g++;
    // the table in LDS: it fits, and every workgroup's environments (256 / G consecutive ones) belong to one map
    const int64_t envs_per_block = lle::COOP_THREADS / G;
    c->lds_table = HW * 4 <= (size_t)lle::LDS_TABLE_MAX_BYTES && (n_maps == 1 || p.envs_per_map % envs_per_block == 0);
    for (int m = 0; m < n_maps; m++) {
        if (upload_map(c, m, maps[m], st) != LLE_OK) {
            lle_coop_free(c);
            return nullptr;
        }
    }
    g_error.clear();
    return c;
}

int lle_coop_update_map(lle_coop* c, int map_index, const lle_map* map, void* stream) {
    if (!c || !map) return fail(LLE_ERR_NULL, "NULL handle or map");
    if (map_index < 0 || map_index >= c->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    MapTables mt;
    std::string err;
    if (!build_map(map, mt, err)) return fail(LLE_ERR_ARG, err);
    const MapTables& old = c->maps[(size_t)map_index];
    if (mt.H != old.H || mt.W != old.W || mt.A != old.A || mt.n_sources != old.n_sources || mt.cells != old.cells || mt.start_ij != old.start_ij ||
        mt.first_word != old.first_word)
        return fail(LLE_ERR_ARG, "not a recompilation of the handle's map (the beams or the starts moved)");
    c->maps[(size_t)map_index] = mt;
    DeviceGuard g(c->device);
    return upload_map(c, map_index, map, reinterpret_cast<hipStream_t>(stream));
}

void* lle_coop_buffer(lle_coop* c, int which) {
    if (!c || which < 0 || which >= LLE_COOP_BUF_COUNT) {
        fail(LLE_ERR_ARG, "NULL handle or `which` not one of LLE_COOP_STEP_EDGES ... LLE_COOP_LAST_PROFILE");
        return nullptr;
    }
    switch (which) {
        case LLE_COOP_STEP_EDGES: return c->p.step_edges;
        case LLE_COOP_EPISODE_EDGES: return c->p.episode_edges;
        case LLE_COOP_LAST_EDGES: return c->p.last_edges;
        case LLE_COOP_EPISODE_PROFILE: return c->p.episode_profile;
        default: return c->p.last_profile;
    }
}

int lle_coop_start_edges(const lle_coop* c, int map_index, uint32_t* out, int cap) {
    if (!c) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= c->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    const MapTables& mt = c->maps[(size_t)map_index];
    if (out)
        for (int a = 0; a < std::min(cap, (int)mt.A); a++) out[a] = mt.starts[(size_t)a];
    return mt.A;
}

int lle_coop_update(lle_coop* c, const lle_coop_update_args* args, void* stream) {
    const int rc = lle_tracker_core::check_update_args(c, args, "lle_coop_update_args", LLE_COOP_HONOUR_AUTO_RESET | LLE_COOP_ENV_SOURCES);
    if (rc != LLE_OK) return rc;
    if ((args->flags & LLE_COOP_ENV_SOURCES) && c->any_start_on_beam && ((args->ops & LLE_COOP_MARK_STARTS) || (args->flags & LLE_COOP_HONOUR_AUTO_RESET)))
        return fail(LLE_ERR_ARG, "a start cell of the map lies on a laser cell and the batch has per-environment sources: the start edges depend on "
                                 "each environment's colours.  Reset through env_mask and send FINISH | CLEAR | MARK_POS on the reset state instead of "
                                 "LLE_COOP_MARK_STARTS / LLE_COOP_HONOUR_AUTO_RESET");
    CoopParams p = c->p;
    p.ops = args->ops;
    p.flags = args->flags;
    p.env_mask = args->env_mask;
    DeviceGuard g(c->device);
    return launch(p, c->log2_g, c->lds_table, reinterpret_cast<hipStream_t>(stream));
}

size_t lle_coop_debug_launched(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 10, g_launched.load(), buf, cap); }
size_t lle_coop_debug_compiled(char* buf, size_t cap) { return names_out(KERNEL_NAMES, 10, 0x3FFu, buf, cap); }

}  // extern "C"
