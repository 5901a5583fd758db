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

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_cooptrails.h"
#include "cooptrails_logic.hpp"

namespace lle {

namespace ct = lle_cooptrails_logic;

constexpr int COOPTRAILS_THREADS = 256;
constexpr int START_PITCH = 16;  // per map: the start edges of every agent

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
    const bool was_reset = (p.flags & LLE_COOPTRAILS_HONOUR_AUTO_RESET) && (p.evcount[env] & 0x80u);
    const uint32_t reset_ops = was_reset ? (uint32_t)(LLE_COOPTRAILS_FINISH | LLE_COOPTRAILS_CLEAR | LLE_COOPTRAILS_MARK_STARTS) : 0u;
    if ((p.ops | reset_ops) == 0u) return;
    const bool refused = (p.flags & LLE_COOPTRAILS_SKIP_REFUSED) && p.err[env] != 0;
    const uint32_t own_ops = refused ? p.ops & ~(uint32_t)LLE_COOPTRAILS_MARK_POS : p.ops;
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
    for (int stage = 0; stage < 3; stage++) {
        const uint32_t ops = stage == 0 ? reset_ops : stage == 1 ? own_ops & ~(uint32_t)LLE_COOPTRAILS_MARK_POS : own_ops & (uint32_t)LLE_COOPTRAILS_MARK_POS;
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

// ================================================================================================ host side
using lle::CoopTrailsParams;

namespace {

thread_local std::string g_error;
std::atomic<uint32_t> g_launched{0};
// bit log2(G)
const char* const KERNEL_NAMES[5] = {"cooptrails_kernel<1>", "cooptrails_kernel<2>", "cooptrails_kernel<4>", "cooptrails_kernel<8>", "cooptrails_kernel<16>"};

int fail(int code, const std::string& why) {
    g_error = why;
    return code;
}

struct DeviceGuard {  // the handle's device current for the call, the caller's put back
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

size_t names_out(uint32_t bits, char* buf, size_t cap) {
    std::string s;
    for (int k = 0; k < 5; k++)
        if ((bits >> k) & 1u) s += std::string(KERNEL_NAMES[k]) + "\n";
    if (buf && cap > 0) {
        const size_t n = std::min(cap - 1, s.size());
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size() + 1;
}

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

struct lle_cooptrails {
    int device = 0;
    int n_maps = 0;
    int log2_g = 0;
    const lle_coop* coop = nullptr;
    uint32_t* d_starts = nullptr;
    uint8_t* d_state = nullptr;  // the four arrays between guard bytes
    CoopTrailsParams p{};
};

namespace {

// The start edges of map `m` from the coop handle to the device (synchronises `st`).
int upload_starts(lle_cooptrails* t, int m, hipStream_t st) {
    uint32_t rows[lle::START_PITCH] = {0};
    const int A = lle_coop_start_edges(t->coop, m, rows, lle::START_PITCH);
    if (A != t->p.A) return fail(LLE_ERR_ARG, std::string("lle_coop_start_edges: ") + (A < 0 ? lle_coop_last_error() : "another number of agents"));
    if (hipMemcpyAsync(t->d_starts + (size_t)m * lle::START_PITCH, rows, sizeof(rows), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "uploading the start edges failed");
    }
    return LLE_OK;
}

}  // namespace

extern "C" {

const char* lle_cooptrails_last_error(void) { return g_error.c_str(); }

void lle_cooptrails_free(lle_cooptrails* t) {
    if (!t) return;
    DeviceGuard g(t->device);
    (void)hipFree(t->d_starts);
    (void)hipFree(t->d_state);
    delete t;
}

lle_cooptrails* lle_cooptrails_create(lle_batch* batch, lle_coop* coop, void* stream) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) {
        (void)hipGetLastError();
        fail(LLE_ERR_NO_DEVICE, "no HIP device: the temporal cooperation tracker runs on the GPU only (there is no CPU fallback)");
        return nullptr;
    }
    if (!batch || !coop) {
        fail(LLE_ERR_NULL, "NULL batch or coop handle");
        return nullptr;
    }
    lle_buffer_desc evcount{}, err{};
    if (lle_batch_get_buffer(batch, LLE_BUF_EVCOUNT, &evcount) || lle_batch_get_buffer(batch, LLE_BUF_ERR, &err)) {
        fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
        return nullptr;
    }
    void* step_edges = lle_coop_buffer(coop, LLE_COOP_STEP_EDGES);
    const int A = lle_coop_start_edges(coop, 0, nullptr, 0);
    const int n_maps = lle_batch_n_maps(batch);
    const int64_t n = lle_batch_n_envs(batch);
    if (!step_edges || A < 1 || A > 16 || n_maps <= 0 || n <= 0 || n % n_maps != 0) {
        fail(LLE_ERR_ARG, "the coop handle or the batch is not usable (agents, maps or environments out of range)");
        return nullptr;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, step_edges) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "the coop handle's arrays are not device memory");
        return nullptr;
    }
    auto* t = new lle_cooptrails();
    t->device = attr.device;
    t->n_maps = n_maps;
    t->coop = coop;
    DeviceGuard g(t->device);
    // the four arrays, each starting on a 256-byte boundary between runs of LLE_COOP_GUARD_BYTES zero bytes that no launch writes
    const size_t guard = LLE_COOP_GUARD_BYTES;
    const size_t sizes[LLE_COOPTRAILS_BUF_COUNT] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4, (size_t)n * 4};
    size_t offsets[LLE_COOPTRAILS_BUF_COUNT], state_bytes = guard;
    for (int k = 0; k < LLE_COOPTRAILS_BUF_COUNT; k++) {
        offsets[k] = state_bytes;
        state_bytes += (sizes[k] + guard - 1) / guard * guard + guard;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t start_bytes = (size_t)n_maps * lle::START_PITCH * 4;
    if (hipMalloc(&t->d_starts, start_bytes) != hipSuccess || hipMalloc(&t->d_state, state_bytes) != hipSuccess ||
        hipMemsetAsync(t->d_starts, 0, start_bytes, st) != hipSuccess || hipMemsetAsync(t->d_state, 0, state_bytes, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating the cooptrails arrays failed");
        lle_cooptrails_free(t);
        return nullptr;
    }
    CoopTrailsParams& p = t->p;
    p.step_edges = static_cast<const uint32_t*>(step_edges);
    p.starts = t->d_starts;
    p.evcount = static_cast<const uint8_t*>(evcount.ptr);
    p.err = static_cast<const uint8_t*>(err.ptr);
    p.episode_trails = reinterpret_cast<uint64_t*>(t->d_state + offsets[LLE_COOPTRAILS_EPISODE_TRAILS]);
    p.last_trails = reinterpret_cast<uint64_t*>(t->d_state + offsets[LLE_COOPTRAILS_LAST_TRAILS]);
    p.episode_tprofile = reinterpret_cast<uint32_t*>(t->d_state + offsets[LLE_COOPTRAILS_EPISODE_TPROFILE]);
    p.last_tprofile = reinterpret_cast<uint32_t*>(t->d_state + offsets[LLE_COOPTRAILS_LAST_TPROFILE]);
    p.n_envs = n;
    p.envs_per_map = n / n_maps;
    p.A = A;
    int G = 1;
    while (G < A) G <<= 1, t->log2_g++;
    for (int m = 0; m < n_maps; m++) {
        if (upload_starts(t, m, st) != LLE_OK) {
            lle_cooptrails_free(t);
            return nullptr;
        }
    }
    g_error.clear();
    return t;
}

int lle_cooptrails_update_map(lle_cooptrails* t, int map_index, void* stream) {
    if (!t) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= t->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    DeviceGuard g(t->device);
    return upload_starts(t, map_index, reinterpret_cast<hipStream_t>(stream));
}

void* lle_cooptrails_buffer(lle_cooptrails* t, int which) {
    if (!t || which < 0 || which >= LLE_COOPTRAILS_BUF_COUNT) {
        fail(LLE_ERR_ARG, "NULL handle or `which` not one of LLE_COOPTRAILS_EPISODE_TRAILS ... LLE_COOPTRAILS_LAST_TPROFILE");
        return nullptr;
    }
    switch (which) {
        case LLE_COOPTRAILS_EPISODE_TRAILS: return t->p.episode_trails;
        case LLE_COOPTRAILS_LAST_TRAILS: return t->p.last_trails;
        case LLE_COOPTRAILS_EPISODE_TPROFILE: return t->p.episode_tprofile;
        default: return t->p.last_tprofile;
    }
}

int lle_cooptrails_update(lle_cooptrails* t, const lle_cooptrails_update_args* args, void* stream) {
    if (!t || !args) return fail(LLE_ERR_NULL, "NULL handle or arguments");
    if (args->struct_bytes != sizeof(lle_cooptrails_update_args))
        return fail(LLE_ERR_ARG, "lle_cooptrails_update_args.struct_bytes is not sizeof(lle_cooptrails_update_args)");
    const uint32_t all_ops = LLE_COOPTRAILS_FINISH | LLE_COOPTRAILS_CLEAR | LLE_COOPTRAILS_MARK_STARTS | LLE_COOPTRAILS_MARK_POS;
    const uint32_t all_flags = LLE_COOPTRAILS_HONOUR_AUTO_RESET | LLE_COOPTRAILS_SKIP_REFUSED;
    if ((args->ops & ~all_ops) || (args->flags & ~all_flags)) return fail(LLE_ERR_ARG, "unknown operation or flag");
    CoopTrailsParams p = t->p;
    p.ops = args->ops;
    p.flags = args->flags;
    p.env_mask = args->env_mask;
    DeviceGuard g(t->device);
    return launch(p, t->log2_g, reinterpret_cast<hipStream_t>(stream));
}

size_t lle_cooptrails_debug_launched(char* buf, size_t cap) { return names_out(g_launched.load(), buf, cap); }
size_t lle_cooptrails_debug_compiled(char* buf, size_t cap) { return names_out(0x1Fu, buf, cap); }

}  // extern "C"
