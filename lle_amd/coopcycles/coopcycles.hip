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

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_coopcycles.h"
#include "../cycles/cycles_logic.hpp"

namespace lle {

namespace cl = lle_cycles_logic;

constexpr int COOPCYCLES_THREADS = 256;
constexpr int START_PITCH = 16;  // per map: the start edges of every agent (lle_coop_start_edges)

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

// Row h of a layer, cleaned by the rule of lle_cooptrails_logic::clean_row: no self-loop, no agent the map lacks.
__device__ __forceinline__ uint32_t clean_row(uint32_t row, int h, int A) { return row & ((1u << A) - 1u) & ~(1u << h) & 0xFFFFu; }

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
    const bool was_reset = (p.flags & LLE_COOPCYCLES_HONOUR_AUTO_RESET) && (p.evcount[env] & 0x80u);
    const uint32_t reset_ops = was_reset ? (uint32_t)(LLE_COOPCYCLES_FINISH | LLE_COOPCYCLES_CLEAR | LLE_COOPCYCLES_MARK_STARTS) : 0u;
    if ((p.ops | reset_ops) == 0u) return;
    const bool refused = (p.flags & LLE_COOPCYCLES_SKIP_REFUSED) && p.err[env] != 0;
    const uint32_t own_ops = refused ? p.ops & ~(uint32_t)LLE_COOPCYCLES_MARK_POS : p.ops;
    const int A = p.A;

    // ---- the arc words of both layers: bit 8 h + b = h helps b
    uint64_t step = 0ull, start = 0ull;
    if (own_ops & LLE_COOPCYCLES_MARK_POS)
        for (int h = 0; h < A; h++) step |= (uint64_t)clean_row(p.step_edges[env * A + h], h, A) << (8 * h);
    if ((own_ops | reset_ops) & LLE_COOPCYCLES_MARK_STARTS)
        for (int h = 0; h < A; h++) start |= (uint64_t)clean_row(p.starts[(env / p.envs_per_map) * START_PITCH + h], h, A) << (8 * h);

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
    for (int stage = 0; stage < 3; stage++) {
        const uint32_t ops = stage == 0 ? reset_ops : stage == 1 ? own_ops & ~(uint32_t)LLE_COOPCYCLES_MARK_POS : own_ops & (uint32_t)LLE_COOPCYCLES_MARK_POS;
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

// ================================================================================================ host side
using lle::CoopCyclesParams;
namespace cl = lle_cycles_logic;

namespace {

thread_local std::string g_error;
std::atomic<uint32_t> g_launched{0};
// bit 0: W = 3, bit 1: W = 21
const char* const KERNEL_NAMES[2] = {"coopcycles_kernel<3>", "coopcycles_kernel<21>"};

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
    for (int k = 0; k < 2; k++)
        if ((bits >> k) & 1u) s += std::string(KERNEL_NAMES[k]) + "\n";
    if (buf && cap > 0) {
        const size_t n = std::min(cap - 1, s.size());
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size() + 1;
}

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

}  // namespace

struct lle_coopcycles {
    int device = 0;
    int n_maps = 0;
    int words = 0;
    const lle_coop* coop = nullptr;
    uint32_t* d_starts = nullptr;
    uint8_t* d_state = nullptr;  // the four arrays between guard bytes
    CoopCyclesParams p{};
};

namespace {

// The start edges of map `m` from the coop handle to the device (synchronises `st`).
int upload_starts(lle_coopcycles* t, int m, hipStream_t st) {
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

const char* lle_coopcycles_last_error(void) { return g_error.c_str(); }

void lle_coopcycles_free(lle_coopcycles* t) {
    if (!t) return;
    DeviceGuard g(t->device);
    (void)hipFree(t->d_starts);
    (void)hipFree(t->d_state);
    delete t;
}

lle_coopcycles* lle_coopcycles_create(lle_batch* batch, lle_coop* coop, void* stream) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) {
        (void)hipGetLastError();
        fail(LLE_ERR_NO_DEVICE, "no HIP device: the closed-trail cooperation tracker runs on the GPU only (there is no CPU fallback)");
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
    if (!step_edges || A < 1 || n_maps <= 0 || n <= 0 || n % n_maps != 0) {
        fail(LLE_ERR_ARG, "the coop handle or the batch is not usable (agents, maps or environments out of range)");
        return nullptr;
    }
    if (A > LLE_COOPCYCLES_MAX_AGENTS) {
        fail(LLE_ERR_UNSUPPORTED, "the closed-trail tracker serves maps of at most " + std::to_string(LLE_COOPCYCLES_MAX_AGENTS) + " agents, this one has " +
                                      std::to_string(A) + ": a packed set of agent masks is one 64-bit word");
        return nullptr;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, step_edges) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "the coop handle's arrays are not device memory");
        return nullptr;
    }
    auto* t = new lle_coopcycles();
    t->device = attr.device;
    t->n_maps = n_maps;
    t->coop = coop;
    t->words = cl::words_of(A);
    DeviceGuard g(t->device);
    // the four arrays, each starting on a 256-byte boundary between runs of LLE_COOP_GUARD_BYTES zero bytes that no launch writes
    const size_t guard = LLE_COOP_GUARD_BYTES;
    const size_t sizes[LLE_COOPCYCLES_BUF_COUNT] = {(size_t)n * 4 * (size_t)t->words, (size_t)n * 4 * (size_t)t->words, (size_t)n * 4, (size_t)n * 4};
    size_t offsets[LLE_COOPCYCLES_BUF_COUNT], state_bytes = guard;
    for (int k = 0; k < LLE_COOPCYCLES_BUF_COUNT; k++) {
        offsets[k] = state_bytes;
        state_bytes += (sizes[k] + guard - 1) / guard * guard + guard;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t start_bytes = (size_t)n_maps * lle::START_PITCH * 4;
    if (hipMalloc(&t->d_starts, start_bytes) != hipSuccess || hipMalloc(&t->d_state, state_bytes) != hipSuccess ||
        hipMemsetAsync(t->d_starts, 0, start_bytes, st) != hipSuccess || hipMemsetAsync(t->d_state, 0, state_bytes, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "allocating the coopcycles arrays failed");
        lle_coopcycles_free(t);
        return nullptr;
    }
    CoopCyclesParams& p = t->p;
    p.step_edges = static_cast<const uint32_t*>(step_edges);
    p.starts = t->d_starts;
    p.evcount = static_cast<const uint8_t*>(evcount.ptr);
    p.err = static_cast<const uint8_t*>(err.ptr);
    p.episode_closed = reinterpret_cast<uint32_t*>(t->d_state + offsets[LLE_COOPCYCLES_EPISODE_CLOSED]);
    p.last_closed = reinterpret_cast<uint32_t*>(t->d_state + offsets[LLE_COOPCYCLES_LAST_CLOSED]);
    p.episode_cprofile = reinterpret_cast<uint32_t*>(t->d_state + offsets[LLE_COOPCYCLES_EPISODE_CPROFILE]);
    p.last_cprofile = reinterpret_cast<uint32_t*>(t->d_state + offsets[LLE_COOPCYCLES_LAST_CPROFILE]);
    p.n_envs = n;
    p.envs_per_map = n / n_maps;
    p.A = A;
    p.order = cl::Order{A, ~0ull, 0ull};  // N = the map's agents, every mask allowed, none "exact": no pruning, no closing
    for (int k = 0; k <= cl::MAX_ORDER; k++) p.of_size[k] = cl::masks_of_size(k);
    for (int m = 0; m < n_maps; m++) {
        if (upload_starts(t, m, st) != LLE_OK) {
            lle_coopcycles_free(t);
            return nullptr;
        }
    }
    g_error.clear();
    return t;
}

int lle_coopcycles_update_map(lle_coopcycles* t, int map_index, void* stream) {
    if (!t) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= t->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    DeviceGuard g(t->device);
    return upload_starts(t, map_index, reinterpret_cast<hipStream_t>(stream));
}

void* lle_coopcycles_buffer(lle_coopcycles* t, int which) {
    if (!t || which < 0 || which >= LLE_COOPCYCLES_BUF_COUNT) {
        fail(LLE_ERR_ARG, "NULL handle or `which` not one of LLE_COOPCYCLES_EPISODE_CLOSED ... LLE_COOPCYCLES_LAST_CPROFILE");
        return nullptr;
    }
    switch (which) {
        case LLE_COOPCYCLES_EPISODE_CLOSED: return t->p.episode_closed;
        case LLE_COOPCYCLES_LAST_CLOSED: return t->p.last_closed;
        case LLE_COOPCYCLES_EPISODE_CPROFILE: return t->p.episode_cprofile;
        default: return t->p.last_cprofile;
    }
}

int lle_coopcycles_update(lle_coopcycles* t, const lle_coopcycles_update_args* args, void* stream) {
    if (!t || !args) return fail(LLE_ERR_NULL, "NULL handle or arguments");
    if (args->struct_bytes != sizeof(lle_coopcycles_update_args))
        return fail(LLE_ERR_ARG, "lle_coopcycles_update_args.struct_bytes is not sizeof(lle_coopcycles_update_args)");
    const uint32_t all_ops = LLE_COOPCYCLES_FINISH | LLE_COOPCYCLES_CLEAR | LLE_COOPCYCLES_MARK_STARTS | LLE_COOPCYCLES_MARK_POS;
    const uint32_t all_flags = LLE_COOPCYCLES_HONOUR_AUTO_RESET | LLE_COOPCYCLES_SKIP_REFUSED;
    if ((args->ops & ~all_ops) || (args->flags & ~all_flags)) return fail(LLE_ERR_ARG, "unknown operation or flag");
    CoopCyclesParams p = t->p;
    p.ops = args->ops;
    p.flags = args->flags;
    p.env_mask = args->env_mask;
    DeviceGuard g(t->device);
    return launch(p, t->words, reinterpret_cast<hipStream_t>(stream));
}

size_t lle_coopcycles_debug_launched(char* buf, size_t cap) { return names_out(g_launched.load(), buf, cap); }
size_t lle_coopcycles_debug_compiled(char* buf, size_t cap) { return names_out(0x3u, buf, cap); }

}  // extern "C"
