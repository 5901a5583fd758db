// tracker_core.hpp -- the handle of a tracker that follows the coop launch, written once for ../cooptrails/cooptrails.hip and
// ../coopcycles/coopcycles.hip: a batch and a coop handle bound through the public ABI alone (lle_batch_get_buffer, lle_coop_buffer,
// lle_coop_start_edges), the map's start edges on the device, FOUR state arrays between guard bytes, and the checks of an update
// call.  A library keeps its Params, its kernel, its launch, its kernel names and its extern "C" functions.  coop.hip takes
// check_update_args only.  Everything here has internal linkage (../common/abi_host.hpp).
//
// What the templates expect.  Params has the fields step_edges, starts, evcount, err, env_mask, n_envs, envs_per_map, A, ops, flags
// of CoopTrailsParams; a handle is `struct lle_x : Tracker<Params>` plus what its launch needs.
#ifndef LLE_TRACKER_CORE_HPP
#define LLE_TRACKER_CORE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lle_coop.h"
#include "../common/abi_host.hpp"
#include "episode_ops.hpp"

namespace lle_tracker_core {
namespace {

using lle_abi_host::DeviceGuard;
using lle_abi_host::fail;
using lle_abi_host::g_error;

constexpr int START_PITCH = 16;  // per map: the start edges of every agent (lle_coop_start_edges)
constexpr int N_ARRAYS = 4;      // the library's LLE_*_BUF_COUNT

template <class Params>
struct Tracker {
    int device = 0;
    int n_maps = 0;
    const lle_coop* coop = nullptr;
    uint32_t* d_starts = nullptr;
    uint8_t* d_state = nullptr;          // the four arrays between guard bytes
    uint8_t* arrays[N_ARRAYS] = {};      // where each starts: what lle_*_buffer returns
    Params p{};
};

// How many agents a library serves.  `unsupported` NULL: more agents fail the general check of bind (LLE_ERR_ARG); otherwise they are
// refused behind it as LLE_ERR_UNSUPPORTED with the text it makes.
struct AgentLimit {
    int max_agents;
    std::string (*unsupported)(int n_agents);
};

// The start edges of map `m` from the coop handle to the device (synchronises `st`).
template <class T>
int upload_starts(T* t, int m, hipStream_t st) {
    uint32_t rows[START_PITCH] = {0};
    const int A = lle_coop_start_edges(t->coop, m, rows, START_PITCH);
    if (A != t->p.A) return fail(LLE_ERR_ARG, std::string("lle_coop_start_edges: ") + (A < 0 ? lle_coop_last_error() : "another number of agents"));
    if (hipMemcpyAsync(t->d_starts + (size_t)m * START_PITCH, rows, sizeof(rows), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "uploading the start edges failed");
    }
    return LLE_OK;
}

template <class T>
void destroy(T* t) {
    if (!t) return;
    DeviceGuard g(t->device);
    (void)hipFree(t->d_starts);
    (void)hipFree(t->d_state);
    delete t;
}

// The first half of lle_*_create: a new handle over `batch` and `coop` with nothing allocated, p.step_edges, p.evcount, p.err,
// p.n_envs, p.envs_per_map and p.A set; NULL and the error on a refusal.  `no_device` is the library's text for a machine without one.
template <class T>
T* bind(lle_batch* batch, lle_coop* coop, const char* no_device, const AgentLimit& limit) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) {
        (void)hipGetLastError();
        fail(LLE_ERR_NO_DEVICE, no_device);
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
    const bool too_many = A > limit.max_agents;
    if (!step_edges || A < 1 || (too_many && !limit.unsupported) || n_maps <= 0 || n <= 0 || n % n_maps != 0) {
        fail(LLE_ERR_ARG, "the coop handle or the batch is not usable (agents, maps or environments out of range)");
        return nullptr;
    }
    if (too_many) {
        fail(LLE_ERR_UNSUPPORTED, limit.unsupported(A));
        return nullptr;
    }
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, step_edges) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, "the coop handle's arrays are not device memory");
        return nullptr;
    }
    auto* t = new T();
    t->device = attr.device;
    t->n_maps = n_maps;
    t->coop = coop;
    t->p.step_edges = static_cast<const uint32_t*>(step_edges);
    t->p.evcount = static_cast<const uint8_t*>(evcount.ptr);
    t->p.err = static_cast<const uint8_t*>(err.ptr);
    t->p.n_envs = n;
    t->p.envs_per_map = n / n_maps;
    t->p.A = A;
    return t;
}

// The second half: the four arrays of env_bytes[k] bytes per environment, each starting on a 256-byte boundary between runs of
// LLE_COOP_GUARD_BYTES zero bytes that no launch writes, and the start edges of every map (synchronises).  t->arrays and p.starts
// are set and the error string is empty afterwards; on a failure `t` is destroyed and false comes back.
template <class T>
bool allocate(T* t, const size_t (&env_bytes)[N_ARRAYS], const char* alloc_failed, void* stream) {
    DeviceGuard g(t->device);
    size_t sizes[N_ARRAYS], offsets[N_ARRAYS];
    for (int k = 0; k < N_ARRAYS; k++) sizes[k] = (size_t)t->p.n_envs * env_bytes[k];
    const size_t state_bytes = lle_episode_ops::guarded_layout(sizes, N_ARRAYS, LLE_COOP_GUARD_BYTES, offsets);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t start_bytes = (size_t)t->n_maps * START_PITCH * 4;
    if (hipMalloc(&t->d_starts, start_bytes) != hipSuccess || hipMalloc(&t->d_state, state_bytes) != hipSuccess ||
        hipMemsetAsync(t->d_starts, 0, start_bytes, st) != hipSuccess || hipMemsetAsync(t->d_state, 0, state_bytes, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        (void)hipGetLastError();
        fail(LLE_ERR_HIP, alloc_failed);
        destroy(t);
        return false;
    }
    t->p.starts = t->d_starts;
    for (int k = 0; k < N_ARRAYS; k++) t->arrays[k] = t->d_state + offsets[k];
    for (int m = 0; m < t->n_maps; m++) {
        if (upload_starts(t, m, st) != LLE_OK) {
            destroy(t);
            return false;
        }
    }
    g_error.clear();
    return true;
}

template <class T>
int update_map(T* t, int map_index, void* stream) {
    if (!t) return fail(LLE_ERR_NULL, "NULL handle");
    if (map_index < 0 || map_index >= t->n_maps) return fail(LLE_ERR_ARG, "map_index out of range");
    DeviceGuard g(t->device);
    return upload_starts(t, map_index, reinterpret_cast<hipStream_t>(stream));
}

// `refusal` is the library's text for a NULL handle or a `which` that names no array.
template <class T>
void* buffer(T* t, int which, const char* refusal) {
    if (!t || which < 0 || which >= N_ARRAYS) {
        fail(LLE_ERR_ARG, refusal);
        return nullptr;
    }
    return t->arrays[which];
}

// What every lle_*_update refuses before it looks at its handle: `struct_name` is the name of Args in the library's header,
// `all_flags` the flags it knows (the operations are those of episode_ops.hpp in every library).
template <class Args>
int check_update_args(const void* handle, const Args* args, const char* struct_name, uint32_t all_flags) {
    if (!handle || !args) return fail(LLE_ERR_NULL, "NULL handle or arguments");
    if (args->struct_bytes != sizeof(Args)) return fail(LLE_ERR_ARG, std::string(struct_name) + ".struct_bytes is not sizeof(" + struct_name + ")");
    if ((args->ops & ~lle_episode_ops::ALL_OPS) || (args->flags & ~all_flags)) return fail(LLE_ERR_ARG, "unknown operation or flag");
    return LLE_OK;
}

// lle_*_update of a follow-on tracker: the checks, the handle's Params with the call's operations, flags and mask, and
// `launch(params, stream)` of the library with the handle's device current.  Nothing is allocated on this path.
template <class T, class Args, class Launch>
int update(T* t, const Args* args, const char* struct_name, void* stream, Launch launch) {
    const int rc = check_update_args(t, args, struct_name, lle_episode_ops::HONOUR_AUTO_RESET | lle_episode_ops::SKIP_REFUSED);
    if (rc != LLE_OK) return rc;
    auto p = t->p;
    p.ops = args->ops;
    p.flags = args->flags;
    p.env_mask = args->env_mask;
    DeviceGuard g(t->device);
    return launch(p, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace
}  // namespace lle_tracker_core
#endif  // LLE_TRACKER_CORE_HPP
