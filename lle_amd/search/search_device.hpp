// search_device.hpp -- the HIP-side code that search.hip, ../forest/forest.hip and the steps-to-go library share: the error string and
// the device guard of a C ABI call, the choice of a device, the binding of an lle_batch's buffers to a BatchView (search_logic.hpp),
// the reset state read out of a batch and seeded into an empty pool and table, the foreign-beam table of a map, and the two device
// functors the table code probes with.  Everything here has internal linkage: every library keeps its own error string, and no
// symbol of one shared object can stand in for another's.  Global atomics are 32 bits wide; counters stay with the libraries.
// search_core.hpp, beside this file, builds the single-tree search of search.hip, ../helpgraph and ../trails on top of it.
#ifndef LLE_SEARCH_DEVICE_HPP
#define LLE_SEARCH_DEVICE_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lle_hip.h"
#include "../common/abi_host.hpp"
#include "search_logic.hpp"

namespace lle_search_device {
namespace {

namespace sl = lle_search_logic;

// the error string, fail, the device guard and names_out of ../common/abi_host.hpp, under this namespace's names
using lle_abi_host::DeviceGuard;
using lle_abi_host::fail;
using lle_abi_host::g_error;
using lle_abi_host::names_out;

// opt_device, or the current device when it is negative.  `no_device` is the library's text for a machine without one.
int choose_device(int opt_device, const char* no_device, int* device) {
    int n_devices = 0;
    if (hipGetDeviceCount(&n_devices) != hipSuccess || n_devices <= 0) {
        (void)hipGetLastError();
        return fail(LLE_ERR_NO_DEVICE, no_device);
    }
    *device = opt_device;
    if (*device < 0 && hipGetDevice(device) != hipSuccess) *device = 0;
    if (*device >= n_devices) return fail(LLE_ERR_ARG, "no such HIP device");
    return LLE_OK;
}

// What a state record holds.  `agents_text` is the library's refusal of too many agents, up to the count.
bool record_limits_ok(const lle_map_info& info, const char* agents_text) {
    if (info.n_agents > sl::MAX_AGENTS || info.n_agents < 1) {
        fail(LLE_ERR_UNSUPPORTED, agents_text + std::to_string(info.n_agents) + ")");
        return false;
    }
    if (info.n_beam_words > sl::MAX_BEAM_WORDS || info.n_beam_words < 0 || info.n_gems > 32) {
        fail(LLE_ERR_UNSUPPORTED, "more beam words or gems than a state record holds");
        return false;
    }
    return true;
}

// The seven buffers of `batch` the search moves states through, checked against the layout include/lle_hip.h describes.
int bind_batch(const lle_batch* batch, const lle_map_info& info, int64_t expected_envs, sl::BatchView* view) {
    lle_buffer_desc pos{}, bits{}, gems{}, beams{}, avail{}, actions{}, errs{};
    if (lle_batch_get_buffer(batch, LLE_BUF_POS, &pos) || lle_batch_get_buffer(batch, LLE_BUF_BITS, &bits) ||
        lle_batch_get_buffer(batch, LLE_BUF_GEMS, &gems) || lle_batch_get_buffer(batch, LLE_BUF_BEAMS, &beams) ||
        lle_batch_get_buffer(batch, LLE_BUF_AVAIL, &avail) || lle_batch_get_buffer(batch, LLE_BUF_ACTIONS, &actions) ||
        lle_batch_get_buffer(batch, LLE_BUF_ERR, &errs))
        return fail(LLE_ERR_ARG, "lle_batch_get_buffer failed");
    if (pos.elem_bytes != 1 || bits.elem_bytes != 8 || gems.elem_bytes != 4 || beams.elem_bytes != 4 || avail.elem_bytes != 1 || actions.elem_bytes != 1 ||
        errs.elem_bytes != 1 || pos.stride[0] < 2 * info.n_agents || avail.stride[0] < info.n_agents || actions.stride[0] < info.n_agents ||
        beams.stride[0] < info.n_beam_words || lle_batch_n_envs(batch) != expected_envs)
        return fail(LLE_ERR_UNSUPPORTED, "the batch's buffers do not have the layout include/lle_hip.h describes");
    view->pos = static_cast<uint8_t*>(pos.ptr);
    view->bits = static_cast<uint64_t*>(bits.ptr);
    view->gems = static_cast<uint32_t*>(gems.ptr);
    view->beams = static_cast<uint32_t*>(beams.ptr);
    view->avail = static_cast<uint8_t*>(avail.ptr);
    view->actions = static_cast<uint8_t*>(actions.ptr);
    view->err = static_cast<const uint8_t*>(errs.ptr);
    view->pos_stride = pos.stride[0];
    view->pos_agent_stride = pos.ndim > 2 ? pos.stride[1] : 2;
    view->beam_stride = beams.stride[0];
    view->avail_stride = avail.stride[0];
    view->act_stride = actions.stride[0];
    return LLE_OK;
}

// The record of environment 0 of a batch, copied to the host (synchronises) and packed by env_word itself.
int read_root(const sl::BatchView& v, const sl::RecordLayout& r, hipStream_t stream, std::vector<uint32_t>* root) {
    std::vector<uint8_t> pos((size_t)std::max<int64_t>(1, v.pos_stride)), avail((size_t)std::max<int64_t>(1, v.avail_stride));
    std::vector<uint32_t> beams((size_t)std::max(1, r.Lw));
    uint64_t bits = 0;
    uint32_t gems = 0;
    bool ok = hipMemcpyAsync(pos.data(), v.pos, pos.size(), hipMemcpyDeviceToHost, stream) == hipSuccess &&
              hipMemcpyAsync(avail.data(), v.avail, avail.size(), hipMemcpyDeviceToHost, stream) == hipSuccess &&
              hipMemcpyAsync(&bits, v.bits, 8, hipMemcpyDeviceToHost, stream) == hipSuccess &&
              hipMemcpyAsync(&gems, v.gems, 4, hipMemcpyDeviceToHost, stream) == hipSuccess;
    if (ok && r.Lw > 0) ok = hipMemcpyAsync(beams.data(), v.beams, (size_t)r.Lw * 4, hipMemcpyDeviceToHost, stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LLE_ERR_HIP, "reading the reset state failed");
    }
    sl::BatchView host = v;  // environment 0 alone, on the host
    host.pos = pos.data();
    host.avail = avail.data();
    host.bits = &bits;
    host.gems = &gems;
    host.beams = beams.data();
    root->assign((size_t)r.n_words, 0u);
    for (int w = 0; w < r.n_words; w++) (*root)[(size_t)w] = sl::env_word(host, r, 0, w);
    return LLE_OK;
}

// An empty table but for the root's slot, which names state 0, and the root's words as state 0 of a pool of `stride` states, with
// the n_extra words `extra` of a search kind behind them (search_logic.hpp: the identity is the key words, then those).  Only
// enqueues: the caller adds what it keeps per state and synchronises before `root` and `extra` change.
bool seed_root(uint32_t* table, uint32_t table_mask, uint32_t* pool, uint64_t stride, const uint32_t* root, const sl::RecordLayout& r, hipStream_t stream,
               const uint32_t* extra = nullptr, int n_extra = 0) {
    static const uint32_t zero = 0u;
    const uint64_t h = sl::hash_record([&](int w) { return w < r.n_key ? root[w] : extra[w - r.n_key]; }, r.n_key + n_extra);
    bool ok = hipMemsetAsync(table, 0xFF, ((size_t)table_mask + 1) * 4, stream) == hipSuccess &&
              hipMemcpyAsync(table + ((uint32_t)h & table_mask), &zero, 4, hipMemcpyHostToDevice, stream) == hipSuccess;
    for (int w = 0; ok && w < r.n_words + n_extra; w++)
        ok = hipMemcpyAsync(pool + (size_t)w * stride, w < r.n_words ? &root[w] : &extra[w - r.n_words], 4, hipMemcpyHostToDevice, stream) == hipSuccess;
    return ok;
}

// foreign[cell] of one map (search_logic.hpp: foreign_bit), H * W bytes appended to `out`; false: a laser tile lies outside the map.
bool build_foreign(const lle_map* map, int H, int W, std::vector<uint8_t>& out) {
    std::vector<lle_source_info> src((size_t)std::max(0, lle_map_sources(map, nullptr, 0)));
    lle_map_sources(map, src.data(), (int)src.size());
    const size_t base = out.size();
    out.resize(base + (size_t)H * W, 0);
    std::vector<lle_laser_tile> tiles((size_t)std::max(0, lle_map_laser_tiles(map, nullptr, 0)));
    lle_map_laser_tiles(map, tiles.data(), (int)tiles.size());
    for (const auto& t : tiles) {
        if (t.i < 0 || t.i >= H || t.j < 0 || t.j >= W || t.laser_id < 0 || t.laser_id >= (int)src.size()) return false;
        out[base + (size_t)t.i * W + t.j] |= sl::foreign_bit(src[(size_t)t.laser_id].agent_id);
    }
    return true;
}

// ---- how a kernel reads and claims a table slot (search_logic.hpp: probe_step)
__device__ inline uint32_t relaxed_load(const uint32_t* at) { return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
struct SlotLoad {
    __device__ uint32_t operator()(const uint32_t* slot) const { return relaxed_load(slot); }
};
struct SlotCas {
    __device__ uint32_t operator()(uint32_t* slot, uint32_t expected, uint32_t desired) const { return atomicCAS(slot, expected, desired); }
};

}  // namespace
}  // namespace lle_search_device
#endif  // LLE_SEARCH_DEVICE_HPP
