// abi_host.hpp -- the host prelude of a C ABI library, written once: the error string of a call, the device guard, and the text of the
// debug name functions.  Every .hip that exports a C ABI includes it (the search family through ../search/search_device.hpp).
// Everything here has internal linkage: every shared object keeps its own error string, and no symbol of one library can stand in for
// another's.
#ifndef LLE_ABI_HOST_HPP
#define LLE_ABI_HOST_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

namespace lle_abi_host {
namespace {

thread_local std::string g_error;  // what lle_*_last_error returns on this thread

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

// The names whose bit is set, one per line, into buf (truncated to cap); returns the bytes the whole text needs.
size_t names_out(const char* const* names, int count, uint32_t bits, char* buf, size_t cap) {
    std::string s;
    for (int k = 0; k < count; k++)
        if ((bits >> k) & 1u) s += std::string(names[k]) + "\n";
    if (buf && cap > 0) {
        const size_t n = std::min(cap - 1, s.size());
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return s.size() + 1;
}

}  // namespace
}  // namespace lle_abi_host
#endif  // LLE_ABI_HOST_HPP
