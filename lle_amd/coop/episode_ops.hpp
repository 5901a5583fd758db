// episode_ops.hpp -- the parts of a cooperation tracker that are not about its value, the same on the host and on the device and for
// coop.hip, ../cooptrails/cooptrails.hip and ../coopcycles/coopcycles.hip: which operations an environment gets from one update call
// and in which order, the cleaning of a row of help edges, and the layout of a handle's arrays between their guard bytes.
// tests/hostsim/episode_ops.cpp drives all of it under sanitizers.
//
// THE ORDER.  An update call carries operations and flags for every environment; what ONE environment runs is three stages:
//   stage 0  the auto-reset's: FINISH | CLEAR | MARK_STARTS where HONOUR_AUTO_RESET is set and bit 7 of the environment's
//            LLE_BUF_EVCOUNT byte says that the step kernel reset it first; nothing otherwise
//   stage 1  the caller's but MARK_POS
//   stage 2  the caller's MARK_POS -- dropped where SKIP_REFUSED is set and the environment's LLE_BUF_ERR byte is non-zero: a
//            refused step made no state
// and inside a stage FINISH, CLEAR, MARK_STARTS, MARK_POS in this order.  A library without SKIP_REFUSED runs stages 1 and 2 as one.
#ifndef LLE_EPISODE_OPS_HPP
#define LLE_EPISODE_OPS_HPP

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LLE_EPISODE_HD __host__ __device__ inline
#else
#define LLE_EPISODE_HD inline
#endif

namespace lle_episode_ops {

// The values of include/lle_coop.h, lle_cooptrails.h and lle_coopcycles.h (each .hip asserts that its header's are these).
constexpr uint32_t FINISH = 1u, CLEAR = 2u, MARK_STARTS = 4u, MARK_POS = 8u, ALL_OPS = 15u;
constexpr uint32_t HONOUR_AUTO_RESET = 1u, SKIP_REFUSED = 2u;
constexpr int STAGES = 3;

// The operations of stage 0.  `evcount` is where the environment's byte lies: it is read only where the flag asks for it.
LLE_EPISODE_HD uint32_t reset_ops(uint32_t flags, const uint8_t* evcount) {
    const bool was_reset = (flags & HONOUR_AUTO_RESET) && (*evcount & 0x80u);
    return was_reset ? FINISH | CLEAR | MARK_STARTS : 0u;
}
// The caller's operations as the environment takes them (stages 1 and 2).  `err` is where its byte lies, read as above.
LLE_EPISODE_HD uint32_t own_ops(uint32_t ops, uint32_t flags, const uint8_t* err) {
    const bool refused = (flags & SKIP_REFUSED) && *err != 0;
    return refused ? ops & ~MARK_POS : ops;
}
LLE_EPISODE_HD uint32_t stage_ops(uint32_t reset_ops, uint32_t own_ops, int stage) {
    return stage == 0 ? reset_ops : stage == 1 ? own_ops & ~MARK_POS : own_ops & MARK_POS;
}

// Row h of a state as the coop kernel stores it (a u32 of LLE_COOP_STEP_EDGES): bits of agents >= A and the self-loop dropped.
LLE_EPISODE_HD uint32_t clean_row(uint32_t row, int h, int A) { return row & ((1u << A) - 1u) & ~(1u << h) & 0xFFFFu; }

// k arrays of sizes[] bytes behind one another, each starting on a multiple of `guard` bytes (LLE_COOP_GUARD_BYTES) with at least
// `guard` bytes before it, between it and the next, and behind the last: their offsets, and the bytes of the whole.
inline size_t guarded_layout(const size_t* sizes, int k, size_t guard, size_t* offsets) {
    size_t total = guard;
    for (int i = 0; i < k; i++) {
        offsets[i] = total;
        total += (sizes[i] + guard - 1) / guard * guard + guard;
    }
    return total;
}

}  // namespace lle_episode_ops
#endif  // LLE_EPISODE_OPS_HPP
