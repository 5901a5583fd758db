// policy_logic.hpp -- what the steps-to-go table (policy.hip, liblle_policy.so) adds to the search's host/device code
// (../search/search_logic.hpp: RecordLayout, hash_record, probe_step, table_insert, joint_available): a probe that only finds, the
// packing of a value and the exactness rule.  tests/hostsim/policy_values.cpp drives all three under sanitizers.
#ifndef LLE_POLICY_LOGIC_HPP
#define LLE_POLICY_LOGIC_HPP

#include <stdint.h>

#include "../search/search_logic.hpp"

namespace lle_policy_logic {

namespace sl = lle_search_logic;

// ---- a value: (steps << 16) | code, so that the 32-bit minimum is the smallest (steps, code) pair
constexpr uint32_t NO_PLAN = 0xFFFFFFFFu;   // no plan known
constexpr uint32_t MAX_STEPS = 0xFFFEu;     // the longest plan a value holds (0xFFFF in the high half is NO_PLAN's)
constexpr int32_t MAX_HORIZON = 32767;      // LLE_POLICY_MAX_HORIZON
constexpr int32_t ANSWER_UNKNOWN = -1;      // LLE_POLICY_UNKNOWN
constexpr int32_t ANSWER_DEAD_END = -2;     // LLE_POLICY_DEAD_END
constexpr uint32_t STAY = 4u;

LLE_SEARCH_HD uint32_t pack_value(uint32_t steps, uint32_t code) { return (steps << 16) | (code & 0xFFFFu); }
LLE_SEARCH_HD uint32_t value_steps(uint32_t v) { return v >> 16; }
LLE_SEARCH_HD uint32_t value_code(uint32_t v) { return v & 0xFFFFu; }
// The joint action in which every agent stays: digit 4 for each of A agents.
LLE_SEARCH_HD uint32_t stay_code(int A) { return sl::pow5(A) - 1u; }
// What state s offers its predecessor over the joint action `code`: one step more than its own value; NO_PLAN when it has none, or
// when the plan would not fit a value (the caller counts those: such a build has no answer).
LLE_SEARCH_HD uint32_t relaxed_value(uint32_t successor_value, uint32_t code, bool* saturated) {
    if (successor_value == NO_PLAN) return NO_PLAN;
    const uint32_t steps = value_steps(successor_value) + 1u;
    if (steps > MAX_STEPS) {
        *saturated = true;
        return NO_PLAN;
    }
    return pack_value(steps, code);
}

// ---- the exactness rule: the value v of a state first reached at `depth` is the true shortest distance iff the table is complete
// or depth + steps(v) <= horizon (include/lle_policy.h, EXACTNESS).
LLE_SEARCH_HD bool value_exact(uint32_t v, uint32_t depth, int32_t horizon, bool complete) {
    if (v == NO_PLAN) return complete;  // "no goal can be reached" is a statement about every reachable state
    return complete || (uint64_t)depth + value_steps(v) <= (uint64_t)(horizon < 0 ? 0 : horizon);
}
// What a lookup answers for a stored state: steps >= 0, ANSWER_UNKNOWN or ANSWER_DEAD_END.
LLE_SEARCH_HD int32_t answer_of(uint32_t v, uint32_t depth, int32_t horizon, bool complete) {
    if (v == NO_PLAN) return complete ? ANSWER_DEAD_END : ANSWER_UNKNOWN;
    return value_exact(v, depth, horizon, complete) ? (int32_t)value_steps(v) : ANSWER_UNKNOWN;
}

// ---- the probe that only finds
constexpr int64_t FIND_MISSING = -1;

// Linear probing from `hash` in a table of mask + 1 slots that nobody writes any more.  Returns the occupant (a pool index) whose
// record `same_as(occupant)` says is the caller's, or FIND_MISSING at the first empty slot or after mask + 1 slots that all held
// other records.  `load(slot)` is a plain 32-bit read.  An occupant with TAG_BIT (a candidate of a piece: no such slot is left in a
// finished table) is never handed to `same_as`.
template <class Load, class Same>
LLE_SEARCH_HD int64_t table_find(const uint32_t* table, uint32_t mask, uint64_t hash, const Load& load, const Same& same_as) {
    uint32_t s = (uint32_t)hash & mask;
    for (uint64_t n = 0; n <= (uint64_t)mask; n++) {
        const uint32_t seen = load(table + s);
        if (seen == sl::SLOT_EMPTY) return FIND_MISSING;
        if (!(seen & sl::TAG_BIT) && same_as(seen)) return (int64_t)seen;
        s = (s + 1u) & mask;
    }
    return FIND_MISSING;
}

}  // namespace lle_policy_logic
#endif  // LLE_POLICY_LOGIC_HPP
