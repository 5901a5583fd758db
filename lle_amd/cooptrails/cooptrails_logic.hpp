// cooptrails_logic.hpp -- the parts of the temporal cooperation tracker (cooptrails.hip, liblle_cooptrails.so) that run the same on
// the host and on the device: how the arcs of one state lengthen the help trails of an episode, for up to 16 agents, and the field-wise
// maximum of two trail values.  tests/hostsim/cooptrails_logic.cpp drives all of it under sanitizers.
//
// A TRAIL VALUE is one 64-bit word, 4 bits per agent: field a (bits 4 a .. 4 a + 3) = min(L[a], 15), L[a] the length of the longest
// trail of help edges that ends at agent a (chained, times non-decreasing, no temporal edge twice).  15 means
// "15 or more": the update never counts past 15 and never walks more than 15 arcs of a state.
// The ARCS of one state are 16 rows of 16 bits (row h = the beneficiaries of helper h) in four 64-bit words: word h / 4, bits
// 16 (h % 4) .. 16 (h % 4) + 15.  The arcs a walk has used are a mask of 256 bits in the same layout.
// No array is indexed at run time and nothing recurses: on the device everything stays in registers.
#ifndef LLE_COOPTRAILS_LOGIC_HPP
#define LLE_COOPTRAILS_LOGIC_HPP

#include <stdint.h>

#include "../coop/episode_ops.hpp"

#if defined(__HIPCC__)
#define LLE_COOPTRAILS_HD __host__ __device__ inline
#else
#define LLE_COOPTRAILS_HD inline
#endif

namespace lle_cooptrails_logic {

constexpr int MAX_AGENTS = 16;
constexpr uint32_t SATURATED = 15u;  // a field that holds 15 means 15 or more
// Arc extensions ONE walk (one starting agent) may make (LLE_COOPTRAILS_WALK_BUDGET), the budget of ../trails/trails_logic.hpp: a state
// of m arcs allows at most sum over k = 1 .. m of m! / (m - k)! ordered choices of distinct arcs, 1 956 for m = 6; the states a world of
// the catalogue reaches stay far below it, and a denser state leaves a lower bound and the dense mark.
constexpr int WALK_BUDGET = 4096;

struct Arcs {
    uint64_t w0, w1, w2, w3;
};

LLE_COOPTRAILS_HD Arcs no_arcs() { return Arcs{0ull, 0ull, 0ull, 0ull}; }
LLE_COOPTRAILS_HD bool any_arc(const Arcs& e) { return (e.w0 | e.w1 | e.w2 | e.w3) != 0ull; }
LLE_COOPTRAILS_HD uint64_t word_of(const Arcs& e, int k) { return k == 0 ? e.w0 : k == 1 ? e.w1 : k == 2 ? e.w2 : e.w3; }
LLE_COOPTRAILS_HD uint32_t row_of(const Arcs& e, int h) { return (uint32_t)(word_of(e, h >> 2) >> (16 * (h & 3))) & 0xFFFFu; }
// `e` with the bits of `bits` (< 2^16) set (on = true) or cleared in row h
LLE_COOPTRAILS_HD Arcs with_bits(Arcs e, int h, uint32_t bits, bool on) {
    const uint64_t m = (uint64_t)bits << (16 * (h & 3));
    const int k = h >> 2;
    const uint64_t m0 = k == 0 ? m : 0ull, m1 = k == 1 ? m : 0ull, m2 = k == 2 ? m : 0ull, m3 = k == 3 ? m : 0ull;
    if (on) { e.w0 |= m0; e.w1 |= m1; e.w2 |= m2; e.w3 |= m3; }
    else { e.w0 &= ~m0; e.w1 &= ~m1; e.w2 &= ~m2; e.w3 &= ~m3; }
    return e;
}
using lle_episode_ops::clean_row;  // a row of LLE_COOP_STEP_EDGES without the bits of agents >= A and without the self-loop

LLE_COOPTRAILS_HD uint32_t field(uint64_t L, int a) { return (uint32_t)(L >> (4 * a)) & 15u; }
LLE_COOPTRAILS_HD uint64_t with_field(uint64_t L, int a, uint32_t v) { return (L & ~((uint64_t)15 << (4 * a))) | (uint64_t)v << (4 * a); }
LLE_COOPTRAILS_HD uint32_t longest(uint64_t L) {
    uint32_t m = 0u;
    for (int a = 0; a < MAX_AGENTS; a++) m = field(L, a) > m ? field(L, a) : m;
    return m;
}

// The field-wise maximum of two trail values.  Even and odd fields apart, each in a byte of its own: (x | 0x10) - y keeps bit 4 of the
// byte exactly when x >= y and borrows nothing from the next byte.
LLE_COOPTRAILS_HD uint64_t field_max(uint64_t a, uint64_t b) {
    const uint64_t LOW = 0x0F0F0F0F0F0F0F0Full, ONES = 0x0101010101010101ull;
    uint64_t out = 0ull;
    for (int half = 0; half < 2; half++) {
        const uint64_t x = (a >> (4 * half)) & LOW, y = (b >> (4 * half)) & LOW;
        const uint64_t ge = ((((x | (ONES << 4)) - y) >> 4) & ONES) * 15ull;  // 0x0F in the bytes where x >= y
        out |= ((x & ge) | (y & ~ge & LOW)) << (4 * half);
    }
    return out;
}

// The walk from agent x over the arcs `e` of ONE state: L with every field y raised to min(L[x] + |P|, 15) for the trails P of at most
// 15 arcs inside `e` from x to y.  Depth first over the arcs not yet used; a trail standing at y after d arcs has length L[x] + d.
// Why 15 arcs are enough for min(L'[y], 15) to be exact: a trail of 15 or more edges that ends at y has a SUFFIX of exactly 15 edges,
// which is a trail too; the part of it inside this state has at most 15 arcs and starts at an agent whose field holds at least the
// rest.  So at most 15 levels are open: per level 4 bits of agent and 4 bits of cursor (the next beneficiary to try) in two 64-bit
// words, and one bit in `full` once the cursor has passed agent 15.  Every arc extension takes one unit of WALK_BUDGET; when it runs
// out *dense is set and what is returned is a lower bound in every field.
LLE_COOPTRAILS_HD uint64_t walk_from(uint64_t L, const Arcs& e, int x, bool* dense) {
    uint64_t best = L;
    if (row_of(e, x) == 0u) return best;
    const int base = (int)field(L, x);
    uint64_t agents = (uint64_t)x, cursors = 0ull;
    uint32_t full = 0u;
    Arcs used = no_arcs();
    int depth = 0, budget = WALK_BUDGET;
    for (;;) {
        const int cur = (int)(agents >> (4 * depth)) & 15, c = (int)(cursors >> (4 * depth)) & 15;
        const uint32_t open = ((full >> depth) & 1u) ? 0u : (row_of(e, cur) & ~row_of(used, cur) & (0xFFFFu << c) & 0xFFFFu);
        if (open == 0u) {  // nothing left to try from here: back one arc, which becomes free again
            if (depth == 0) break;
            full &= ~(1u << depth);
            depth--;
            used = with_bits(used, (int)(agents >> (4 * depth)) & 15, 1u << cur, false);
            continue;
        }
        if (--budget < 0) {
            *dense = true;
            break;
        }
        const int b = __builtin_ctz(open);
        cursors = (cursors & ~((uint64_t)15 << (4 * depth))) | (uint64_t)((b + 1) & 15) << (4 * depth);
        if (b == 15) full |= 1u << depth;
        const int len = base + depth + 1 < (int)SATURATED ? base + depth + 1 : (int)SATURATED;
        if ((uint32_t)len > field(best, b)) best = with_field(best, b, (uint32_t)len);
        if (depth + 1 >= (int)SATURATED) continue;  // 15 arcs: not extended
        used = with_bits(used, cur, 1u << b, true);
        depth++;  // <= 14
        agents = (agents & ~((uint64_t)15 << (4 * depth))) | (uint64_t)b << (4 * depth);
        cursors &= ~((uint64_t)15 << (4 * depth));
    }
    return best;
}

// The trail value after ONE more state whose arcs are `e` (rows cleaned by clean_row):
//   L'[y] = max(L[y], max over x and over trails P inside `e` from x to y of L[x] + |P|), every field saturating at 15.
// A state without arcs leaves L as it is without entering a walk.  The walks of the starting agents are independent (each reads the L
// of before the state): the device runs them in the lanes of a group and combines them with field_max.
LLE_COOPTRAILS_HD uint64_t layer_update(uint64_t L, const Arcs& e, int A, bool* dense) {
    if (!any_arc(e)) return L;
    uint64_t best = L;
    for (int x = 0; x < A; x++) best = field_max(best, walk_from(L, e, x, dense));
    return best;
}

}  // namespace lle_cooptrails_logic
#endif  // LLE_COOPTRAILS_LOGIC_HPP
