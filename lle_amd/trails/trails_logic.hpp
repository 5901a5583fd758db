// trails_logic.hpp -- the parts of the trail search (trails.hip, liblle_trails.so) that run the same on the host and on the device: how
// the arcs of one state lengthen the trails of a trajectory, what no-sequence-N rejects, and TrailKind: the trail word as the extra
// word of a record of ../search/search_logic.hpp.  tests/hostsim/trails_logic.cpp drives all of it under sanitizers.
//
// A TRAIL VALUE is one 32-bit word, 4 bits per agent: field a (bits 4 a .. 4 a + 3) = L[a], the length of the longest trail of help
// edges that ends at agent a (chained, times non-decreasing, no temporal edge twice).  It is part of a record's identity: hashed and
// compared after the search's key words.  A stored value holds at most N - 1 <= 15 in a field; what layer_update returns may carry
// REACHED in bit 31 instead: some trail has N edges.
#ifndef LLE_TRAILS_LOGIC_HPP
#define LLE_TRAILS_LOGIC_HPP

#include <stdint.h>

#include "../helpgraph/helpgraph_logic.hpp"
#include "../search/search_logic.hpp"

namespace lle_trails_logic {

namespace sl = lle_search_logic;
namespace hl = lle_helpgraph_logic;

constexpr int MIN_LENGTH = 2, MAX_LENGTH = 16;  // include/lle_trails.h: LLE_TRAILS_MIN_LENGTH, LLE_TRAILS_MAX_LENGTH
// Arc extensions one layer_update may make (LLE_TRAILS_WALK_BUDGET).  Every extension is a distinct non-empty ordered choice of
// distinct arcs of the state, so a state of m arcs makes at most sum over k = 1 .. m of m! / (m - k)! of them: 1 956 for m = 6, below
// the budget; the denser states no map of the catalogue reaches either answer within the budget or report DENSE.
constexpr int WALK_BUDGET = 4096;
constexpr uint32_t REACHED = 0x80000000u;  // bit 31 of what layer_update returns: a trail of N edges exists (agents use bits 0-23)

LLE_SEARCH_HD uint32_t field(uint32_t L, int a) { return (L >> (4 * a)) & 15u; }
LLE_SEARCH_HD uint32_t with_field(uint32_t L, int a, uint32_t v) { return (L & ~(15u << (4 * a))) | (v << (4 * a)); }
LLE_SEARCH_HD uint32_t longest(uint32_t L, int A) {
    uint32_t m = 0u;
    for (int a = 0; a < A; a++) m = field(L, a) > m ? field(L, a) : m;
    return m;
}

// Does no-sequence-N reject the trail value?  (Once true it stays true: L only grows.)
LLE_SEARCH_HD bool violates_sequence(uint32_t L, int N, int A) { return (L & REACHED) != 0u || (int)longest(L, A) >= N; }

// The trail value after ONE more state whose arcs are `edges` (the 48-bit help value of hl::state_edges: bit 8 h + b = h helps b):
//   L'[y] = max(L[y], max over x and over trails P inside `edges` from x to y of L[x] + |P|).
// A depth-first walk from every agent x that has an arc, over the arcs not yet used (a 48-bit mask in the layout of `edges`); a trail
// standing at y after d arcs has length L[x] + d.  The walk stops at once when a length reaches N: the value returned then has REACHED
// set and the caller drops the trajectory, so a level that goes on has length < N <= 16 and the stack is at most 15 arcs deep:
// 3 bits of agent and 3 bits of cursor (the next beneficiary to try) per level, in two 64-bit words.  No array, no recursion.
// Every arc extension takes one unit of `budget`; when it runs out `budget` is left negative and what is returned means nothing.
// A state without arcs leaves L as it is without entering the walk.  2 <= N <= 16, fields of L below N.
LLE_SEARCH_HD uint32_t layer_update(uint32_t L, uint64_t edges, int N, int A, int& budget) {
    if (edges == 0ull) return L;
    uint32_t best = L;
    for (int x = 0; x < A; x++) {
        if (hl::row_of(edges, x) == 0u) continue;
        const int base = (int)field(L, x);
        uint64_t agents = (uint64_t)x, cursors = 0ull, used = 0ull;
        int depth = 0;
        for (;;) {
            const int cur = (int)(agents >> (3 * depth)) & 7, c = (int)(cursors >> (3 * depth)) & 7;
            const uint32_t open = hl::row_of(edges & ~used, cur) & (0xFFu << c) & sl::agents_mask(A);
            if (open == 0u) {  // nothing left to try from here: back one arc, which becomes free again
                if (depth == 0) break;
                depth--;
                used &= ~((uint64_t)1 << (8 * ((int)(agents >> (3 * depth)) & 7) + cur));
                continue;
            }
            if (--budget < 0) return best;
            const int b = __builtin_ctz(open);
            cursors = (cursors & ~((uint64_t)7 << (3 * depth))) | (uint64_t)(b + 1) << (3 * depth);
            const int len = base + depth + 1;
            if (len >= N) return with_field(best, b, (uint32_t)(len < 15 ? len : 15)) | REACHED;
            if ((uint32_t)len > field(best, b)) best = with_field(best, b, (uint32_t)len);
            used |= (uint64_t)1 << (8 * cur + b);
            depth++;
            agents = (agents & ~((uint64_t)7 << (3 * depth))) | (uint64_t)b << (3 * depth);
            cursors &= ~((uint64_t)7 << (3 * depth));
        }
    }
    return best;
}

// ---- records with a trail word: the trail kind of ../search/search_logic.hpp, one extra word
// The IDENTITY of a record: the n_key key words of `rec`, then the trail word.
template <class Record>
LLE_SEARCH_HD sl::KeyWithExtra<Record, 1> key_with_trail(const Record& rec, int n_key, uint32_t trail) {
    return sl::key_with_extra(rec, n_key, sl::ExtraWords<1>{{trail}});
}
// The trail word of record s of a pool of `stride` records, at n_words behind search_logic.hpp's record.
LLE_SEARCH_HD uint32_t pool_trail(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t s) { return sl::pool_extra<1>(pool, stride, r, s).w[0]; }
LLE_SEARCH_HD void store_pool_trail(uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t s, uint32_t trail) {
    sl::store_pool_extra(pool, stride, r, s, sl::ExtraWords<1>{{trail}});
}

// The trail value of a successor whose state has the arcs `edges` and whose parent is pool record `parent`.
LLE_SEARCH_HD uint32_t successor_trail(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t parent, uint64_t edges, int N, int& budget) {
    return layer_update(pool_trail(pool, stride, r, parent), edges, N, r.A, budget);
}

struct TrailKind {
    static constexpr int EXTRA = 1;
    using Value = uint32_t;  // the trail value
    hl::EdgeRule rule;
    int32_t N;  // no trail of N edges
    template <class Record, class Cell>
    LLE_SEARCH_HD uint64_t state(const Record& rec, const sl::RecordLayout& r, const Cell& cell) const { return hl::state_edges(rec, r, rule, cell); }
    // false: the walk ran out of budget, and *trail means nothing
    LLE_SEARCH_HD bool successor(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t parent, uint64_t edges, Value* trail) const {
        int budget = WALK_BUDGET;
        *trail = successor_trail(pool, stride, r, parent, edges, N, budget);
        return budget >= 0;
    }
    LLE_SEARCH_HD bool violates(Value trail, int A) const { return violates_sequence(trail, N, A); }
    LLE_SEARCH_HD bool accepts(Value, int) const { return true; }
    static LLE_SEARCH_HD sl::ExtraWords<1> words(Value trail) { return sl::ExtraWords<1>{{trail}}; }
};

}  // namespace lle_trails_logic
#endif  // LLE_TRAILS_LOGIC_HPP
