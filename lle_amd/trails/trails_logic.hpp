// trails_logic.hpp -- the parts of the trail search (trails.hip, liblle_trails.so) that run the same on the host and on the device: how
// the arcs of one state lengthen the trails of a trajectory, what no-sequence-N rejects, and the functors that append the trail word to
// a record of ../search/search_logic.hpp.  tests/hostsim/trails_logic.cpp drives all of it under sanitizers.
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

// ---- records with a trail word
// The IDENTITY of a record: the n_key key words of `rec`, then the trail word.  What hash_record and same_record read, with n_key + 1 words.
template <class Record>
struct KeyWithTrail {
    const Record& rec;
    int n_key;
    uint32_t trail;
    LLE_SEARCH_HD uint32_t operator()(int w) const { return w < n_key ? rec(w) : trail; }
};
template <class Record>
LLE_SEARCH_HD KeyWithTrail<Record> key_with_trail(const Record& rec, int n_key, uint32_t trail) {
    return KeyWithTrail<Record>{rec, n_key, trail};
}
// Record s of a pool of `stride` records: the n_words words of search_logic.hpp's record, then the trail word at n_words.  It lives
// only here: the batch has no buffer for it.
LLE_SEARCH_HD uint32_t pool_trail(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t s) { return pool[(uint64_t)r.n_words * stride + s]; }
LLE_SEARCH_HD void store_pool_trail(uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t s, uint32_t trail) {
    pool[(uint64_t)r.n_words * stride + s] = trail;
}
struct PoolKeyWithTrail {  // the identity of pool record s
    const uint32_t* pool;
    uint64_t stride, s;
    int n_key, n_words;
    LLE_SEARCH_HD uint32_t operator()(int w) const { return pool[(uint64_t)(w < n_key ? w : n_words) * stride + s]; }
};

// The trail value of a successor whose state has the arcs `edges` and whose parent is pool record `parent`.  Both the parent's word
// and the state in the batch were written by earlier launches, so any lane may compute it for any candidate of the piece, at any time.
LLE_SEARCH_HD uint32_t successor_trail(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t parent, uint64_t edges, int N, int& budget) {
    return layer_update(pool_trail(pool, stride, r, parent), edges, N, r.A, budget);
}

// Whom the occupant of a table slot may name, as sl::Occupants, with what it takes to work out a candidate's trail value.
struct TrailOccupants {
    sl::BatchView batch;
    uint32_t n_tags;
    const uint32_t* pool;
    uint64_t stride, cap;
    uint64_t first_state, item0;  // the piece: candidate t expands pool record first_state + (item0 + t) / n_joint
    uint32_t n_joint;
    int32_t N;
};
// Is `occupant` the record `me` (a KeyWithTrail over the caller's own record, whose state has the arcs `edges`)?  A tag's key words lie
// complete in the batch since the step; its trail word is not stored anywhere during the insert launch: it is worked out here.  Equal
// key words mean an equal state and so equal arcs: the caller's `edges` are applied to the other candidate's parent, with the same
// function as by the lane that owns the candidate -- which found it within the budget and below N, or the tag would not be in the
// table.  No lane waits for another.
template <class Me>
LLE_SEARCH_HD bool trail_occupant_is(const TrailOccupants& o, const sl::RecordLayout& r, uint32_t occupant, const Me& me, uint64_t edges) {
    if (occupant & sl::TAG_BIT) {
        const uint32_t tag = occupant & ~sl::TAG_BIT;
        if (tag >= o.n_tags) return false;
        const sl::EnvRecord other{o.batch, r, (int64_t)tag};
        if (!sl::same_record(other, me, r.n_key)) return false;
        const uint64_t parent = o.first_state + (o.item0 + tag) / o.n_joint;
        if (parent >= o.cap) return false;
        int budget = WALK_BUDGET;
        const uint32_t trail = successor_trail(o.pool, o.stride, r, parent, edges, o.N, budget);
        return budget >= 0 && trail == me(r.n_key);
    }
    if (occupant >= o.cap) return false;
    return sl::same_record(PoolKeyWithTrail{o.pool, o.stride, occupant, r.n_key, r.n_words}, me, r.n_key + 1);
}

}  // namespace lle_trails_logic
#endif  // LLE_TRAILS_LOGIC_HPP
