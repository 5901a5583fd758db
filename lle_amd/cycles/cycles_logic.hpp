// cycles_logic.hpp -- the parts of the closed-trail search (cycles.hip, liblle_cycles.so) that run the same on the host and on the
// device: the packed set of (anchor, current, support) triples of a trajectory, how the arcs of one state extend it, what
// no-interdependence-N rejects, and CycleKind: the packed set as the extra words of a record of ../search/search_logic.hpp.
// tests/hostsim/cycles_logic.cpp drives all of it under sanitizers.
//
// THE VALUE.  R is the set of triples (anchor a, current c, support S) such that some trail of help edges (chained, times
// non-decreasing, no temporal edge twice) leads from a to c and visits exactly the agents S.  One more state with arcs E gives
//   R' = R u { (a, y, S u V(P)) : (a, x, S) in R u {(x, x, {x})}, P a non-empty trail inside E from x to y },
// P using every arc of E at most once, V(P) the agents P touches.  The sources are those of R, never of R': two trails inside one
// state may not be chained, they could share an arc.
//
// THE PRUNING RULE, part of the identity of a record.  Under no-interdependence-N:
//   a triple with |S| > N is never stored, because supports only grow;
//   a trajectory is dropped the moment some (a, a, S) with |S| = N appears;
//   kept are (a, c, S) with a != c and |S| <= N, and (a, a, S) with |S| < N.
//
// THE BITS.  Maps of up to 4 agents use the agent class AC = 4 and 3 words, maps of 5 or 6 agents AC = 6 and 21 words.  A pair (a, c)
// owns one FIELD, a bitset over the subsets of the REMAINING agents of the class: S always holds a and c, so bit p of the field stands
// for the support whose agent mask is p with a one inserted at bit min(a, c) and then at bit max(a, c) (a closed pair: at bit a).
//   closed field a            2^(AC - 1) bits at bit  a * 2^(AC - 1)                                          (AC = 6: word a)
//   open field (a, c), a != c 2^(AC - 2) bits at bit  AC * 2^(AC - 1) + (a * (AC - 1) + c - (c > a)) * 2^(AC - 2)
// AC = 4: 4 * 8 + 12 * 4 = 80 bits, AC = 6: 6 * 32 + 30 * 16 = 672 bits; no field straddles a word; unused bits are zero.
// The walk works on a field UNFOLDED to a bitset over all 2^AC agent masks (64 bits): there, adding agent v to every support of a set
// is one mask and one shift.  Nothing outside this library depends on the layout but lle_amd.cycles.triples.
#ifndef LLE_CYCLES_LOGIC_HPP
#define LLE_CYCLES_LOGIC_HPP

#include <stdint.h>

#include "../helpgraph/helpgraph_logic.hpp"
#include "../search/search_logic.hpp"

#if defined(__clang__)
#define LLE_CYCLES_UNROLL _Pragma("unroll")  // (the loops over a lane's unfolded supports: unrolled, they index registers)
#else
#define LLE_CYCLES_UNROLL
#endif

namespace lle_cycles_logic {

namespace sl = lle_search_logic;
namespace hl = lle_helpgraph_logic;

constexpr int MIN_ORDER = 2, MAX_ORDER = 6;  // include/lle_cycles.h: LLE_CYCLES_MIN_ORDER, LLE_CYCLES_MAX_ORDER
constexpr int WALK_BUDGET = 4096;            // arc extensions one layer_update may make (LLE_CYCLES_WALK_BUDGET, = LLE_TRAILS_WALK_BUDGET)
constexpr int SMALL_AGENTS = 4, SMALL_WORDS = 3, LARGE_WORDS = 21;  // LLE_CYCLES_VALUE_WORDS = LARGE_WORDS
// A trail inside one state uses every arc at most once: up to A (A - 1) = 30 arcs deep, 31 levels of the packed stack.
constexpr int MAX_DEPTH = sl::MAX_AGENTS * (sl::MAX_AGENTS - 1);
constexpr int LEVELS_PER_WORD = 21;  // 3 bits per level in a 64-bit word
static_assert(MAX_DEPTH + 1 <= 2 * LEVELS_PER_WORD, "the packed stack (two 64-bit words of 3-bit levels) holds a trail over all 30 arcs of one state");
static_assert(sl::MAX_AGENTS <= 6, "a bitset over all agent masks is one 64-bit word");

LLE_SEARCH_HD int words_of(int A) { return A <= SMALL_AGENTS ? SMALL_WORDS : LARGE_WORDS; }

template <int W>
struct Layout {
    static_assert(W == SMALL_WORDS || W == LARGE_WORDS, "two agent classes");
    static constexpr int AC = W == SMALL_WORDS ? SMALL_AGENTS : sl::MAX_AGENTS;
    static constexpr int CLOSED_BITS = 1 << (AC - 1), OPEN_BITS = 1 << (AC - 2);
    static constexpr int OPEN_BASE = AC * CLOSED_BITS, BITS = OPEN_BASE + AC * (AC - 1) * OPEN_BITS;
    static_assert((BITS + 31) / 32 == W, "the fields fill the words");
    static LLE_SEARCH_HD int closed_at(int a) { return a * CLOSED_BITS; }
    static LLE_SEARCH_HD int open_at(int a, int c) { return OPEN_BASE + (a * (AC - 1) + c - (c > a ? 1 : 0)) * OPEN_BITS; }
};

// ---- bitsets over agent masks
LLE_SEARCH_HD uint64_t even_blocks(int j) {  // the masks whose bit j is clear: the even blocks of 2^j bits
    return j == 0 ? 0x5555555555555555ull : j == 1 ? 0x3333333333333333ull : j == 2 ? 0x0F0F0F0F0F0F0F0Full : j == 3 ? 0x00FF00FF00FF00FFull
         : j == 4 ? 0x0000FFFF0000FFFFull : 0x00000000FFFFFFFFull;
}
// Of a bitset over masks, those that hold agent k, as a bitset over the masks with bit k taken out (half as many bits).
LLE_SEARCH_HD uint64_t take_with(uint64_t set, int k) {
    uint64_t t = (set >> (1u << k)) & even_blocks(k);
    for (int j = k; j < 5; j++) t = (t | (t >> (1u << j))) & even_blocks(j + 1);
    return t;
}
// The reverse: a bitset over masks without a bit k (at most 32 bits) as the bitset over masks that hold agent k.
LLE_SEARCH_HD uint64_t put_with(uint64_t set, int k) {
    uint64_t t = set;
    for (int j = 4; j >= k; j--) t = (t | (t << (1u << j))) & even_blocks(j);
    return t << (1u << k);
}
// Every agent of `agents` joins every support of the set: per agent v, the masks without v move onto those with it.
LLE_SEARCH_HD uint64_t lifted(uint64_t set, uint32_t agents) {
    for (int v = 0; v < sl::MAX_AGENTS; v++)
        if ((agents >> v) & 1u) set = (set & ~even_blocks(v)) | ((set & even_blocks(v)) << (1u << v));
    return set;
}
// The agent masks of exactly n agents, as a bitset.
LLE_SEARCH_HD uint64_t masks_of_size(int n) {
    uint64_t out = 0ull;
    for (uint32_t m = 0; m < 64u; m++)
        if ((int)(hl::popcount8(m)) == n) out |= (uint64_t)1 << m;
    return out;
}

// What the walk needs of N, worked out once on the host.
struct Order {
    int32_t N;
    uint64_t upto;     // the masks of at most N agents
    uint64_t exactly;  // the masks of exactly N agents
};
inline Order make_order(int N) {
    Order o{N, 0ull, masks_of_size(N)};
    for (int n = 0; n <= N; n++) o.upto |= masks_of_size(n);
    return o;
}

// ---- the words of a value: somebody's W words, `stride` words apart (a plain array: 1; one lane's slab in LDS: the workgroup's lanes)
struct Words {
    uint32_t* base;
    int32_t stride;
    LLE_SEARCH_HD uint32_t operator()(int i) const { return base[i * stride]; }
    LLE_SEARCH_HD void set(int i, uint32_t v) const { base[i * stride] = v; }
    LLE_SEARCH_HD void merge(int i, uint32_t v) const { base[i * stride] |= v; }
};
struct PoolWords {  // the value of record s of a pool, behind its n_words record words
    const uint32_t* pool;
    uint64_t stride, s;
    int32_t n_words;
    LLE_SEARCH_HD uint32_t operator()(int i) const { return pool[(uint64_t)(n_words + i) * stride + s]; }
};
struct NoWords {  // the empty set
    LLE_SEARCH_HD uint32_t operator()(int) const { return 0u; }
};

template <class Read>
LLE_SEARCH_HD uint32_t field(const Read& words, int at, int bits) {
    const uint32_t w = words(at >> 5) >> (at & 31);
    return bits >= 32 ? w : w & ((1u << bits) - 1u);
}
// The supports of (a, c) in R, unfolded.
template <int W, class Read>
LLE_SEARCH_HD uint64_t supports(const Read& words, int a, int c) {
    using Y = Layout<W>;
    if (a == c) return put_with(field(words, Y::closed_at(a), Y::CLOSED_BITS), a);
    const int lo = a < c ? a : c, hi = a < c ? c : a;
    return put_with(put_with(field(words, Y::open_at(a, c), Y::OPEN_BITS), lo), hi);
}
// The unfolded supports `set` of (a, c), every one holding a and c, joined to the field.
template <int W>
LLE_SEARCH_HD void merge_supports(const Words& words, int a, int c, uint64_t set) {
    using Y = Layout<W>;
    if (a == c) {
        const int at = Y::closed_at(a);
        words.merge(at >> 5, (uint32_t)take_with(set, a) << (at & 31));
        return;
    }
    const int lo = a < c ? a : c, hi = a < c ? c : a, at = Y::open_at(a, c);
    words.merge(at >> 5, (uint32_t)take_with(take_with(set, hi), lo) << (at & 31));
}

struct Stack {  // 3 bits per level
    uint64_t lo, hi;
    LLE_SEARCH_HD int get(int d) const { return (int)((d < LEVELS_PER_WORD ? lo >> (3 * d) : hi >> (3 * (d - LEVELS_PER_WORD))) & 7u); }
    LLE_SEARCH_HD void set(int d, int v) {
        if (d < LEVELS_PER_WORD) lo = (lo & ~((uint64_t)7 << (3 * d))) | (uint64_t)v << (3 * d);
        else hi = (hi & ~((uint64_t)7 << (3 * (d - LEVELS_PER_WORD)))) | (uint64_t)v << (3 * (d - LEVELS_PER_WORD));
    }
};

// `out` = R' of the pruning rule above, from R = `old` and ONE more state whose arcs are `edges` (the 48-bit help value of
// hl::state_edges: bit 8 h + b = h helps b).  A depth-first walk from every agent x that has an arc, over the arcs not yet used (a
// 48-bit mask in the layout of `edges`), no recursion: agent and cursor (the next beneficiary to try) of every level in a packed
// Stack, how often the trail stands on each agent in 5 bits per agent.  At a trail from x standing at y with agents V, every
// anchor's supports of (a, x) -- unfolded once per x, with (x, x, {x}) among those of x -- are lifted by V, cut to at most N agents and
// joined to (a, y).  An arc to an agent that would make |V| exceed N is not taken: no support of at most N agents lies behind it.
// The walk stops at once with `closed` set when some (a, a, S) with |S| = N appears: the caller drops the trajectory, and `out` means
// nothing.  Every arc tried takes one unit of `budget`; when it runs out `budget` is left negative and `out` means nothing.
// `out` may not alias `old`.  2 <= N <= 6.
template <int W, class Old>
LLE_SEARCH_HD void layer_update(const Old& old, const Words& out, uint64_t edges, const Order& order, int A, int& budget, bool& closed) {
    constexpr int AC = Layout<W>::AC;
    for (int i = 0; i < W; i++) out.set(i, old(i));
    if (edges == 0ull) return;
    for (int x = 0; x < A; x++) {
        if (hl::row_of(edges, x) == 0u) continue;
        uint64_t from[AC];  // (registers: every loop over it is unrolled)
LLE_CYCLES_UNROLL
        for (int a = 0; a < AC; a++) {
            from[a] = a < A ? supports<W>(old, a, x) : 0ull;
            if (a == x) from[a] |= (uint64_t)1 << (1u << x);
        }
        Stack agents{(uint64_t)x, 0ull}, cursors{0ull, 0ull};
        uint64_t used = 0ull;
        uint32_t stands = 1u << (5 * x);
        int depth = 0;
        for (;;) {
            const int cur = agents.get(depth), c = cursors.get(depth);
            const uint32_t open = hl::row_of(edges & ~used, cur) & (0xFFu << c) & sl::agents_mask(A);
            if (open == 0u) {  // nothing left to try from here: back one arc, which becomes free again
                if (depth == 0) break;
                depth--;
                used &= ~((uint64_t)1 << (8 * agents.get(depth) + cur));
                stands -= 1u << (5 * cur);
                continue;
            }
            if (--budget < 0) return;
            const int y = __builtin_ctz(open);
            cursors.set(depth, y + 1);
            uint32_t V = 1u << y;
            for (int v = 0; v < AC; v++)
                if ((stands >> (5 * v)) & 31u) V |= 1u << v;
            if ((int)hl::popcount8(V) > order.N) continue;
LLE_CYCLES_UNROLL
            for (int a = 0; a < AC; a++) {
                if (from[a] == 0ull) continue;
                const uint64_t set = lifted(from[a], V) & order.upto;
                if (set == 0ull) continue;
                if (a == y && (set & order.exactly) != 0ull) {
                    closed = true;
                    return;
                }
                merge_supports<W>(out, a, y, set);
            }
            used |= (uint64_t)1 << (8 * cur + y);
            stands += 1u << (5 * y);
            depth++;
            agents.set(depth, y);
            cursors.set(depth, 0);
        }
    }
}

// ---- records with a packed set: the cycle kind of ../search/search_logic.hpp, W extra words
struct CycleRule {  // what does not depend on the agent class: the kernels' parameters hold it
    hl::EdgeRule rule;
    Order order;     // no closed trail over exactly order.N agents
    uint32_t* work;  // W words, `work_stride` words apart, that successor() may write: one lane's own
    int32_t work_stride;
};

template <int W>
struct CycleKind : CycleRule {
    static constexpr int EXTRA = W;
    struct Value {
        uint32_t w[W];
        uint32_t closed;  // != 0: a closed trail of order N exists, and w means nothing
    };
    LLE_SEARCH_HD explicit CycleKind(const CycleRule& r) : CycleRule(r) {}
    template <class Record, class Cell>
    LLE_SEARCH_HD uint64_t state(const Record& rec, const sl::RecordLayout& r, const Cell& cell) const { return hl::state_edges(rec, r, rule, cell); }
    // The value after a state with the arcs `edges`, from R = `old`.  false: the walk ran out of budget, and *value means nothing.
    template <class Old>
    LLE_SEARCH_HD bool update(const Old& old, uint64_t edges, int A, Value* value) const {
        int budget = WALK_BUDGET;
        bool closed = false;
        const Words out{work, work_stride};
        layer_update<W>(old, out, edges, order, A, budget, closed);
LLE_CYCLES_UNROLL
        for (int i = 0; i < W; i++) value->w[i] = out(i);
        value->closed = closed ? 1u : 0u;
        return budget >= 0;
    }
    LLE_SEARCH_HD bool successor(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t parent, uint64_t edges, Value* value) const {
        return update(PoolWords{pool, stride, parent, r.n_words}, edges, r.A, value);
    }
    LLE_SEARCH_HD bool violates(const Value& value, int) const { return value.closed != 0u; }
    LLE_SEARCH_HD bool accepts(const Value&, int) const { return true; }
    static LLE_SEARCH_HD sl::ExtraWords<W> words(const Value& value) {
        sl::ExtraWords<W> x;
LLE_CYCLES_UNROLL
        for (int i = 0; i < W; i++) x.w[i] = value.w[i];
        return x;
    }
};

}  // namespace lle_cycles_logic
#endif  // LLE_CYCLES_LOGIC_HPP
