// helpgraph_logic.hpp -- the parts of the help-graph search (helpgraph.hip, liblle_helpgraph.so) that run the same on the host and on the
// device: the help edges of one state, what a mode rejects and accepts, and HelpKind: the two help words as the extra words of a
// record of ../search/search_logic.hpp.  tests/hostsim/helpgraph_logic.cpp drives all of it under sanitizers.
//
// A HELP VALUE is 48 bits: byte h = the beneficiaries of helper h, bit 8 h + b set iff h has helped b in some state of the trajectory.
// It travels as two 32-bit words (lo, hi) that are part of a record's identity: hashed and compared after the search's key words.
#ifndef LLE_HELPGRAPH_LOGIC_HPP
#define LLE_HELPGRAPH_LOGIC_HPP

#include <stdint.h>

#include "../search/search_logic.hpp"

namespace lle_helpgraph_logic {

namespace sl = lle_search_logic;

// include/lle_helpgraph.h: LLE_HELPGRAPH_*
enum { STANDARD = 0, NO_ASYMMETRIC = 1, NO_MUTUAL = 2, NO_FULLY_COUPLED = 3, NO_CONVERGENCE = 4, NO_DIVERGENCE = 5, N_MODES = 6 };
constexpr int MAX_SOURCES = 32;  // one bit per source in a cell's word

LLE_SEARCH_HD uint32_t popcount8(uint32_t x) {  // of the low byte
    x &= 255u;
    x = (x & 0x55u) + ((x >> 1) & 0x55u);
    x = (x & 0x33u) + ((x >> 2) & 0x33u);
    return (x + (x >> 4)) & 15u;
}
LLE_SEARCH_HD uint32_t row_of(uint64_t help, int h) { return (uint32_t)(help >> (8 * h)) & 255u; }
LLE_SEARCH_HD uint32_t help_lo(uint64_t help) { return (uint32_t)help; }
LLE_SEARCH_HD uint32_t help_hi(uint64_t help) { return (uint32_t)(help >> 32); }
LLE_SEARCH_HD uint64_t help_of(uint32_t lo, uint32_t hi) { return (uint64_t)lo | (uint64_t)hi << 32; }

// What the edge rule needs of a map: cells[i * W + j] = the sources that own a laser tile on the cell (bit laser_id), mine[a] = the
// sources of colour a, enabled = the sources that are enabled.  `cell(c)` reads cells[c] (LDS or global memory on the device).
struct EdgeRule {
    int32_t A, H, W;
    uint32_t enabled;
    uint32_t mine[sl::MAX_AGENTS];
};

// The help value of ONE state, the coop kernel's rule: m_a = the cell word where agent a is its cell's occupant (bit 32 + a of
// LLE_BUF_BITS), else 0; own_a = m_a & mine[a] & enabled: the enabled sources of its colour whose tiles it stands on; a helps b != a
// iff m_b & own_a.  `rec(w)` reads word w of the state's record (positions in the first words, the occupant bits in word w_bits + 1).
template <class Record, class Cell>
LLE_SEARCH_HD uint64_t state_edges(const Record& rec, const sl::RecordLayout& r, const EdgeRule& e, const Cell& cell) {
    uint32_t m[sl::MAX_AGENTS];
    const uint32_t occupant = rec(r.w_bits + 1);
    bool any = false;
    for (int a = 0; a < sl::MAX_AGENTS; a++) {
        m[a] = 0u;
        if (a >= e.A || !((occupant >> a) & 1u)) continue;
        const uint32_t ij = rec(a >> 1) >> (16 * (a & 1));
        const int i = (int)(ij & 255u), j = (int)((ij >> 8) & 255u);
        if (i < e.H && j < e.W) m[a] = cell(i * e.W + j);
        any = any || m[a] != 0u;
    }
    uint64_t help = 0;
    if (!any) return help;
    for (int h = 0; h < e.A; h++) {
        const uint32_t own = m[h] & e.mine[h] & e.enabled;
        if (!own) continue;
        for (int b = 0; b < e.A; b++)
            if (b != h && (m[b] & own)) help |= (uint64_t)1 << (8 * h + b);
    }
    return help;
}

// Does a monotone mode reject the help value?  (Once true it stays true: a trajectory is dropped as soon as it is.)
LLE_SEARCH_HD bool violates(uint64_t help, int mode, int param, int A) {
    if (mode == NO_DIVERGENCE) {
        for (int h = 0; h < A; h++)
            if ((int)popcount8(row_of(help, h)) >= param) return true;
        return false;
    }
    if (mode == NO_CONVERGENCE) {
        for (int b = 0; b < A; b++) {
            int helpers = 0;
            for (int h = 0; h < A; h++) helpers += (int)((help >> (8 * h + b)) & 1u);
            if (helpers >= param) return true;
        }
        return false;
    }
    if (mode == NO_MUTUAL) {
        for (int h = 0; h < A; h++)
            for (int b = h + 1; b < A; b++)
                if (((help >> (8 * h + b)) & 1u) && ((help >> (8 * b + h)) & 1u)) return true;
        return false;
    }
    if (mode == NO_FULLY_COUPLED) {
        if (A < 2) return false;
        const uint32_t all = sl::agents_mask(A);
        for (int h = 0; h < A; h++)
            if ((row_of(help, h) | (1u << h)) != all) return false;
        return true;
    }
    return false;
}

// May a goal state with this help value end a plan?  NO_ASYMMETRIC: no edge whose helper is nobody's beneficiary.
LLE_SEARCH_HD bool accepts(uint64_t help, int mode, int A) {
    if (mode != NO_ASYMMETRIC) return true;
    uint32_t helped = 0u;
    for (int h = 0; h < A; h++) helped |= row_of(help, h);
    for (int h = 0; h < A; h++)
        if (row_of(help, h) != 0u && !((helped >> h) & 1u)) return false;
    return true;
}

// ---- records with help words: the help kind of ../search/search_logic.hpp, two extra words (lo, hi)
LLE_SEARCH_HD sl::ExtraWords<2> help_words(uint64_t help) { return sl::ExtraWords<2>{{help_lo(help), help_hi(help)}}; }
// The IDENTITY of a record: the n_key key words of `rec`, then the two help words.
template <class Record>
LLE_SEARCH_HD sl::KeyWithExtra<Record, 2> key_with_help(const Record& rec, int n_key, uint64_t help) {
    return sl::key_with_extra(rec, n_key, help_words(help));
}
// The help words of record s of a pool of `stride` records, at n_words and n_words + 1 behind search_logic.hpp's record.
LLE_SEARCH_HD uint64_t pool_help(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t s) {
    const sl::ExtraWords<2> x = sl::pool_extra<2>(pool, stride, r, s);
    return help_of(x.w[0], x.w[1]);
}
LLE_SEARCH_HD void store_pool_help(uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t s, uint64_t help) {
    sl::store_pool_extra(pool, stride, r, s, help_words(help));
}

struct HelpKind {
    static constexpr int EXTRA = 2;
    using Value = uint64_t;  // the help value
    EdgeRule rule;
    int32_t mode, param;
    template <class Record, class Cell>
    LLE_SEARCH_HD uint64_t state(const Record& rec, const sl::RecordLayout& r, const Cell& cell) const { return state_edges(rec, r, rule, cell); }
    // The help value of a successor: its parent's, from the pool, or-ed with the edges of its own state.
    LLE_SEARCH_HD bool successor(const uint32_t* pool, uint64_t stride, const sl::RecordLayout& r, uint64_t parent, uint64_t edges, Value* help) const {
        *help = pool_help(pool, stride, r, parent) | edges;
        return true;
    }
    LLE_SEARCH_HD bool violates(Value help, int A) const { return lle_helpgraph_logic::violates(help, mode, param, A); }
    LLE_SEARCH_HD bool accepts(Value help, int A) const { return lle_helpgraph_logic::accepts(help, mode, A); }
    static LLE_SEARCH_HD sl::ExtraWords<2> words(Value help) { return help_words(help); }
};

}  // namespace lle_helpgraph_logic
#endif  // LLE_HELPGRAPH_LOGIC_HPP
