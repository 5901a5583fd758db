// search_logic.hpp -- the parts of the shortest-plan search (search.hip, liblle_search.so) that run the same on the host and on the
// device: the layout of a state record, its hash, one probe step of the open-addressing table and what a record means (dead agent,
// everybody arrived, an agent on a foreign beam).  tests/hostsim/search_table.cpp drives the table code under sanitizers.
//
// A RECORD is the dynamic state of one environment as 32-bit words, the identity first:
//   [0, n_pos)              LLE_BUF_POS: the 2 A position bytes (i, j per agent), little-endian, zero padded
//   [n_pos, n_pos + 2)      LLE_BUF_BITS: low word (alive 0-15 | arrived 16-31), high word (occupant 32-47 | dead by set_state 48-63)
//   [.., .. + Lw)           LLE_BUF_BEAMS: every beam word
//   [gems]                  LLE_BUF_GEMS
//   [avail, avail + n_av)   LLE_BUF_AVAIL: the A availability bytes, zero padded
// Two states are the same when their first n_key words are: everything up to the beams, the gem word too when gems must be collected.
#ifndef LLE_SEARCH_LOGIC_HPP
#define LLE_SEARCH_LOGIC_HPP

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LLE_SEARCH_HD __host__ __device__ inline
#else
#define LLE_SEARCH_HD inline
#endif

namespace lle_search_logic {

constexpr int MAX_BEAM_WORDS = 32;             // LLE_MAX_BEAM_WORDS
constexpr int MAX_RECORD_WORDS = 3 + 2 + MAX_BEAM_WORDS + 1 + 2;  // 40
constexpr uint32_t SLOT_EMPTY = 0xFFFFFFFFu;   // a table slot nobody has claimed
constexpr uint32_t TAG_BIT = 0x80000000u;      // slot = TAG_BIT | k: candidate k of the piece in flight; below TAG_BIT: a pool index
constexpr uint32_t MAX_CHUNK = 1u << 30;       // so that no tag is SLOT_EMPTY
constexpr uint32_t MAX_STATES = 1u << 30;      // the table has at most 2^31 slots: no slot number is SLOT_EMPTY

struct RecordLayout {
    int32_t A, Lw;
    int32_t n_pos, n_av;      // words of the position and availability bytes
    int32_t w_bits, w_beams, w_gems, w_avail;
    int32_t n_words;          // whole record
    int32_t n_key;            // identity: the words compared and hashed
};

LLE_SEARCH_HD RecordLayout make_layout(int A, int Lw, bool collect_gems) {
    RecordLayout r;
    r.A = A;
    r.Lw = Lw;
    r.n_pos = (2 * A + 3) / 4;
    r.n_av = (A + 3) / 4;
    r.w_bits = r.n_pos;
    r.w_beams = r.w_bits + 2;
    r.w_gems = r.w_beams + Lw;
    r.w_avail = r.w_gems + 1;
    r.n_words = r.w_avail + r.n_av;
    r.n_key = collect_gems ? r.w_gems + 1 : r.w_gems;
    return r;
}

LLE_SEARCH_HD uint64_t mix64(uint64_t x) {  // the finaliser of splitmix64
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Hash of the first n_key words of a record; `word(w)` reads word w.
template <class Word>
LLE_SEARCH_HD uint64_t hash_record(const Word& word, int n_key) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n_key;
    for (int w = 0; w < n_key; w++) h = mix64(h ^ ((uint64_t)word(w) + 0x9E3779B97F4A7C15ull * (uint64_t)(w + 1)));
    return h;
}

enum { PROBE_CLAIMED = 0, PROBE_DUPLICATE = 1, PROBE_NEXT = 2 };

// One probe step on `slot`.  `load(slot)` is a plain 32-bit read (a stale SLOT_EMPTY only costs the compare-and-swap it was meant to
// save), `cas(slot, expected, desired)` a 32-bit compare-and-swap that returns the value it found;
// `same_as(occupant)` compares the caller's record, word for word, with the one `occupant` (a pool index or a tag) stands for.
// A slot never goes back to SLOT_EMPTY and the record behind an occupant is complete before anybody can see the occupant, so one
// compare-and-swap and one comparison decide: nothing here waits for another lane.
template <class Load, class Cas, class Same>
LLE_SEARCH_HD int probe_step(uint32_t* slot, uint32_t tag, const Load& load, const Cas& cas, const Same& same_as) {
    uint32_t seen = load(slot);
    if (seen == SLOT_EMPTY) {
        seen = cas(slot, SLOT_EMPTY, tag);
        if (seen == SLOT_EMPTY) return PROBE_CLAIMED;
    }
    return same_as(seen) ? PROBE_DUPLICATE : PROBE_NEXT;
}

enum { INSERT_DUPLICATE = -1, INSERT_FULL = -2 };

// Linear probing from `hash` in a table of mask + 1 slots (a power of two).  Returns the slot claimed (>= 0), INSERT_DUPLICATE, or
// INSERT_FULL after mask + 1 slots that all held other records.
template <class Load, class Cas, class Same>
LLE_SEARCH_HD int64_t table_insert(uint32_t* table, uint32_t mask, uint64_t hash, uint32_t tag, const Load& load, const Cas& cas, const Same& same_as) {
    uint32_t s = (uint32_t)hash & mask;
    for (uint64_t n = 0; n <= (uint64_t)mask; n++) {
        const int r = probe_step(table + s, tag, load, cas, same_as);
        if (r == PROBE_CLAIMED) return (int64_t)s;
        if (r == PROBE_DUPLICATE) return INSERT_DUPLICATE;
        s = (s + 1u) & mask;
    }
    return INSERT_FULL;
}

// ---- what a record means
LLE_SEARCH_HD uint32_t agents_mask(int A) { return (1u << A) - 1u; }
// bits_lo = the low word of LLE_BUF_BITS
LLE_SEARCH_HD bool anybody_dead(uint32_t bits_lo, int A) { return (bits_lo & agents_mask(A)) != agents_mask(A); }
LLE_SEARCH_HD bool all_arrived(uint32_t bits_lo, int A) { return ((bits_lo >> 16) & agents_mask(A)) == agents_mask(A); }
LLE_SEARCH_HD bool all_gems(uint32_t gems, int G) { return G >= 32 ? gems == 0xFFFFFFFFu : gems == (1u << G) - 1u; }
// foreign[cell] (one byte) = bit min(c, FOREIGN_OTHER) set when a source of colour c owns a laser tile on the cell -- agents are at most
// 6, so bits 0-5 are theirs and every colour from 7 on shares bit 7: agent a may not stand there without cooperation when any bit but
// its own is set.
constexpr int FOREIGN_OTHER = 7;
LLE_SEARCH_HD uint8_t foreign_bit(int colour) { return (uint8_t)(1u << (colour < 0 ? FOREIGN_OTHER : colour < FOREIGN_OTHER ? colour : FOREIGN_OTHER)); }
LLE_SEARCH_HD bool on_foreign_beam(uint32_t cell_colours, int a) { return (cell_colours & ~(1u << a)) != 0u; }

// Joint action `code` in base 5, agent 0 the lowest digit: is every component in the agent's availability byte?  `avail(a)` reads it.
template <class Avail>
LLE_SEARCH_HD bool joint_available(uint32_t code, int A, const Avail& avail) {
    for (int a = 0; a < A; a++) {
        if (!((avail(a) >> (code % 5u)) & 1u)) return false;
        code /= 5u;
    }
    return true;
}

LLE_SEARCH_HD uint32_t pow5(int A) {
    uint32_t p = 1;
    for (int a = 0; a < A; a++) p *= 5u;
    return p;
}

}  // namespace lle_search_logic
#endif  // LLE_SEARCH_LOGIC_HPP
