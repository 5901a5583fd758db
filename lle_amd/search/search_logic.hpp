// search_logic.hpp -- the parts of the shortest-plan search (search.hip, liblle_search.so) that run the same on the host and on the
// device: the layout of a state record, its hash, one probe step of the open-addressing table, what a record means (dead agent,
// everybody arrived, an agent on a foreign beam) and the record I/O: how a record is read out of and written into the buffers of a
// batch (BatchView, env_word, scatter_item, copy_record), how it lies in a pool (PoolRecord) and whom a table slot names
// (occupant_is), and the records with extra words of a search KIND (ExtraWords, KeyWithExtra, Piece and the occupant comparison over
// a kind) that ../helpgraph, ../trails and ../helpforest search with.  ../forest/forest.hip and the steps-to-go library use the same
// code; search_device.hpp holds what needs HIP, search_core.hpp the single-tree search itself.
// tests/hostsim/search_table.cpp drives the table code under sanitizers, tests/hostsim/record_io.cpp the record I/O.
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

constexpr int MAX_AGENTS = 6;                  // LLE_SEARCH_MAX_AGENTS: 5^A joint actions fit 16 bits, the availability bytes two words
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

// A power of two >= max(2 cap, cap + chunk + 1): at most half full, with room for the candidates of one piece beside a full pool.
LLE_SEARCH_HD uint64_t table_slots(uint64_t cap, uint64_t chunk) {
    const uint64_t want = 2 * cap > cap + chunk + 1 ? 2 * cap : cap + chunk + 1;
    uint64_t slots = 8;
    while (slots < want) slots <<= 1;
    return slots;
}

// ---- record I/O: a batch as include/lle_hip.h describes its buffers (pointers to environment 0, strides in elements)
struct KeyView {  // the buffers that hold a state's identity, read only: all a lookup in somebody else's batch needs
    const uint8_t* pos;     // LLE_BUF_POS
    const uint64_t* bits;   // LLE_BUF_BITS
    const uint32_t* gems;   // LLE_BUF_GEMS
    const uint32_t* beams;  // LLE_BUF_BEAMS
    int64_t pos_stride, pos_agent_stride, beam_stride;
};
struct BatchView {
    uint8_t* pos;
    uint64_t* bits;
    uint32_t* gems;
    uint32_t* beams;
    uint8_t* avail;         // LLE_BUF_AVAIL
    uint8_t* actions;       // LLE_BUF_ACTIONS
    const uint8_t* err;     // LLE_BUF_ERR
    int64_t pos_stride, pos_agent_stride, beam_stride, avail_stride, act_stride;
    LLE_SEARCH_HD KeyView key() const { return KeyView{pos, bits, gems, beams, pos_stride, pos_agent_stride, beam_stride}; }
};

// Word w of the record in environment k: the identity words (w <= w_gems) from a KeyView, every word from a BatchView.
LLE_SEARCH_HD uint32_t env_word(const KeyView& v, const RecordLayout& r, int64_t k, int w) {
    if (w < r.n_pos) {
        uint32_t x = 0u;
        for (int b = 0; b < 4; b++) {
            const int byte = 4 * w + b;
            if (byte < 2 * r.A) x |= (uint32_t)v.pos[k * v.pos_stride + (byte >> 1) * v.pos_agent_stride + (byte & 1)] << (8 * b);
        }
        return x;
    }
    if (w == r.w_bits) return (uint32_t)v.bits[k];
    if (w == r.w_bits + 1) return (uint32_t)(v.bits[k] >> 32);
    if (w < r.w_gems) return v.beams[k * v.beam_stride + (w - r.w_beams)];
    return v.gems[k];
}
LLE_SEARCH_HD uint32_t env_word(const BatchView& v, const RecordLayout& r, int64_t k, int w) {
    if (w <= r.w_gems) return env_word(v.key(), r, k, w);
    uint32_t x = 0u;
    for (int b = 0; b < 4; b++) {
        const int a = 4 * (w - r.w_avail) + b;
        if (a < r.A) x |= (uint32_t)v.avail[k * v.avail_stride + a] << (8 * b);
    }
    return x;
}
struct EnvRecord {  // the record in environment k, as the functor hash_record and same_record read
    const BatchView& v;
    const RecordLayout& r;
    int64_t k;
    LLE_SEARCH_HD uint32_t operator()(int w) const { return env_word(v, r, k, w); }
};
// State s of a pool stored as structure of arrays: word w at base[w * stride + s] (a wavefront's reads of word w are as dense as its
// state indices).  One pool: (pool, max_states).  A map's segment of the forest's: (pool + map * n_words * cap, cap).
struct PoolRecord {
    const uint32_t* base;
    uint64_t stride, s;
    LLE_SEARCH_HD uint32_t operator()(int w) const { return base[(uint64_t)w * stride + s]; }
};

// One work item: the record `rec` with the joint action `code` (base 5, agent 0 the lowest digit) into environment k -- state, mask
// and action digits -- when every component is in the record's availability bytes.  Returns that; an unavailable item writes nothing.
template <class Record>
LLE_SEARCH_HD bool scatter_item(const BatchView& v, const RecordLayout& r, const Record& rec, int64_t k, uint32_t code) {
    const uint32_t av[2] = {rec(r.w_avail), r.n_av > 1 ? rec(r.w_avail + 1) : 0u};
    auto avail = [&](int a) { return (av[a >> 2] >> (8 * (a & 3))) & 255u; };
    if (!joint_available(code, r.A, avail)) return false;
    for (int w = 0; w < r.n_pos; w++) {
        const uint32_t x = rec(w);
        for (int b = 0; b < 4; b++) {
            const int byte = 4 * w + b;
            if (byte < 2 * r.A) v.pos[k * v.pos_stride + (byte >> 1) * v.pos_agent_stride + (byte & 1)] = (uint8_t)(x >> (8 * b));
        }
    }
    v.bits[k] = (uint64_t)rec(r.w_bits) | (uint64_t)rec(r.w_bits + 1) << 32;
    for (int w = 0; w < r.Lw; w++) v.beams[k * v.beam_stride + w] = rec(r.w_beams + w);
    v.gems[k] = rec(r.w_gems);
    for (int a = 0; a < r.A; a++) {
        v.avail[k * v.avail_stride + a] = (uint8_t)avail(a);
        v.actions[k * v.act_stride + a] = (uint8_t)(code % 5u);
        code /= 5u;
    }
    return true;
}

// The record in environment k into state idx of a pool (base, stride as PoolRecord's).
LLE_SEARCH_HD void copy_record(const BatchView& v, const RecordLayout& r, int64_t k, uint32_t* base, uint64_t stride, uint64_t idx) {
    for (int w = 0; w < r.n_words; w++) base[(uint64_t)w * stride + idx] = env_word(v, r, k, w);
}

template <class A, class B>
LLE_SEARCH_HD bool same_record(const A& a, const B& b, int n_key) {
    for (int w = 0; w < n_key; w++)
        if (a(w) != b(w)) return false;
    return true;
}

// Whom the occupant of a table slot may name: tag t < n_tags the candidate in environment env0 + t of `batch`, whose record lies
// complete there since the step; an index s < cap state s of the pool.  A finished table names states only: n_tags = 0.
struct Occupants {
    KeyView batch;
    int64_t env0;
    uint32_t n_tags;
    const uint32_t* pool;
    uint64_t stride, cap;
};
// Is `occupant` the record `me`, on its first r.n_key words?  (A tag or index out of range names nobody: no such occupant in a sound table.)
template <class Record>
LLE_SEARCH_HD bool occupant_is(const Occupants& o, const RecordLayout& r, uint32_t occupant, const Record& me) {
    if (occupant & TAG_BIT) {
        const uint32_t tag = occupant & ~TAG_BIT;
        if (tag >= o.n_tags) return false;
        const int64_t k = o.env0 + tag;
        return same_record([&](int w) { return env_word(o.batch, r, k, w); }, me, r.n_key);
    }
    if (occupant >= o.cap) return false;
    return same_record(PoolRecord{o.pool, o.stride, occupant}, me, r.n_key);
}

// ---- records with extra words.  A KIND of search carries EXTRA (<= MAX_EXTRA) more words of identity per record: the VALUE of the trajectory
// that reached the state, hashed and compared after the key words.  The words live only in the pool, as the arrays n_words ..
// n_words + EXTRA - 1 behind the record's: the batch has no buffer for them.  A kind says (PlainKind below; HelpKind of
// ../helpgraph/helpgraph_logic.hpp; TrailKind of ../trails/trails_logic.hpp; CycleKind of ../cycles/cycles_logic.hpp):
//   EXTRA, Value      the word count, and the value as the kernels keep it per candidate between insert and commit
//   state             the arcs of one state (`rec` its record, `cell` the map's cell table): all of it the value depends on
//   successor         the value of a successor with those arcs whose parent is record `parent` of the pool; false: no value, the
//                     run has no answer (the trail kind's walk ran out of budget)
//   violates, accepts does the mode drop a trajectory with this value; may a goal state with it end a plan
//   words             the value as ExtraWords
constexpr int MAX_EXTRA = 21;  // the cycle kind's larger agent class (../cycles/cycles_logic.hpp)
template <int EXTRA>
struct ExtraWords {
    static_assert(EXTRA >= 0 && EXTRA <= MAX_EXTRA, "a kind carries at most MAX_EXTRA words");
    uint32_t w[EXTRA > 0 ? EXTRA : 1];
    // Word i, i < EXTRA not known at compile time: selects over the words, which so stay in registers.
    LLE_SEARCH_HD uint32_t pick(int i) const {
        uint32_t v = w[0];
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 1; k < EXTRA; k++) v = i == k ? w[k] : v;
        return v;
    }
};
// The IDENTITY of a record: the n_key key words of `rec`, then the extra words.  What hash_record and same_record read, with n_key + EXTRA words.
template <class Record, int EXTRA>
struct KeyWithExtra {
    const Record& rec;
    int n_key;
    ExtraWords<EXTRA> x;
    LLE_SEARCH_HD uint32_t operator()(int w) const {
        if constexpr (EXTRA <= 2) return w < n_key ? rec(w) : EXTRA > 1 && w > n_key ? x.w[EXTRA > 1] : x.w[0];
        else return w < n_key ? rec(w) : x.pick(w - n_key);
    }
};
template <int EXTRA, class Record>
LLE_SEARCH_HD KeyWithExtra<Record, EXTRA> key_with_extra(const Record& rec, int n_key, const ExtraWords<EXTRA>& x) { return {rec, n_key, x}; }
struct PoolKey {  // the identity of pool record s: its key words, then the words from n_words on
    const uint32_t* pool;
    uint64_t stride, s;
    int n_key, n_words;
    LLE_SEARCH_HD uint32_t operator()(int w) const { return pool[(uint64_t)(w < n_key ? w : n_words + (w - n_key)) * stride + s]; }
};
template <int EXTRA>
LLE_SEARCH_HD ExtraWords<EXTRA> pool_extra(const uint32_t* pool, uint64_t stride, const RecordLayout& r, uint64_t s) {
    ExtraWords<EXTRA> x{};
    for (int i = 0; i < EXTRA; i++) x.w[i] = pool[(uint64_t)(r.n_words + i) * stride + s];
    return x;
}
template <int EXTRA>
LLE_SEARCH_HD void store_pool_extra(uint32_t* pool, uint64_t stride, const RecordLayout& r, uint64_t s, const ExtraWords<EXTRA>& x) {
    for (int i = 0; i < EXTRA; i++) pool[(uint64_t)(r.n_words + i) * stride + s] = x.w[i];
}

struct PlainKind {  // the plain search: no extra words, nothing dropped
    static constexpr int EXTRA = 0;
    using Value = uint32_t;
    template <class Record, class Cell> LLE_SEARCH_HD uint64_t state(const Record&, const RecordLayout&, const Cell&) const { return 0; }
    LLE_SEARCH_HD bool successor(const uint32_t*, uint64_t, const RecordLayout&, uint64_t, uint64_t, Value* value) const { return *value = 0u, true; }
    LLE_SEARCH_HD bool violates(Value, int) const { return false; }
    LLE_SEARCH_HD bool accepts(Value, int) const { return true; }
    static LLE_SEARCH_HD ExtraWords<0> words(Value) { return ExtraWords<0>{}; }
};

// The candidates of one tree in the piece in flight, and the pool they are compared with: tag t < n_tags names the candidate in
// environment env0 + t of `batch`, work item item0 + t of the tree's level, which expands record first_state + (item0 + t) / n_joint
// of `pool` (one pool: stride = cap = max_states; a map's segment of many: both the segment's length).  A tag at or past
// items - item0 names nobody.  One tree alone: env0 = 0, n_tags = the piece's items, and items = item0 + n_tags or ALL_ITEMS, which
// says the same without a second comparison in the kernel.
constexpr uint64_t ALL_ITEMS = ~0ull;
struct Piece {
    BatchView batch;
    int64_t env0;
    uint32_t n_tags;
    const uint32_t* pool;
    uint64_t stride, cap;
    uint64_t first_state, item0, items;
    uint32_t n_joint;
};
// The record candidate `tag` expands (may be >= cap for a tag that names nobody: the callers check).
LLE_SEARCH_HD uint64_t tag_parent(const Piece& o, uint32_t tag) { return o.first_state + (o.item0 + (uint64_t)tag) / o.n_joint; }
LLE_SEARCH_HD bool tag_in_piece(const Piece& o, uint32_t tag) { return tag < o.n_tags && o.item0 + (uint64_t)tag < o.items; }

// Is `occupant` the record `me` (a KeyWithExtra over the caller's own record, whose state has the arcs `arcs`)?  A tag's key words lie
// complete in the batch since the step; its extra words are not stored anywhere during the insert launch: they are worked out here,
// AGAIN, with the same function as by the lane that owns the candidate -- which found a value the mode keeps, or the tag would not be
// in the table.  Equal key words mean an equal state and so equal arcs: the caller's `arcs` are applied to the other candidate's own
// parent, which an earlier launch wrote.  No lane waits for another.
template <class Kind, class Me>
LLE_SEARCH_HD bool occupant_is(const Piece& o, const RecordLayout& r, const Kind& kind, uint64_t arcs, uint32_t occupant, const Me& me) {
    if (occupant & TAG_BIT) {
        const uint32_t tag = occupant & ~TAG_BIT;
        if (!tag_in_piece(o, tag)) return false;
        const EnvRecord other{o.batch, r, o.env0 + (int64_t)tag};
        if (!same_record(other, me, r.n_key)) return false;
        if constexpr (Kind::EXTRA > 0) {
            const uint64_t parent = tag_parent(o, tag);
            typename Kind::Value value;
            if (parent >= o.cap || !kind.successor(o.pool, o.stride, r, parent, arcs, &value)) return false;
            const ExtraWords<Kind::EXTRA> x = kind.words(value);
            for (int i = 0; i < Kind::EXTRA; i++)
                if (x.w[i] != me(r.n_key + i)) return false;
        }
        return true;
    }
    if (occupant >= o.cap) return false;
    return same_record(PoolKey{o.pool, o.stride, occupant, r.n_key, r.n_words}, me, r.n_key + Kind::EXTRA);
}

// bits_lo, gems: the words w_bits and w_gems of a record.  G = the map's gems.
LLE_SEARCH_HD bool is_goal(uint32_t bits_lo, uint32_t gems, const RecordLayout& r, bool collect_gems, int G) {
    return all_arrived(bits_lo, r.A) && (!collect_gems || all_gems(gems, G));
}

// Does an agent of the record `root` stand on a cell where a beam of another colour may run (foreign: H * W bytes, foreign_bit)?
LLE_SEARCH_HD bool root_on_foreign_beam(const uint32_t* root, const RecordLayout& r, const uint8_t* foreign, int H, int W) {
    for (int a = 0; a < r.A; a++) {
        const uint32_t ij = root[a >> 1] >> (16 * (a & 1));
        const int i = ij & 255u, j = (ij >> 8) & 255u;
        if (i < H && j < W && on_foreign_beam(foreign[i * W + j], a)) return true;
    }
    return false;
}

}  // namespace lle_search_logic
#endif  // LLE_SEARCH_LOGIC_HPP
