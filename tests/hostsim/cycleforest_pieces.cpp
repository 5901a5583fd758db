// cycleforest_pieces.cpp -- what the insert and commit kernels of the cycle forest (lle_amd/cycleforest/cycleforest.hip) do, RESTATED on
// the host over the shared logic headers (cycles_logic.hpp: cl::CycleKind<3> and <21>; search_logic.hpp; forest_logic.hpp), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_cycleforest_cpu.py and run as a child process.  It does not include
// lle_amd/forest/forest_core.hpp (which needs HIP): insert_lane and commit_lane below are written after the core's insert_front,
// insert_back and commit, as in tests/hostsim/helpforest_pieces.cpp, and a change to those bodies is not seen here.
//
// Checked: (1) a small synthetic forest of three maps that hold candidates with IDENTICAL key words in the same pieces, under different
// cell tables and edge rules.  The lanes' work words are interleaved in ONE array laid out like the kernel's LDS (word i of a lane at
// i * WG + its number inside the workgroup, work_stride = WG lanes), the workgroups straddle maps (E = 7 and 1 beside 64), and every
// lane's footprint in that array is checked: CycleKind's strided words keep to the lane they were given, W words and nothing else.
// That cf_insert hands every lane threadIdx.x is NOT shown here: the GPU runs at E = 7 hold that.  A tag's value is worked out from
// the tag's own parent in its own segment, every map stores exactly the records a plain set gives for it alone; (2) per-map dense and
// capacity fates that leave the neighbours alone.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../../lle_amd/cycles/cycles_logic.hpp"
#include "../../lle_amd/helpforest/helpforest_logic.hpp"

namespace sl = lle_search_logic;
namespace fl = lle_forest_logic;
namespace hl = lle_helpgraph_logic;
namespace cl = lle_cycles_logic;
namespace hfl = lle_helpforest_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static uint64_t lanes_checked = 0, records_stored = 0, tag_matches = 0, pool_matches = 0, dropped_closed = 0;
constexpr int WG = 16;  // lanes of a simulated workgroup: no multiple of 7
constexpr uint32_t POISON = 0xA5A5A5A5u;

struct HostLoad {
    uint32_t operator()(const uint32_t* slot) const { return *slot; }
};
struct HostCas {
    uint32_t operator()(uint32_t* slot, uint32_t expected, uint32_t desired) const {
        const uint32_t seen = *slot;
        if (seen == expected) *slot = desired;
        return seen;
    }
};

// A batch of `lanes` environments of A agents on a 4 x 4 map, as include/lle_hip.h lays its buffers out.
struct Envs {
    int A;
    std::vector<uint8_t> pos, avail, actions, err;
    std::vector<uint64_t> bits;
    std::vector<uint32_t> gems, beams;
    sl::BatchView b{};
    Envs(int A_, size_t lanes) : A(A_) {
        pos.assign(lanes * 2 * (size_t)A, 0);
        avail.assign(lanes * (size_t)A, 31);
        actions.assign(lanes * (size_t)A, 0);
        err.assign(lanes, 0);
        bits.assign(lanes, 0);
        gems.assign(lanes, 0);
        beams.assign(lanes, 0);
        b.pos = pos.data();
        b.bits = bits.data();
        b.gems = gems.data();
        b.beams = beams.data();
        b.avail = avail.data();
        b.actions = actions.data();
        b.err = err.data();
        b.pos_stride = 2 * A;
        b.pos_agent_stride = 2;
        b.beam_stride = 1;
        b.avail_stride = A;
        b.act_stride = A;
    }
    // what the "step" makes of joint action `code`: agent a < 3 in column 1 + a, in row 1 or 2 by its digit; the others in row 0
    void write(int64_t k, uint32_t code) {
        for (int a = 0; a < A; a++) {
            pos[(size_t)k * 2 * A + 2 * a] = a < 3 ? (uint8_t)(1 + (code % 5u) % 2u) : 0;
            pos[(size_t)k * 2 * A + 2 * a + 1] = a < 3 ? (uint8_t)(1 + a) : (uint8_t)(a - 3);
            if (a < 3) code /= 5u;
        }
        const uint64_t all = sl::agents_mask(A);
        bits[(size_t)k] = all | all << 32;  // everybody alive, everybody the occupant of its cell
    }
};

template <int W>
struct Forest {
    static constexpr int A = W == cl::SMALL_WORDS ? 2 : 5, H = 4, Wd = 4, N_MAPS = 3;
    using Kind = cl::CycleKind<W>;
    int64_t E;
    uint64_t cap, slots;
    uint32_t n_joint = A == 2 ? 25u : 125u;
    sl::RecordLayout r = sl::make_layout(A, 1, false);
    Envs envs;
    std::vector<uint8_t> valid;
    std::vector<typename Kind::Value> cand;
    std::vector<uint32_t> pool, parent, table, win, cells, slabs;
    std::vector<uint64_t> counters;
    std::vector<fl::MapDescriptor> desc;
    hl::EdgeRule rules[N_MAPS];
    cl::Order order;

    Forest(int64_t E_, uint64_t cap_, int N) : E(E_), cap(cap_), slots(fl::table_slots(cap_, (uint64_t)E_)), envs(A, (size_t)(N_MAPS * E_)), order(cl::make_order(N)) {
        const size_t lanes = (size_t)(N_MAPS * E);
        valid.assign(lanes, 0);
        cand.assign(lanes, typename Kind::Value{});
        win.assign(lanes, sl::SLOT_EMPTY);
        pool.assign((size_t)fl::pool_segment_offset(N_MAPS, r.n_words + W, cap), 0xDEADBEEFu);
        parent.assign((size_t)N_MAPS * cap, 0);
        table.assign((size_t)N_MAPS * slots, sl::SLOT_EMPTY);
        counters.assign((size_t)N_MAPS * fl::N_COUNTERS, 0);
        desc.assign(N_MAPS, fl::MapDescriptor{});
        cells.assign((size_t)N_MAPS * H * Wd, 0u);
        slabs.assign((size_t)W * WG, POISON);  // exactly the kernel's W * lanes words: ASan sees a word past them
        // map 0: no laser tile at all; map 1: source 0 (agent 0's and agent 2's) along row 1, source 1 (agent 1's) along row 2; map 2:
        // the same tiles, the colours of agents 0 and 1 swapped
        for (int m = 1; m < N_MAPS; m++)
            for (int j = 0; j < Wd; j++) {
                cells[((size_t)m * H + 1) * Wd + j] = 1u;
                cells[((size_t)m * H + 2) * Wd + j] = 2u;
            }
        for (int m = 0; m < N_MAPS; m++) {
            rules[m].A = A;
            rules[m].H = H;
            rules[m].W = Wd;
            rules[m].enabled = 3u;
            for (int a = 0; a < sl::MAX_AGENTS; a++) rules[m].mine[a] = 0u;
            rules[m].mine[0] = m == 2 ? 2u : 1u;
            rules[m].mine[1] = m == 2 ? 1u : 2u;
            if (A > 2) rules[m].mine[2] = 1u;
        }
    }
    uint32_t* segment(int64_t m) { return pool.data() + fl::pool_segment_offset(m, r.n_words + W, cap); }
    const uint32_t* map_cells(int64_t m) const { return cells.data() + (size_t)m * H * Wd; }
    // the kind of map m with the work words of lane `in_group` of a workgroup (a plain array: base = it, stride 1)
    Kind kind_of(int64_t m, uint32_t* work, int32_t stride) const { return Kind(cl::CycleRule{rules[m], order, work, stride}); }
};

// The past of frontier record s: odd records have seen agent 0 help agent 1.
template <int W>
static typename cl::CycleKind<W>::Value past_of(const Forest<W>& f, int64_t m, uint64_t s) {
    uint32_t work[W] = {};
    typename cl::CycleKind<W>::Value v{};
    CHECK(f.kind_of(m, work, 1).update(cl::NoWords{}, s % 2 ? (uint64_t)1 << 1 : 0ull, f.r.A, &v) && !v.closed);
    return v;
}

// cf_insert<W>, lane k: forest_core.hpp's insert_front and insert_back
template <int W>
static void insert_lane(Forest<W>& f, uint64_t piece, int64_t k) {
    using Kind = cl::CycleKind<W>;
    if (!f.valid[(size_t)k]) return;
    f.win[(size_t)k] = sl::SLOT_EMPTY;
    const int64_t map = k / f.E;
    const uint32_t local = (uint32_t)(k % f.E);
    uint64_t* counters = f.counters.data() + fl::counter_index(map, 0);
    if (counters[fl::CNT_OVERFLOW] != 0u) return;
    const sl::RecordLayout& r = f.r;
    const sl::EnvRecord rec{f.envs.b, r, k};
    const fl::MapDescriptor d = f.desc[(size_t)map];
    const uint32_t* seg = f.segment(map);
    const sl::Piece who{f.envs.b, fl::env_index(map, f.E, 0), (uint32_t)f.E, seg, f.cap, f.cap, d.first_state, piece * (uint64_t)f.E, d.items, f.n_joint};
    const uint32_t* cells = f.map_cells(map);
    auto cell = [&](int c) { return cells[c]; };
    // the lane's slab: indexed by its number inside the WORKGROUP (threadIdx.x), whatever map it serves
    const int in_group = (int)(k % WG);
    std::fill(f.slabs.begin(), f.slabs.end(), POISON);
    const Kind kind = f.kind_of(map, f.slabs.data() + in_group, WG);
    const uint64_t arcs = kind.state(rec, r, cell);
    typename Kind::Value value;
    bool stored = false;
    if (!kind.successor(seg, f.cap, r, sl::tag_parent(who, local), arcs, &value)) {
        counters[fl::CNT_DENSE]++;
    } else if (kind.violates(value, r.A)) {
        dropped_closed++;
    } else {
        const auto me = sl::key_with_extra(rec, r.n_key, kind.words(value));
        auto same_as = [&](uint32_t occupant) {
            const bool same = sl::occupant_is(who, r, kind, arcs, occupant, me);
            if (same) (occupant & sl::TAG_BIT ? tag_matches : pool_matches)++;
            return same;
        };
        const int64_t slot = sl::table_insert(f.table.data() + fl::table_base(map, f.slots), (uint32_t)(f.slots - 1), sl::hash_record(me, r.n_key + Kind::EXTRA),
                                              sl::TAG_BIT | local, HostLoad{}, HostCas{}, same_as);
        if (slot >= 0) {
            f.win[(size_t)k] = (uint32_t)slot;
            f.cand[(size_t)k] = value;
            stored = true;
        } else if (slot == sl::INSERT_FULL) {
            counters[fl::CNT_OVERFLOW] = 1;
        }
    }
    (void)stored;
    // the footprint: the lane's own W words (the walk copies the parent's into them first), and nothing of a neighbour's
    for (int i = 0; i < W; i++)
        for (int l = 0; l < WG; l++)
            if (l != in_group) CHECK(f.slabs[(size_t)i * WG + l] == POISON);
    lanes_checked++;
}

// cf_commit<W>, lane k: forest_core.hpp's is_winner and commit
template <int W>
static void commit_lane(Forest<W>& f, uint64_t piece, int64_t k) {
    using Kind = cl::CycleKind<W>;
    if (!f.valid[(size_t)k]) return;
    const uint32_t slot = f.win[(size_t)k];
    if (slot == sl::SLOT_EMPTY) return;
    const int64_t map = k / f.E;
    uint64_t* counters = f.counters.data() + fl::counter_index(map, 0);
    const uint64_t idx = counters[fl::CNT_STATES]++;
    if (idx >= f.cap) {
        counters[fl::CNT_OVERFLOW] = 1;
        return;
    }
    uint32_t* seg = f.segment(map);
    sl::copy_record(f.envs.b, f.r, k, seg, f.cap, idx);
    sl::store_pool_extra(seg, f.cap, f.r, idx, Kind::words(f.cand[(size_t)k]));
    const uint64_t item = piece * (uint64_t)f.E + (uint64_t)(k % f.E);
    f.parent[fl::state_index(map, f.cap, idx)] = f.desc[(size_t)map].first_state + (uint32_t)(item / f.n_joint);
    f.table[fl::table_base(map, f.slots) + slot] = (uint32_t)idx;
}

// One level of three maps with frontiers of 2, 3 and 1 records whose pasts differ from parent to parent; every map's stored records
// against a plain set of (key words, value words) computed for that map alone.
template <int W>
static void simulated_level(int N, int64_t E, uint64_t cap, uint64_t small_cap) {
    using F = Forest<W>;
    using Kind = cl::CycleKind<W>;
    F f(E, cap, N);
    const sl::RecordLayout& r = f.r;
    const uint64_t frontier[F::N_MAPS] = {2, 3, 1};
    const uint64_t first = 4;  // the frontier begins at record 4 of every segment
    for (int m = 0; m < F::N_MAPS; m++) {
        uint32_t* seg = f.segment(m);
        for (uint64_t s = first; s < first + frontier[m]; s++) {
            for (int w = 0; w < r.n_words; w++) seg[(uint64_t)w * cap + s] = 0u;  // (a parent's own state is never a candidate's)
            sl::store_pool_extra(seg, cap, r, s, Kind::words(past_of(f, m, s)));
        }
        fl::MapProgress p = fl::fresh_progress(true);
        p.level_start = first;
        p.level_end = first + frontier[m];
        f.desc[(size_t)m] = fl::level_descriptor(p, f.n_joint);
        f.counters[fl::counter_index(m, fl::CNT_STATES)] = first + frontier[m];
        f.counters[fl::counter_index(m, fl::CNT_GOAL)] = fl::NO_GOAL;
    }
    const uint64_t pieces = fl::piece_count(f.desc.data(), F::N_MAPS, E);
    const int64_t lanes = F::N_MAPS * E;
    for (uint64_t q = 0; q < pieces; q++) {
        for (int64_t k = 0; k < lanes; k++) {  // cf_expand and the step
            const fl::LaneWork w = fl::lane_work(k, q, E, f.desc.data());
            f.valid[(size_t)k] = w.idle ? 0 : 1;
            if (!w.idle) f.envs.write(k, (uint32_t)(w.item % f.n_joint));
        }
        for (int64_t k = 0; k < lanes; k++) insert_lane(f, q, k);
        for (int64_t k = 0; k < lanes; k++) commit_lane(f, q, k);
    }
    bool any_overflow = false;
    for (int m = 0; m < F::N_MAPS; m++) {
        // the reference: this map alone, one environment, a plain array for the walk, a plain set
        std::set<std::vector<uint32_t>> want;
        const uint32_t* cells = f.map_cells(m);
        auto cell = [&](int c) { return cells[c]; };
        Envs one(F::A, 1);
        const sl::EnvRecord rec{one.b, r, 0};
        uint32_t work[W];
        const Kind alone = f.kind_of(m, work, 1);
        auto identity = [&](const typename Kind::Value& v) {
            std::vector<uint32_t> id;
            for (int w = 0; w < r.n_key; w++) id.push_back(rec(w));
            for (int i = 0; i < W; i++) id.push_back(v.w[i]);
            return id;
        };
        for (uint64_t s = first; s < first + frontier[m]; s++)
            for (uint32_t code = 0; code < f.n_joint; code++) {
                one.write(0, code);
                typename Kind::Value v;
                const typename Kind::Value past = past_of(f, m, s);
                CHECK(alone.update([&](int i) { return past.w[i]; }, alone.state(rec, r, cell), r.A, &v));
                if (!alone.violates(v, r.A)) want.insert(identity(v));
            }
        const uint64_t* c = f.counters.data() + fl::counter_index(m, 0);
        CHECK(c[fl::CNT_DENSE] == 0u);
        if (c[fl::CNT_OVERFLOW] != 0u || c[fl::CNT_STATES] > cap) {  // this map ran out of room: its neighbours must not have
            any_overflow = true;
            CHECK(first + frontier[m] + want.size() > cap);
            continue;
        }
        CHECK(c[fl::CNT_STATES] == first + frontier[m] + want.size());
        std::set<std::vector<uint32_t>> got;
        const uint32_t* seg = f.segment(m);
        for (uint64_t idx = first + frontier[m]; idx < c[fl::CNT_STATES]; idx++) {
            const sl::PoolKey key{seg, cap, idx, r.n_key, r.n_words};
            std::vector<uint32_t> id;
            for (int w = 0; w < r.n_key + W; w++) id.push_back(key(w));
            CHECK(got.insert(id).second);  // no record twice
            // the value is that of the record's OWN parent in its OWN segment, extended by the record's own state under the map's OWN rule
            const uint64_t par = f.parent[fl::state_index(m, cap, idx)];
            CHECK(par >= first && par < first + frontier[m]);
            typename Kind::Value v;
            CHECK(alone.successor(seg, cap, r, par, alone.state(sl::PoolRecord{seg, cap, idx}, r, cell), &v) && !v.closed);
            for (int i = 0; i < W; i++) CHECK(v.w[i] == id[(size_t)(r.n_key + i)]);
            records_stored++;
        }
        CHECK(got == want);
        if (m == 0) CHECK(want.size() == (F::A == 2 ? 8u : 16u));  // no tiles, no edges: 4 (8) states x 2 pasts
        // a finished segment names records of its own map only: no tag is left, no index past its counter
        for (uint64_t s = 0; s < f.slots; s++) {
            const uint32_t occupant = f.table[fl::table_base(m, f.slots) + s];
            CHECK(occupant == sl::SLOT_EMPTY || (!(occupant & sl::TAG_BIT) && occupant < c[fl::CNT_STATES] && occupant >= first + frontier[m]));
        }
    }
    CHECK(any_overflow == (cap == small_cap));
}

// ------------------------------------------------------------------------------------------------ (2) fates
static void fates() {
    const int CAPACITY = -20, DENSE = -21;  // LLE_CYCLES_CAPACITY, LLE_CYCLES_DENSE
    uint64_t c[3][fl::N_COUNTERS] = {};
    fl::MapProgress p[3];
    for (int m = 0; m < 3; m++) {
        p[m] = fl::fresh_progress(true);
        c[m][fl::CNT_STATES] = 5;
        c[m][fl::CNT_EXPANDED] = 9;
        c[m][fl::CNT_GOAL] = fl::NO_GOAL;
    }
    c[1][fl::CNT_DENSE] = 3;  // the middle map's walk ran out of budget
    int64_t fr[3] = {-1, -1, -1}, ex[3] = {-1, -1, -1};
    const int fate0 = fl::advance(p[0], c[0], 100, 1, CAPACITY, DENSE, &fr[0], &ex[0]);
    const int fate1 = fl::advance(p[1], c[1], 100, 1, CAPACITY, DENSE, &fr[1], &ex[1]);
    const int fate2 = fl::advance(p[2], c[2], 100, 1, CAPACITY, DENSE, &fr[2], &ex[2]);
    CHECK(fate0 == fl::FATE_CONTINUE && fate2 == fl::FATE_CONTINUE && fate1 == fl::FATE_DENSE);
    CHECK(!p[1].active && p[1].status == DENSE && p[1].length == -1 && p[1].n_states == 1 && p[1].depth_reached == 1 && fr[1] == -1);
    for (int m : {0, 2}) CHECK(p[m].active && p[m].status == 0 && p[m].n_states == 5 && fr[m] == 4 && ex[m] == 9 && p[m].level_start == 1 && p[m].level_end == 5);
    fl::MapProgress q = fl::fresh_progress(true);
    c[1][fl::CNT_OVERFLOW] = 1;  // capacity goes before dense, and isolates the same way
    CHECK(fl::advance(q, c[1], 100, 1, CAPACITY, DENSE, &fr[1], &ex[1]) == fl::FATE_CAPACITY && q.status == CAPACITY && q.n_states == 100);
    const fl::MapProgress s = hfl::skipped_progress();
    CHECK(!s.active && s.length == -1 && s.n_states == 0 && s.depth_reached == 0 && s.status == 0 && fl::level_descriptor(s, 125).items == 0);
    CHECK(cl::words_of(4) == cl::SMALL_WORDS && cl::words_of(5) == cl::LARGE_WORDS && cl::LARGE_WORDS <= sl::MAX_EXTRA);
    CHECK(fl::pool_segment_offset(255, 40 + cl::LARGE_WORDS, (uint64_t)1 << 30) == (uint64_t)255 * 61 * ((uint64_t)1 << 30));
}

int main() {
    for (int64_t E : {1, 7, 64}) {
        // (12: maps 0 and 1 run out of room under two agents, map 2 -- 5 records and at most 4 new ones -- does not)
        for (uint64_t cap : {(uint64_t)64, (uint64_t)12}) simulated_level<cl::SMALL_WORDS>(2, E, cap, 12);
        for (int N : {2, 3})
            for (uint64_t cap : {(uint64_t)256, (uint64_t)20}) simulated_level<cl::LARGE_WORDS>(N, E, cap, 20);
    }
    fates();
    if (failures) {
        std::printf("FAILED %d checks\n", failures);
        return 1;
    }
    std::printf("OK lanes=%llu records=%llu tag_matches=%llu pool_matches=%llu dropped_closed=%llu\n", (unsigned long long)lanes_checked,
                (unsigned long long)records_stored, (unsigned long long)tag_matches, (unsigned long long)pool_matches, (unsigned long long)dropped_closed);
    return 0;
}
