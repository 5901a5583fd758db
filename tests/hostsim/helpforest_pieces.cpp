// helpforest_pieces.cpp -- the host/device-shared logic of the help forest (lle_amd/helpforest/helpforest_logic.hpp, over forest_logic.hpp,
// helpgraph_logic.hpp and trails_logic.hpp) on the host, built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_helpforest_cpu.py and run as a child process.
//
// Checked: (1) lane -> (map, environment, tag, parent) over ragged frontiers with E in {1, 7, 64, 256}: a served lane's tag is in the
// piece and its parent inside its map's frontier, an idle lane's tag names nobody; (2) a host simulation of hf_insert and hf_commit, both
// kinds, over a small synthetic forest of three maps that hold candidates with IDENTICAL key words in the same pieces, under different
// cell tables and edge rules: a table segment never matches a record of another map, a tag's extra words are worked out from the tag's
// own parent in its own segment, every map stores exactly the records a plain set gives for it alone; (3) per-map dense and capacity
// fates that leave the neighbours' progress alone.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "../../lle_amd/helpforest/helpforest_logic.hpp"

namespace sl = lle_search_logic;
namespace fl = lle_forest_logic;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;
namespace hfl = lle_helpforest_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static uint64_t lanes_checked = 0, records_stored = 0, tag_matches = 0, pool_matches = 0;

// ------------------------------------------------------------------------------------------------ (1) lanes
static void ragged_lanes(unsigned seed) {
    std::mt19937_64 rng(seed);
    const int64_t sizes[4] = {1, 7, 64, 256};
    for (int64_t E : sizes)
        for (int round = 0; round < 12; round++) {
            const int n_maps = 1 + (int)(rng() % 6);
            const uint32_t n_joint = round % 2 ? 25u : 125u;
            std::vector<fl::MapDescriptor> desc((size_t)n_maps);
            std::vector<uint64_t> frontier((size_t)n_maps);
            uint64_t first = 1 + rng() % 50;
            for (int m = 0; m < n_maps; m++) {
                fl::MapProgress p = fl::fresh_progress(rng() % 4 != 0);
                frontier[(size_t)m] = E == 1 ? rng() % 2 : rng() % 5;
                p.level_start = first + (uint64_t)m;
                p.level_end = p.level_start + frontier[(size_t)m];
                desc[(size_t)m] = fl::level_descriptor(p, n_joint);
            }
            const uint64_t pieces = fl::piece_count(desc.data(), n_maps, E);
            for (uint64_t q = 0; q < pieces; q++)
                for (int64_t k = 0; k < n_maps * E; k++) {
                    const fl::LaneWork w = fl::lane_work(k, q, E, desc.data());
                    const fl::MapDescriptor& d = desc[(size_t)w.map];
                    const sl::Piece piece{sl::BatchView{}, fl::env_index(w.map, E, 0), (uint32_t)E, nullptr, 1000, 1000, d.first_state, q * (uint64_t)E, d.items, n_joint};
                    const uint32_t tag = (uint32_t)w.local;
                    CHECK(piece.env0 + (int64_t)tag == k);  // the candidate a local tag names lies in the lane's own environment
                    CHECK(!sl::tag_in_piece(piece, (uint32_t)E));
                    if (w.idle) {
                        CHECK(!d.active || !sl::tag_in_piece(piece, tag));
                        continue;
                    }
                    CHECK(sl::tag_in_piece(piece, tag));
                    const uint64_t parent = sl::tag_parent(piece, tag);
                    CHECK(parent == d.first_state + w.item / n_joint);
                    CHECK(parent >= first + (uint64_t)w.map && parent < first + (uint64_t)w.map + frontier[(size_t)w.map]);
                    lanes_checked++;
                }
        }
}

// ------------------------------------------------------------------------------------------------ (2) insert and commit on the host
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

struct Forest {
    static constexpr int A = 2, H = 4, W = 4, N_MAPS = 3;
    int64_t E;
    uint64_t cap, slots;
    uint32_t n_joint = 25;
    sl::RecordLayout r = sl::make_layout(A, 1, false);
    std::vector<uint8_t> pos, avail, actions, err, valid;
    std::vector<uint64_t> bits, cand;
    std::vector<uint32_t> gems, beams, pool, parent, table, win, cells;
    std::vector<uint64_t> counters;
    std::vector<fl::MapDescriptor> desc;
    hl::EdgeRule rules[N_MAPS];
    sl::BatchView b{};

    Forest(int64_t E_, uint64_t cap_) : E(E_), cap(cap_), slots(fl::table_slots(cap_, (uint64_t)E_)) {
        const size_t lanes = (size_t)(N_MAPS * E);
        pos.assign(lanes * 4, 0);
        avail.assign(lanes * 2, 31);
        actions.assign(lanes * 2, 0);
        err.assign(lanes, 0);
        valid.assign(lanes, 0);
        bits.assign(lanes, 0);
        cand.assign(lanes, 0);
        gems.assign(lanes, 0);
        beams.assign(lanes, 0);
        win.assign(lanes, sl::SLOT_EMPTY);
        pool.assign((size_t)fl::pool_segment_offset(N_MAPS, r.n_words + hfl::EXTRA_WORDS, cap), 0xDEADBEEFu);
        parent.assign((size_t)N_MAPS * cap, 0);
        table.assign((size_t)N_MAPS * slots, sl::SLOT_EMPTY);
        counters.assign((size_t)N_MAPS * fl::N_COUNTERS, 0);
        desc.assign(N_MAPS, fl::MapDescriptor{});
        cells.assign((size_t)N_MAPS * H * W, 0u);
        // map 0: no laser tile at all; map 1: source 0 (agent 0's) along row 1, source 1 (agent 1's) along row 2; map 2: the same tiles,
        // the colours swapped
        for (int m = 1; m < N_MAPS; m++)
            for (int j = 0; j < W; j++) {
                cells[((size_t)m * H + 1) * W + j] = 1u;
                cells[((size_t)m * H + 2) * W + j] = 2u;
            }
        for (int m = 0; m < N_MAPS; m++) {
            rules[m].A = A;
            rules[m].H = H;
            rules[m].W = W;
            rules[m].enabled = 3u;
            for (int a = 0; a < sl::MAX_AGENTS; a++) rules[m].mine[a] = 0u;
            rules[m].mine[0] = m == 2 ? 2u : 1u;
            rules[m].mine[1] = m == 2 ? 1u : 2u;
        }
        b.pos = pos.data();
        b.bits = bits.data();
        b.gems = gems.data();
        b.beams = beams.data();
        b.avail = avail.data();
        b.actions = actions.data();
        b.err = err.data();
        b.pos_stride = 4;
        b.pos_agent_stride = 2;
        b.beam_stride = 1;
        b.avail_stride = 2;
        b.act_stride = 2;
    }
    uint32_t* segment(int64_t m) { return pool.data() + fl::pool_segment_offset(m, r.n_words + hfl::EXTRA_WORDS, cap); }
    const uint32_t* map_cells(int64_t m) const { return cells.data() + (size_t)m * H * W; }
    // what the "step" makes of joint action `code`: agent 0 in column 1, agent 1 in column 2, each in row 1 or 2 -- four states per map
    void write_env(int64_t k, uint32_t code) {
        pos[(size_t)k * 4 + 0] = (uint8_t)(1 + (code % 5u) % 2u);
        pos[(size_t)k * 4 + 1] = 1;
        pos[(size_t)k * 4 + 2] = (uint8_t)(1 + (code / 5u) % 2u);
        pos[(size_t)k * 4 + 3] = 2;
        bits[(size_t)k] = 3ull | 3ull << 32;  // both alive, both the occupants of their cells
    }
};

// hf_insert, lane k (kind help or trail; `param`: k of no-divergence, or N)
static void insert_lane(Forest& f, int kind, int mode, int param, uint64_t piece, int64_t k) {
    if (!f.valid[(size_t)k]) return;
    f.win[(size_t)k] = sl::SLOT_EMPTY;
    const int64_t map = k / f.E;
    const uint32_t local = (uint32_t)(k % f.E);
    uint64_t* counters = f.counters.data() + fl::counter_index(map, 0);
    if (counters[fl::CNT_OVERFLOW] != 0u) return;
    const sl::RecordLayout& r = f.r;
    const sl::EnvRecord rec{f.b, r, k};
    const fl::MapDescriptor d = f.desc[(size_t)map];
    const uint32_t* seg = f.segment(map);
    const sl::Piece who{f.b, fl::env_index(map, f.E, 0), (uint32_t)f.E, seg, f.cap, f.cap, d.first_state, piece * (uint64_t)f.E, d.items, f.n_joint};
    const uint64_t parent = sl::tag_parent(who, local);
    const uint32_t* cells = f.map_cells(map);
    auto cell = [&](int c) { return cells[c]; };
    const hl::EdgeRule& rule = f.rules[map];
    uint32_t* table = f.table.data() + fl::table_base(map, f.slots);
    int64_t slot;
    uint64_t extra;
    if (kind == hfl::KIND_HELP) {
        const hl::HelpKind help_kind{rule, mode, param};
        const uint64_t edges = help_kind.state(rec, r, cell);
        uint64_t help = 0;
        CHECK(help_kind.successor(seg, f.cap, r, parent, edges, &help));
        if (hl::violates(help, mode, param, r.A)) return;
        const auto me = hl::key_with_help(rec, r.n_key, help);
        auto same_as = [&](uint32_t occupant) {
            const bool same = sl::occupant_is(who, r, help_kind, edges, occupant, me);
            if (same) (occupant & sl::TAG_BIT ? tag_matches : pool_matches)++;
            return same;
        };
        slot = sl::table_insert(table, (uint32_t)(f.slots - 1), sl::hash_record(me, r.n_key + 2), sl::TAG_BIT | local, HostLoad{}, HostCas{}, same_as);
        extra = help;
    } else {
        const tl::TrailKind trail_kind{rule, param};
        const uint64_t edges = trail_kind.state(rec, r, cell);
        uint32_t trail = 0;
        if (!trail_kind.successor(seg, f.cap, r, parent, edges, &trail)) {
            counters[fl::CNT_DENSE]++;
            return;
        }
        if (tl::violates_sequence(trail, param, r.A)) return;
        const auto me = tl::key_with_trail(rec, r.n_key, trail);
        auto same_as = [&](uint32_t occupant) {
            const bool same = sl::occupant_is(who, r, trail_kind, edges, occupant, me);
            if (same) (occupant & sl::TAG_BIT ? tag_matches : pool_matches)++;
            return same;
        };
        slot = sl::table_insert(table, (uint32_t)(f.slots - 1), sl::hash_record(me, r.n_key + 1), sl::TAG_BIT | local, HostLoad{}, HostCas{}, same_as);
        extra = trail;
    }
    if (slot >= 0) {
        f.win[(size_t)k] = (uint32_t)slot;
        f.cand[(size_t)k] = extra;
    } else if (slot == sl::INSERT_FULL) {
        counters[fl::CNT_OVERFLOW] = 1;
    }
}

// hf_commit, lane k
static void commit_lane(Forest& f, int kind, uint64_t piece, int64_t k) {
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
    sl::copy_record(f.b, f.r, k, seg, f.cap, idx);
    if (kind == hfl::KIND_HELP) hl::store_pool_help(seg, f.cap, f.r, idx, f.cand[(size_t)k]);
    else tl::store_pool_trail(seg, f.cap, f.r, idx, (uint32_t)f.cand[(size_t)k]);
    const uint64_t item = piece * (uint64_t)f.E + (uint64_t)(k % f.E);
    f.parent[fl::state_index(map, f.cap, idx)] = f.desc[(size_t)map].first_state + (uint32_t)(item / f.n_joint);
    f.table[fl::table_base(map, f.slots) + slot] = (uint32_t)idx;
}

// One level of three maps with frontiers of 2, 3 and 1 records whose extra words differ from parent to parent; every map's stored
// records against a plain set of (position word, extra words) computed for that map alone.
static void simulated_level(int kind, int mode, int param, int64_t E, uint64_t cap) {
    Forest f(E, cap);
    const sl::RecordLayout& r = f.r;
    const uint64_t frontier[Forest::N_MAPS] = {2, 3, 1};
    const uint64_t first = 4;  // the frontier begins at record 4 of every segment
    for (int m = 0; m < Forest::N_MAPS; m++) {
        uint32_t* seg = f.segment(m);
        for (uint64_t s = first; s < first + frontier[m]; s++) {
            for (int w = 0; w < r.n_words; w++) seg[(uint64_t)w * cap + s] = 0u;  // (a parent's own state is never a candidate's)
            // parents with different pasts: help 0 -> 1 already there or not; trail L[0] = 1 or not
            if (kind == hfl::KIND_HELP) hl::store_pool_help(seg, cap, r, s, s % 2 ? (uint64_t)1 << 1 : 0ull);
            else tl::store_pool_trail(seg, cap, r, s, s % 2 ? 1u : 0u);
        }
        fl::MapProgress p = fl::fresh_progress(true);
        p.level_start = first;
        p.level_end = first + frontier[m];
        f.desc[(size_t)m] = fl::level_descriptor(p, f.n_joint);
        f.counters[fl::counter_index(m, fl::CNT_STATES)] = first + frontier[m];
        f.counters[fl::counter_index(m, fl::CNT_GOAL)] = fl::NO_GOAL;
    }
    const uint64_t pieces = fl::piece_count(f.desc.data(), Forest::N_MAPS, E);
    const int64_t lanes = Forest::N_MAPS * E;
    for (uint64_t q = 0; q < pieces; q++) {
        for (int64_t k = 0; k < lanes; k++) {  // hf_expand and the step
            const fl::LaneWork w = fl::lane_work(k, q, E, f.desc.data());
            f.valid[(size_t)k] = w.idle ? 0 : 1;
            if (!w.idle) f.write_env(k, (uint32_t)(w.item % f.n_joint));
        }
        for (int64_t k = 0; k < lanes; k++) insert_lane(f, kind, mode, param, q, k);
        for (int64_t k = 0; k < lanes; k++) commit_lane(f, kind, q, k);
    }
    bool any_overflow = false;
    for (int m = 0; m < Forest::N_MAPS; m++) {
        // the reference: this map alone, a plain set
        std::set<std::tuple<uint32_t, uint64_t>> want;
        const uint32_t* cells = f.map_cells(m);
        auto cell = [&](int c) { return cells[c]; };
        for (uint64_t s = first; s < first + frontier[m]; s++)
            for (uint32_t code = 0; code < f.n_joint; code++) {
                const uint32_t word = (1u + (code % 5u) % 2u) | 1u << 8 | (1u + (code / 5u) % 2u) << 16 | 2u << 24;
                const uint32_t words[3] = {word, 3u, 3u};
                const uint64_t edges = hl::state_edges([&](int w) { return words[w]; }, r, f.rules[m], cell);
                if (kind == hfl::KIND_HELP) {
                    const uint64_t help = (s % 2 ? (uint64_t)1 << 1 : 0ull) | edges;
                    if (!hl::violates(help, mode, param, r.A)) want.insert({word, help});
                } else {
                    int budget = tl::WALK_BUDGET;
                    const uint32_t trail = tl::layer_update(s % 2 ? 1u : 0u, edges, param, r.A, budget);
                    CHECK(budget >= 0);
                    if (!tl::violates_sequence(trail, param, r.A)) want.insert({word, trail});
                }
            }
        const uint64_t* c = f.counters.data() + fl::counter_index(m, 0);
        if (c[fl::CNT_OVERFLOW] != 0u || c[fl::CNT_STATES] > cap) {  // this map ran out of room: its neighbours must not have
            any_overflow = true;
            CHECK(first + frontier[m] + want.size() > cap);
            continue;
        }
        CHECK(c[fl::CNT_STATES] == first + frontier[m] + want.size());
        std::set<std::tuple<uint32_t, uint64_t>> got;
        const uint32_t* seg = f.segment(m);
        for (uint64_t idx = first + frontier[m]; idx < c[fl::CNT_STATES]; idx++) {
            const uint64_t extra = kind == hfl::KIND_HELP ? hl::pool_help(seg, cap, r, idx) : (uint64_t)tl::pool_trail(seg, cap, r, idx);
            CHECK(got.insert({seg[idx], extra}).second);  // no record twice
            // the extra words are those of the record's OWN parent in its OWN segment
            const uint64_t par = f.parent[fl::state_index(m, cap, idx)];
            CHECK(par >= first && par < first + frontier[m]);
            const uint32_t words[3] = {seg[idx], seg[cap + idx], seg[2 * cap + idx]};
            const uint64_t edges = hl::state_edges([&](int w) { return words[w]; }, r, f.rules[m], cell);
            if (kind == hfl::KIND_HELP) {
                CHECK(extra == (hl::pool_help(seg, cap, r, par) | edges));
            } else {
                int budget = tl::WALK_BUDGET;
                CHECK(extra == tl::layer_update(tl::pool_trail(seg, cap, r, par), edges, param, r.A, budget));
            }
            records_stored++;
        }
        CHECK(got == want);
        if (m == 0) CHECK(want.size() == 8u);  // no tiles, no edges: 4 states x 2 pasts
        // a finished segment names records of its own map only: no tag is left, no index past its counter
        for (uint64_t s = 0; s < f.slots; s++) {
            const uint32_t occupant = f.table[fl::table_base(m, f.slots) + s];
            CHECK(occupant == sl::SLOT_EMPTY || (!(occupant & sl::TAG_BIT) && occupant < c[fl::CNT_STATES] && occupant >= first + frontier[m]));
        }
    }
    CHECK(any_overflow == (cap == 12));  // (12: maps 0 and 1 run out of room, map 2 -- 5 records and at most 4 new ones -- does not)
}

// ------------------------------------------------------------------------------------------------ (3) fates
static void fates() {
    const int CAPACITY = -20, DENSE = -21;
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
    // capacity goes before dense, and isolates the same way
    fl::MapProgress q = fl::fresh_progress(true);
    c[1][fl::CNT_OVERFLOW] = 1;
    CHECK(fl::advance(q, c[1], 100, 1, CAPACITY, DENSE, &fr[1], &ex[1]) == fl::FATE_CAPACITY && q.status == CAPACITY && q.n_states == 100);
    c[1][fl::CNT_OVERFLOW] = 0;
    c[1][fl::CNT_STATES] = 101;
    q = fl::fresh_progress(true);
    CHECK(fl::advance(q, c[1], 100, 1, CAPACITY, DENSE, &fr[1], &ex[1]) == fl::FATE_CAPACITY);
    // a goal beside a dense item is no answer
    c[1][fl::CNT_STATES] = 7;
    c[1][fl::CNT_GOAL] = 6;
    q = fl::fresh_progress(true);
    CHECK(fl::advance(q, c[1], 100, 1, CAPACITY, DENSE, &fr[1], &ex[1]) == fl::FATE_DENSE && q.length == -1);
    c[1][fl::CNT_DENSE] = 0;
    q = fl::fresh_progress(true);
    CHECK(fl::advance(q, c[1], 100, 1, CAPACITY, DENSE, &fr[1], &ex[1]) == fl::FATE_SOLVED && q.length == 1 && q.goal == 6);
    // a map the mask leaves out
    const fl::MapProgress s = hfl::skipped_progress();
    CHECK(!s.active && s.length == -1 && s.n_states == 0 && s.depth_reached == 0 && s.status == 0 && fl::level_descriptor(s, 25).items == 0);
    CHECK(hfl::kind_of(hfl::NO_SEQUENCE) == hfl::KIND_TRAIL && hfl::kind_of(hl::NO_ASYMMETRIC) == hfl::KIND_HELP && hfl::NO_SEQUENCE == 6);
    CHECK(fl::pool_segment_offset(255, 40 + hfl::EXTRA_WORDS, (uint64_t)1 << 30) == (uint64_t)255 * 42 * ((uint64_t)1 << 30));
}

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    ragged_lanes(seed);
    for (int64_t E : {1, 7, 64, 256})
        for (uint64_t cap : {(uint64_t)64, (uint64_t)12}) {  // 12: map 1 (7 frontier records and more than 5 new ones) overflows alone
            simulated_level(hfl::KIND_HELP, hl::STANDARD, 2, E, cap);
            simulated_level(hfl::KIND_HELP, hl::NO_MUTUAL, 2, E, cap);
            simulated_level(hfl::KIND_TRAIL, hfl::NO_SEQUENCE, 3, E, cap);
            simulated_level(hfl::KIND_TRAIL, hfl::NO_SEQUENCE, 2, E, cap);
        }
    fates();
    if (failures) {
        std::printf("FAILED %d checks\n", failures);
        return 1;
    }
    std::printf("OK lanes=%llu records=%llu tag_matches=%llu pool_matches=%llu\n", (unsigned long long)lanes_checked, (unsigned long long)records_stored,
                (unsigned long long)tag_matches, (unsigned long long)pool_matches);
    return 0;
}
