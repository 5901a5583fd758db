// forest_pieces.cpp -- the host/device-shared logic of the forest search (lle_amd/forest/forest_logic.hpp) on the host, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_forest_cpu.py and run as a child process.
//
// Checked: (1) over a level, every work item of every active map is served by exactly one lane of exactly one piece, a stopped map is
// served by none, the piece count is the least that does so and the occupancy numerator is the number of served lanes -- for E in
// {1, 7, 64, 256}, 1 to 9 maps and ragged frontier sizes, zero and one included; every served lane's frontier state lies inside the
// frontier; (2) lane, segment and item arithmetic just under 2^31 and beyond does not wrap; (3) the table segment is the power of two
// the header promises; (4) the descriptor of a level and the fate of a map follow from its counters as lle_search_run's do.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../lle_amd/forest/forest_logic.hpp"

namespace fl = lle_forest_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static uint64_t levels = 0, lanes_total = 0, served_total = 0;

// One level: frontier sizes per map (active[m] == 0: the map has stopped), n_joint joint actions per state.
static void one_level(int64_t E, const std::vector<uint64_t>& frontier, const std::vector<int>& active, uint32_t n_joint, uint64_t first_state) {
    const int64_t n_maps = (int64_t)frontier.size();
    std::vector<fl::MapDescriptor> desc((size_t)n_maps);
    std::vector<std::vector<uint8_t>> served((size_t)n_maps);
    for (int64_t m = 0; m < n_maps; m++) {
        fl::MapProgress p = fl::fresh_progress(active[(size_t)m] != 0);
        p.level_start = first_state + (uint64_t)m;
        p.level_end = p.level_start + frontier[(size_t)m];
        desc[(size_t)m] = fl::level_descriptor(p, n_joint);
        CHECK(desc[(size_t)m].items == (active[(size_t)m] ? frontier[(size_t)m] * n_joint : 0u));
        CHECK(desc[(size_t)m].first_state == (uint32_t)p.level_start);
        served[(size_t)m].assign((size_t)desc[(size_t)m].items, 0);  // (sized exactly: a lane past the items trips the sanitizer)
    }
    const uint64_t pieces = fl::piece_count(desc.data(), n_maps, E);
    uint64_t need = 0, busy = 0;
    for (int64_t m = 0; m < n_maps; m++) need = std::max<uint64_t>(need, (desc[(size_t)m].items + (uint64_t)E - 1) / (uint64_t)E);
    CHECK(pieces == need);
    for (uint64_t q = 0; q < pieces; q++)
        for (int64_t k = 0; k < n_maps * E; k++) {
            const fl::LaneWork w = fl::lane_work(k, q, E, desc.data());
            CHECK(w.map == k / E && w.map >= 0 && w.map < n_maps && w.local == k % E && fl::env_index(w.map, E, w.local) == k);
            if (w.idle) continue;
            CHECK(active[(size_t)w.map]);
            served[(size_t)w.map].at((size_t)w.item)++;
            busy++;
            const uint64_t s = desc[(size_t)w.map].first_state + w.item / n_joint;  // as the kernels compute it
            CHECK(s >= first_state + (uint64_t)w.map && s < first_state + (uint64_t)w.map + frontier[(size_t)w.map]);
        }
    for (int64_t m = 0; m < n_maps; m++)
        for (uint8_t count : served[(size_t)m]) CHECK(count == 1);
    CHECK(busy == fl::level_items(desc.data(), n_maps));
    levels++;
    lanes_total += pieces * (uint64_t)(n_maps * E);
    served_total += busy;
}

static void ragged_levels(unsigned seed) {
    std::mt19937_64 rng(seed);
    const int64_t sizes[4] = {1, 7, 64, 256};
    for (int64_t E : sizes)
        for (int round = 0; round < 24; round++) {
            const int n_maps = 1 + (int)(rng() % 9);
            const uint32_t n_joint = round % 3 == 0 ? 1u : round % 3 == 1 ? 5u : 25u;
            std::vector<uint64_t> frontier((size_t)n_maps);
            std::vector<int> active((size_t)n_maps);
            for (int m = 0; m < n_maps; m++) {
                const int kind = (int)(rng() % 6);
                const uint64_t limit = E == 1 ? 40 : (uint64_t)(3 * E + 5);
                frontier[(size_t)m] = kind == 0 ? 0 : kind == 1 ? 1 : 1 + rng() % (limit / n_joint + 1);
                active[(size_t)m] = rng() % 5 != 0;
            }
            if (round == 0) std::fill(active.begin(), active.end(), 0);         // nobody left: no piece
            if (round == 1) std::fill(frontier.begin(), frontier.end(), 0);      // every frontier empty
            if (round == 2) { std::fill(frontier.begin(), frontier.end(), 1); std::fill(active.begin(), active.end(), 1); }
            if (round == 3) frontier[0] = (uint64_t)E, active[0] = 1;            // exactly one full piece at n_joint = 1
            one_level(E, frontier, active, n_joint, 1 + rng() % 1000);
        }
}

static void large_indices() {
    const int64_t E = (int64_t)1 << 30;  // the largest block
    fl::MapDescriptor desc[2];
    desc[0] = {0u, 1u, 0u};
    desc[1] = {7u, 1u, ~(uint64_t)0};
    const int64_t k = ((int64_t)1 << 31) - 1;  // the last lane of two such maps
    const fl::LaneWork w = fl::lane_work(k, 3, E, desc);
    CHECK(w.map == 1 && w.local == E - 1 && !w.idle);
    CHECK(w.item == 3 * ((uint64_t)1 << 30) + (((uint64_t)1 << 30) - 1));     // 2^32 - 1: past 32 bits of lane arithmetic
    CHECK(fl::lane_work(E - 1, 0, E, desc).idle);                              // map 0 has no items
    CHECK(fl::env_index(1, E, E - 1) == k);
    CHECK(fl::env_index(((int64_t)1 << 20) - 1, 2048, 2047) == ((int64_t)1 << 31) - 1);
    CHECK(fl::env_index((int64_t)1 << 20, 2048, 0) == (int64_t)1 << 31);
    // 7 agents' worth would not fit, 6 do: a frontier just under 2^30 states times 15 625 joint actions
    fl::MapProgress p = fl::fresh_progress(true);
    p.level_start = 1;
    p.level_end = ((uint64_t)1 << 30);
    const fl::MapDescriptor d = fl::level_descriptor(p, 15625u);
    CHECK(d.items == (((uint64_t)1 << 30) - 1) * 15625u && d.items > ((uint64_t)1 << 43));
    desc[0] = d;
    desc[1].active = 0;
    CHECK(fl::piece_count(desc, 2, 256) == (d.items + 255) / 256);
    CHECK(fl::piece_count(desc, 2, E) == 15625u);  // ceil((2^30 - 1) * 15625 / 2^30)
    // segments: map 255 of pools of 2^30 states of 40 words
    const uint64_t cap = (uint64_t)1 << 30;
    CHECK(fl::pool_index(255, 40, 39, cap, cap - 1) == ((uint64_t)255 * 40 + 39) * cap + cap - 1);
    CHECK(fl::pool_index(255, 40, 39, cap, cap - 1) > ((uint64_t)1 << 43));
    CHECK(fl::pool_index(1, 8, 0, ((uint64_t)1 << 28) - 1, 0) == 8 * (((uint64_t)1 << 28) - 1));  // just under 2^31
    CHECK(fl::pool_index(1, 8, 0, (uint64_t)1 << 28, 5) == ((uint64_t)1 << 31) + 5);
    CHECK(fl::state_index(3, cap, cap - 1) == 4 * cap - 1 && fl::state_index(2, cap - 1, cap - 2) == 3 * cap - 4);
    CHECK(fl::table_base(3, (uint64_t)1 << 31) == (uint64_t)3 << 31);
    CHECK(fl::counter_index(((int64_t)1 << 28), 7) == ((uint64_t)1 << 31) + 7);
    CHECK(fl::foreign_base(((int64_t)1 << 16), 255, 255) == ((uint64_t)1 << 16) * 65025u);
}

static void table_sizes() {
    const uint64_t caps[] = {1, 2, 3, 64, 128, 1000, 65536, (uint64_t)1 << 30};
    const uint64_t blocks[] = {1, 7, 64, 256, 1024, 65536, (uint64_t)1 << 30};
    for (uint64_t cap : caps)
        for (uint64_t E : blocks) {
            const uint64_t slots = fl::table_slots(cap, E), want = std::max(2 * cap, cap + E + 1);
            CHECK(slots >= 8 && (slots & (slots - 1)) == 0 && slots >= want && (slots == 8 || slots / 2 < want));
            CHECK((slots <= fl::MAX_TABLE_SLOTS) == (cap + E + 1 <= fl::MAX_TABLE_SLOTS));  // (beyond it lle_forest_create refuses)
        }
    CHECK(fl::table_slots((uint64_t)1 << 30, (uint64_t)1 << 30) == (uint64_t)1 << 32 && fl::table_slots((uint64_t)1 << 30, ((uint64_t)1 << 30) - 1) == fl::MAX_TABLE_SLOTS);
    CHECK(fl::table_slots(128, 256) == 512 && fl::table_slots(65536, 256) == 131072 && fl::table_slots(1, 1) == 8);
}

static void fates() {
    const int CAPACITY = -20;
    uint64_t c[fl::N_COUNTERS] = {1, 0, fl::NO_GOAL, 0, 0, 0, 0, 0};
    int64_t fr = -1, ex = -1;
    fl::MapProgress p = fl::fresh_progress(true);
    CHECK(p.active && p.level_start == 0 && p.level_end == 1 && p.length == -1 && p.n_states == 1 && p.depth_reached == 0);
    CHECK(!fl::fresh_progress(false).active && fl::level_descriptor(fl::fresh_progress(false), 25).items == 0);
    CHECK(fl::level_descriptor(p, 25).items == 25 && fl::level_descriptor(p, 25).active == 1);
    // level 1: 9 available joint actions, 4 new states
    c[fl::CNT_STATES] = 5;
    c[fl::CNT_EXPANDED] = 9;
    CHECK(fl::advance(p, c, 100, 1, CAPACITY, 0, &fr, &ex) == fl::FATE_CONTINUE && fr == 4 && ex == 9 && p.active);
    CHECK(p.level_start == 1 && p.level_end == 5 && p.n_states == 5 && p.depth_reached == 1);
    CHECK(fl::level_descriptor(p, 25).first_state == 1 && fl::level_descriptor(p, 25).items == 100);
    // level 2: a goal among 7 new states -- the level is whole, the map stops
    c[fl::CNT_STATES] = 12;
    c[fl::CNT_EXPANDED] = 40;
    c[fl::CNT_GOAL] = 8;
    fl::MapProgress solved = p;
    CHECK(fl::advance(solved, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_SOLVED && fr == 7 && ex == 31);
    CHECK(!solved.active && solved.length == 2 && solved.goal == 8 && solved.n_states == 12 && solved.status == 0);
    CHECK(fl::level_descriptor(solved, 25).active == 0 && fl::level_descriptor(solved, 25).items == 0);
    // level 2 otherwise: nothing new -- the frontier ran empty at depth 2
    c[fl::CNT_STATES] = 5;
    c[fl::CNT_GOAL] = fl::NO_GOAL;
    fl::MapProgress empty = p;
    CHECK(fl::advance(empty, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_EMPTY && fr == 0 && ex == 31 && !empty.active && empty.length == -1);
    CHECK(empty.depth_reached == 2 && empty.n_states == 5);
    // the pool overflowed: by the flag, or by a counter past cap (the flag's launch may be the level's last)
    c[fl::CNT_STATES] = 12;
    c[fl::CNT_OVERFLOW] = 1;
    fl::MapProgress over = p;
    CHECK(fl::advance(over, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_CAPACITY && !over.active && over.status == CAPACITY && over.length == -1 && over.n_states == 100);
    c[fl::CNT_OVERFLOW] = 0;
    c[fl::CNT_STATES] = 101;
    c[fl::CNT_GOAL] = 3;  // a goal beside an overflow is no answer
    over = p;
    CHECK(fl::advance(over, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_CAPACITY && over.length == -1);
    c[fl::CNT_STATES] = 100;  // exactly full is no overflow
    over = p;
    CHECK(fl::advance(over, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_SOLVED && over.n_states == 100);
    c[fl::CNT_GOAL] = fl::NO_GOAL;
    c[fl::CNT_STEP_ERRORS] = 2;
    fl::MapProgress refused = p;
    CHECK(fl::advance(refused, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_STEP_ERROR && !refused.active);
    // a kind without a walk (dense_status 0) does not read the dense counter, whatever lies there
    c[fl::CNT_STEP_ERRORS] = 0;
    c[fl::CNT_DENSE] = 7;
    fl::MapProgress plain = p;
    CHECK(fl::advance(plain, c, 100, 2, CAPACITY, 0, &fr, &ex) == fl::FATE_CONTINUE && plain.status == 0 && plain.n_states == 100 && fr == 95);
    c[fl::CNT_DENSE] = 0;
    // counters near 2^31 and past it
    c[fl::CNT_STEP_ERRORS] = 0;
    fl::MapProgress big = fl::fresh_progress(true);
    big.level_start = 5;
    big.level_end = ((uint64_t)1 << 30) - 3;
    big.expanded_before = ((uint64_t)1 << 31) - 1;
    c[fl::CNT_STATES] = (uint64_t)1 << 30;
    c[fl::CNT_EXPANDED] = ((uint64_t)1 << 44) + 5;
    CHECK(fl::advance(big, c, (uint64_t)1 << 30, 9, CAPACITY, 0, &fr, &ex) == fl::FATE_CONTINUE && fr == 3);
    CHECK(ex == (int64_t)(((uint64_t)1 << 44) + 5 - (((uint64_t)1 << 31) - 1)) && big.level_start == ((uint64_t)1 << 30) - 3);
}

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    ragged_levels(seed);
    large_indices();
    table_sizes();
    fates();
    if (failures) {
        std::printf("FAILED %d checks\n", failures);
        return 1;
    }
    std::printf("OK levels=%llu lanes=%llu served=%llu\n", (unsigned long long)levels, (unsigned long long)lanes_total, (unsigned long long)served_total);
    return 0;
}
