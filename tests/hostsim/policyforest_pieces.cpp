// policyforest_pieces.cpp -- the host/device-shared logic of the forest of steps-to-go tables (lle_amd/policyforest/
// policyforest_logic.hpp, over forest_logic.hpp and policy_logic.hpp) on the host, built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_policyforest_cpu.py and run as a child process.
//
// Checked: (1) over a relaxation level, every work item of every map that takes part is served by exactly one lane of exactly one
// piece, with the level found in the level-start array; a map that has converged, has no table or never expanded the level is served
// by none; the piece count is the least that does so -- for E in {1, 7, 64, 256}, 1 to 9 maps of different depths; (2) which maps take
// part in level d of a pass and when a map leaves the relaxation; (3) the map of an environment of a caller's batch for 1, 7, 211 and
// 2^20 environments per map, with 64-bit indices near the bounds; (4) what a lookup answers from a map's facts, a map over capacity
// included; (5) the relaxation itself, run lane by lane over a three-map forest of random graphs cut at a horizon, reaches the fixpoint
// of the restatement (tests/policy_ref.py: the smallest (steps, code) pair over the stored edges) whatever E is.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../lle_amd/policyforest/policyforest_logic.hpp"

namespace fl = lle_forest_logic;
namespace pl = lle_policy_logic;
namespace pfl = lle_policyforest_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static uint64_t levels = 0, lanes_total = 0, served_total = 0, passes_total = 0, answers_total = 0;
constexpr int CAPACITY = -20;  // LLE_POLICY_CAPACITY

// A forest after its exploration: per map the level starts, as lle_policyforest_build lays them out.
struct Forest {
    int64_t n_maps = 0, stride = 0;
    std::vector<pfl::MapFacts> facts;
    std::vector<pfl::MapPass> pass;
    std::vector<uint32_t> level_start;
};

static Forest make_forest(const std::vector<std::vector<uint32_t>>& starts, const std::vector<int>& status, uint64_t cap) {
    Forest f;
    f.n_maps = (int64_t)starts.size();
    uint32_t deepest = 0;
    for (int64_t m = 0; m < f.n_maps; m++) {
        const std::vector<uint32_t>& s = starts[(size_t)m];  // s[d] .. s[d + 1]: the states of depth d; one entry more than depths
        const uint32_t depth_reached = (uint32_t)s.size() - 2;
        const bool complete = s[s.size() - 1] == s[s.size() - 2];
        f.facts.push_back(pfl::make_facts(m, 9, cap, fl::table_slots(cap, 64), s.back(), complete, status[(size_t)m], depth_reached));
        deepest = std::max(deepest, f.facts.back().depth_reached);
        f.pass.push_back(pfl::MapPass{pfl::has_table(f.facts.back()) && f.facts.back().depth_reached > 0 ? 1u : 0u, 0u, 0u, 0u});
    }
    f.stride = (int64_t)deepest + 2;
    f.level_start.assign((size_t)(f.n_maps * f.stride), 0u);  // (sized exactly: a read past a map's row trips the sanitizer or the checks)
    for (int64_t m = 0; m < f.n_maps; m++)
        for (int64_t d = 0; d < f.stride; d++)
            f.level_start[(size_t)(m * f.stride + d)] = !pfl::has_table(f.facts[(size_t)m]) ? 0u
                                                        : (size_t)d < starts[(size_t)m].size() ? starts[(size_t)m][(size_t)d]
                                                                                               : f.facts[(size_t)m].n_states;
    return f;
}

// ---- (1), (2): one level of one pass
static void one_level(const Forest& f, int64_t E, uint32_t level, uint32_t n_joint, const std::vector<std::vector<uint32_t>>& starts) {
    std::vector<std::vector<uint8_t>> served((size_t)f.n_maps);
    uint64_t need = 0, want_items = 0;
    for (int64_t m = 0; m < f.n_maps; m++) {
        const pfl::MapFacts& facts = f.facts[(size_t)m];
        const bool takes_part = f.pass[(size_t)m].relaxing && facts.status == 0 && level < facts.depth_reached;
        CHECK(pfl::relaxes_at(facts, f.pass[(size_t)m], level) == takes_part);
        const uint64_t items = takes_part ? (uint64_t)(starts[(size_t)m][level + 1] - starts[(size_t)m][level]) * n_joint : 0u;
        CHECK(pfl::relax_items(facts, f.pass[(size_t)m], f.level_start.data(), f.stride, m, level, n_joint) == items);
        served[(size_t)m].assign((size_t)items, 0);  // (sized exactly: a lane past the items trips the sanitizer)
        need = std::max<uint64_t>(need, (items + (uint64_t)E - 1) / (uint64_t)E);
        want_items += items;
    }
    uint64_t items = 0, busy = 0;
    const uint64_t pieces = pfl::relax_piece_count(f.facts.data(), f.pass.data(), f.level_start.data(), f.stride, f.n_maps, E, level, n_joint, &items);
    CHECK(pieces == need && items == want_items);
    for (uint64_t q = 0; q < pieces; q++)
        for (int64_t k = 0; k < f.n_maps * E; k++) {
            const pfl::RelaxWork w = pfl::relax_work(k, q, E, level, n_joint, f.facts.data(), f.pass.data(), f.level_start.data(), f.stride);
            CHECK(w.map == k / E && w.local == k % E && w.item == q * (uint64_t)E + (uint64_t)(k % E));
            if (w.idle) continue;
            served[(size_t)w.map].at((size_t)w.item)++;
            busy++;
            const uint32_t s = w.first_state + (uint32_t)(w.item / n_joint);  // as the kernels compute it
            CHECK(w.first_state == starts[(size_t)w.map][level] && s < starts[(size_t)w.map][level + 1] && s < f.facts[(size_t)w.map].n_states);
        }
    for (int64_t m = 0; m < f.n_maps; m++)
        for (uint8_t count : served[(size_t)m]) CHECK(count == 1);
    CHECK(busy == items);
    levels++;
    lanes_total += pieces * (uint64_t)(f.n_maps * E);
    served_total += busy;
}

static std::vector<uint32_t> random_starts(std::mt19937_64& rng, int depth, bool complete, uint32_t widest) {
    std::vector<uint32_t> s{0u, 1u};
    for (int d = 1; d <= depth; d++) s.push_back(s.back() + (d == depth && complete ? 0u : 1u + (uint32_t)(rng() % widest)));
    return s;
}

static void ragged_passes(unsigned seed) {
    std::mt19937_64 rng(seed);
    const int64_t sizes[4] = {1, 7, 64, 256};
    for (int64_t E : sizes)
        for (int round = 0; round < 16; round++) {
            const int n_maps = 1 + (int)(rng() % 9);
            const uint32_t n_joint = round % 3 == 0 ? 1u : round % 3 == 1 ? 5u : 25u;
            std::vector<std::vector<uint32_t>> starts;
            std::vector<int> status;
            for (int m = 0; m < n_maps; m++) {
                starts.push_back(random_starts(rng, (int)(rng() % 7), rng() % 2 == 0, E == 1 ? 6u : (uint32_t)(2 * E / n_joint + 3)));  // depth 0: nothing expanded
                status.push_back(rng() % 6 == 0 ? CAPACITY : 0);
            }
            Forest f = make_forest(starts, status, 1u << 16);
            for (int m = 0; m < n_maps; m++) {
                const pfl::MapFacts& facts = f.facts[(size_t)m];
                CHECK(pfl::has_table(facts) == (status[(size_t)m] == 0));
                CHECK(f.pass[(size_t)m].relaxing == (status[(size_t)m] == 0 && starts[(size_t)m].size() > 2 ? 1u : 0u));
                if (status[(size_t)m] != 0) CHECK(facts.n_states == 0 && facts.complete == 0 && facts.depth_reached == 0);
            }
            // passes: every map that still relaxes is walked from the deepest level down; a random half of them converges per pass
            for (int pass = 0; pass < 6; pass++) {
                const uint32_t top = pfl::relax_depth(f.facts.data(), f.pass.data(), f.n_maps);
                uint32_t want_top = 0;
                for (int m = 0; m < n_maps; m++)
                    if (f.pass[(size_t)m].relaxing) want_top = std::max(want_top, f.facts[(size_t)m].depth_reached);
                CHECK(top == want_top);
                if (top == 0) break;
                for (uint32_t d = top; d-- > 0u;) one_level(f, E, d, n_joint, starts);
                for (int m = 0; m < n_maps; m++) {
                    pfl::MapPass& p = f.pass[(size_t)m];
                    const bool was = p.relaxing != 0u, moved = rng() % 2 == 0;
                    p.changed = was && moved ? 1u : 0u;
                    CHECK(pfl::next_pass(p) == (was && moved) && p.changed == 0u && (p.relaxing != 0u) == (was && moved));
                }
                passes_total++;
            }
        }
    // a map that is not relaxing stays out whatever its flag says; a level at or past depth_reached is nobody's
    pfl::MapFacts facts = pfl::make_facts(0, 9, 64, 256, 10, false, 0, 3);
    pfl::MapPass idle{0u, 1u, 0u, 0u}, busy{1u, 0u, 0u, 0u};
    CHECK(!pfl::next_pass(idle) && idle.relaxing == 0u && idle.changed == 0u);
    CHECK(!pfl::relaxes_at(facts, idle, 0) && pfl::relaxes_at(facts, busy, 2) && !pfl::relaxes_at(facts, busy, 3));
}

// ---- (3): the map of an environment of a caller's batch
static void lookup_maps() {
    const int64_t sizes[4] = {1, 7, 211, (int64_t)1 << 20};
    for (int64_t E : sizes)
        for (int64_t n_maps : {(int64_t)1, (int64_t)16, (int64_t)256, (int64_t)1024}) {
            const int64_t n = n_maps * E;
            for (int64_t m : {(int64_t)0, n_maps / 2, n_maps - 1}) {
                CHECK(pfl::lookup_map(m * E, n, E, -1) == m && pfl::lookup_map(m * E + E - 1, n, E, -1) == m);
                if (m > 0) CHECK(pfl::lookup_map(m * E - 1, n, E, -1) == m - 1);
                CHECK(pfl::lookup_map(m * E, n, E, 5) == 5);  // a single-map batch: the map the caller names
            }
        }
    // past 32 bits of environment arithmetic: 2^13 maps of 2^20 environments
    const int64_t E = (int64_t)1 << 20, n = E << 13;
    CHECK(n == (int64_t)1 << 33 && pfl::lookup_map(n - 1, n, E, -1) == 8191 && pfl::lookup_map(((int64_t)1 << 32) + 5, n, E, -1) == 4096);
    CHECK(pfl::lookup_map(((int64_t)1 << 32) - 1, n, E, -1) == 4095 && pfl::lookup_map((int64_t)1 << 32, n, E, -1) == 4096);
    CHECK(pfl::lookup_map(((int64_t)1 << 31) - 2, ((int64_t)1 << 31) - 1, 1, -1) == ((int64_t)1 << 31) - 2);
    CHECK(pfl::lookup_map(0xFFFFFFFEll, 0xFFFFFFFFll, 1, -1) == 0xFFFFFFFEll);           // the last batch that takes the 32-bit division
    CHECK(pfl::lookup_map(0xFFFFFFFFll, 0x100000000ll, 1, -1) == 0xFFFFFFFFll);          // the first that does not
    CHECK(pfl::lookup_map(0xFFFFFFFFll, 0x100000000ll, 2, -1) == 0x7FFFFFFFll);
    // a map's segments: map 255 of pools of 2^30 states of 40 words
    const uint64_t cap = (uint64_t)1 << 30;
    const pfl::MapFacts far = pfl::make_facts(255, 40, cap, (uint64_t)1 << 31, (uint32_t)cap, true, 0, 7);
    CHECK(far.pool_offset == (uint64_t)255 * 40 * cap && far.pool_offset > ((uint64_t)1 << 43));
    CHECK(far.state_offset == 255 * cap && far.table_offset == (uint64_t)255 << 31 && far.n_states == cap && far.complete == 1 && far.depth_reached == 7);
    CHECK(far.state_offset + (far.n_states - 1) == 256 * cap - 1);
    CHECK(sizeof(pfl::MapFacts) == 40 && sizeof(pfl::MapPass) == 16);
}

// ---- (4): the answer rule per map
static void answers() {
    const uint32_t stay = pl::stay_code(2);
    const pfl::MapFacts cut = pfl::make_facts(0, 9, 64, 256, 40, false, 0, 6), whole = pfl::make_facts(1, 9, 64, 256, 40, true, 0, 9);
    const pfl::MapFacts over = pfl::make_facts(2, 9, 64, 256, 64, true, CAPACITY, 4);
    CHECK(pfl::has_table(cut) && pfl::has_table(whole) && !pfl::has_table(over) && over.n_states == 0 && over.status == CAPACITY);
    for (uint32_t depth = 0; depth <= 6; depth++)
        for (uint32_t steps = 0; steps <= 8; steps++) {
            const uint32_t v = pl::pack_value(steps, 7u);
            CHECK(pfl::map_answer(cut, true, v, depth, 6) == (depth + steps <= 6 ? (int32_t)steps : pl::ANSWER_UNKNOWN));  // the exactness rule
            CHECK(pfl::map_answer(whole, true, v, depth, 6) == (int32_t)steps);                                          // complete: always exact
            CHECK(pfl::map_answer(over, true, v, depth, 6) == pl::ANSWER_UNKNOWN);                                        // over capacity: no table
            CHECK(pfl::map_answer(cut, false, v, depth, 6) == pl::ANSWER_UNKNOWN && pfl::map_answer(whole, false, v, depth, 6) == pl::ANSWER_UNKNOWN);
            answers_total += 5;
        }
    CHECK(pfl::map_answer(cut, true, pl::NO_PLAN, 2, 6) == pl::ANSWER_UNKNOWN && pfl::map_answer(whole, true, pl::NO_PLAN, 2, 6) == pl::ANSWER_DEAD_END);
    CHECK(pfl::map_answer(over, true, pl::NO_PLAN, 2, 6) == pl::ANSWER_UNKNOWN && pfl::map_answer(over, false, pl::NO_PLAN, 0, 6) == pl::ANSWER_UNKNOWN);
    CHECK(pl::value_code(pl::pack_value(0u, stay)) == 24u);
    const pfl::MapFacts empty = pfl::make_facts(3, 9, 64, 256, 0, false, 0, 0);  // (no build leaves a map without its reset state; such facts answer nothing)
    CHECK(!pfl::has_table(empty) && pfl::map_answer(empty, true, 0u, 0, 6) == pl::ANSWER_UNKNOWN);
}

// ---- (5): the relaxation on the host
struct Graph {                            // one map: the states in the order of their discovery, as the exploration stores them
    std::vector<uint32_t> depth;
    std::vector<uint8_t> goal;
    std::vector<std::vector<int64_t>> edge;  // edge[s][code]: the successor, -1: the joint action is unavailable, deadly or its successor is not stored
    std::vector<uint32_t> starts;
    bool complete = false;
};

static Graph random_graph(std::mt19937_64& rng, int n_nodes, uint32_t n_joint, int horizon, int goals) {
    std::vector<std::vector<int>> raw((size_t)n_nodes, std::vector<int>(n_joint, -1));
    for (auto& row : raw)
        for (auto& t : row) t = rng() % 3 == 0 ? -1 : (int)(rng() % (uint64_t)n_nodes);
    // breadth first from node 0 up to `horizon` levels: the order of discovery is the pool order, a level a contiguous range
    Graph g;
    std::vector<int> index((size_t)n_nodes, -1), order{0};
    index[0] = 0;
    g.depth.push_back(0);
    g.starts = {0u, 1u};
    int depth = 0;
    while (depth < horizon && g.starts[(size_t)depth + 1] > g.starts[(size_t)depth]) {
        for (uint32_t s = g.starts[(size_t)depth]; s < g.starts[(size_t)depth + 1]; s++)
            for (uint32_t c = 0; c < n_joint; c++) {
                const int t = raw[(size_t)order[s]][c];
                if (t >= 0 && index[(size_t)t] < 0) {
                    index[(size_t)t] = (int)order.size();
                    order.push_back(t);
                    g.depth.push_back((uint32_t)depth + 1);
                }
            }
        depth++;
        g.starts.push_back((uint32_t)order.size());
    }
    g.complete = g.starts[(size_t)depth + 1] == g.starts[(size_t)depth];
    g.goal.assign(order.size(), 0);
    for (int k = 0; k < goals; k++) g.goal[(size_t)(rng() % order.size())] = 1;
    g.edge.assign(order.size(), std::vector<int64_t>(n_joint, -1));
    for (size_t s = 0; s < order.size(); s++)
        if (g.depth[s] < (uint32_t)depth)  // an expanded state: every successor is stored
            for (uint32_t c = 0; c < n_joint; c++) {
                const int t = raw[(size_t)order[s]][c];
                g.edge[s][c] = t < 0 ? -1 : index[(size_t)t];
            }
    return g;
}

// The restatement's fixpoint (tests/policy_ref.py): the smallest (steps, code) pair over the stored edges, goals at (0, all-STAY).
static std::vector<uint32_t> fixpoint(const Graph& g, uint32_t n_joint, uint32_t stay) {
    std::vector<uint32_t> value(g.depth.size(), pl::NO_PLAN);
    for (size_t s = 0; s < value.size(); s++)
        if (g.goal[s]) value[s] = pl::pack_value(0u, stay);
    for (bool changed = true; changed;) {
        changed = false;
        for (size_t s = value.size(); s-- > 0;)
            for (uint32_t c = 0; c < n_joint; c++) {
                const int64_t t = g.edge[s][c];
                if (t < 0 || value[(size_t)t] == pl::NO_PLAN) continue;
                const uint32_t cand = pl::pack_value(pl::value_steps(value[(size_t)t]) + 1u, c);
                if (cand < value[s]) value[s] = cand, changed = true;
            }
    }
    return value;
}

static void relaxation(unsigned seed) {
    std::mt19937_64 rng(seed);
    const uint32_t n_joint = 5, stay = 4;
    for (int round = 0; round < 12; round++) {
        // three maps: one cut at the horizon, one that runs empty early (a small graph), one without a goal or over capacity
        const int horizon = 3 + round % 4;
        std::vector<Graph> maps{random_graph(rng, 60, n_joint, horizon, 2), random_graph(rng, 6, n_joint, horizon, 1), random_graph(rng, 40, n_joint, horizon, 0)};
        std::vector<int> status{0, 0, round % 2 ? CAPACITY : 0};
        std::vector<std::vector<uint32_t>> starts;
        uint64_t cap = 0;
        for (const Graph& g : maps) {
            starts.push_back(g.starts);
            cap = std::max<uint64_t>(cap, g.depth.size());
        }
        CHECK(maps[1].complete || maps[1].depth.size() <= 6);
        for (int64_t E : {(int64_t)1, (int64_t)7, (int64_t)64}) {
            Forest f = make_forest(starts, status, cap);
            std::vector<uint32_t> value((size_t)(3 * cap), pl::NO_PLAN);  // [n_maps][cap], as the library's
            for (size_t m = 0; m < 3; m++) {
                CHECK(f.facts[m].state_offset == m * cap);
                for (size_t s = 0; s < maps[m].depth.size(); s++)
                    if (maps[m].goal[s]) value[m * cap + s] = pl::pack_value(0u, stay);
            }
            std::vector<int> passes(3, 0);
            for (uint32_t top = pfl::relax_depth(f.facts.data(), f.pass.data(), 3); top > 0u; top = pfl::relax_depth(f.facts.data(), f.pass.data(), 3)) {
                for (uint32_t d = top; d-- > 0u;) {
                    const uint64_t pieces = pfl::relax_piece_count(f.facts.data(), f.pass.data(), f.level_start.data(), f.stride, 3, E, d, n_joint, nullptr);
                    for (uint64_t q = 0; q < pieces; q++)
                        for (int64_t k = 0; k < 3 * E; k++) {  // pf_relax, lane k
                            const pfl::RelaxWork w = pfl::relax_work(k, q, E, d, n_joint, f.facts.data(), f.pass.data(), f.level_start.data(), f.stride);
                            if (w.idle) continue;
                            const Graph& g = maps[(size_t)w.map];
                            const uint32_t s = w.first_state + (uint32_t)(w.item / n_joint), code = (uint32_t)(w.item % n_joint);
                            CHECK(g.depth.at(s) == d);
                            const int64_t succ = g.edge.at(s)[code];
                            if (succ < 0) continue;
                            uint32_t* v = value.data() + f.facts[(size_t)w.map].state_offset;
                            bool saturated = false;
                            const uint32_t offer = pl::relaxed_value(v[succ], code, &saturated);
                            CHECK(!saturated);
                            if (offer == pl::NO_PLAN || v[s] <= offer) continue;
                            v[s] = offer;
                            f.pass[(size_t)w.map].changed = 1u;
                        }
                }
                for (size_t m = 0; m < 3; m++) {
                    if (!f.pass[m].relaxing) continue;
                    passes[m]++;
                    pfl::next_pass(f.pass[m]);
                }
                passes_total++;
            }
            for (size_t m = 0; m < 3; m++) {
                const std::vector<uint32_t> want = fixpoint(maps[m], n_joint, stay);
                const bool relaxed = status[m] == 0 && maps[m].starts.size() > 2;
                CHECK(passes[m] >= (relaxed ? 1 : 0) && (relaxed || passes[m] == 0));
                for (size_t s = 0; s < want.size(); s++) {
                    if (status[m] == 0) CHECK(value[m * cap + s] == want[s]);
                    // and what a lookup makes of it
                    const int32_t answer = pfl::map_answer(f.facts[m], true, value[m * cap + s], maps[m].depth[s], horizon);
                    if (status[m] != 0) CHECK(answer == pl::ANSWER_UNKNOWN);
                    else if (want[s] == pl::NO_PLAN) CHECK(answer == (maps[m].complete ? pl::ANSWER_DEAD_END : pl::ANSWER_UNKNOWN));
                    else CHECK(answer == (maps[m].complete || maps[m].depth[s] + pl::value_steps(want[s]) <= (uint32_t)horizon ? (int32_t)pl::value_steps(want[s]) : pl::ANSWER_UNKNOWN));
                    answers_total++;
                }
            }
        }
    }
}

int main(int argc, char** argv) {
    const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
    ragged_passes(seed);
    lookup_maps();
    answers();
    relaxation(seed);
    if (failures) {
        std::printf("FAILED %d checks\n", failures);
        return 1;
    }
    std::printf("OK levels=%llu lanes=%llu served=%llu passes=%llu answers=%llu\n", (unsigned long long)levels, (unsigned long long)lanes_total,
                (unsigned long long)served_total, (unsigned long long)passes_total, (unsigned long long)answers_total);
    return 0;
}
