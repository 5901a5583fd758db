// cooptrails_logic.cpp -- the host-and-device logic of the temporal cooperation tracker (lle_amd/cooptrails/cooptrails_logic.hpp) on the
// host, built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_cooptrails_cpu.py.
//
//   * the wide layer_update, applied state after state, against a brute-force longest trail over the TEMPORAL edges (helper, beneficiary,
//     t) of seeded random graphs of 1 .. 16 agents and several layers; every fourth graph of 16 agents is shifted so that agent 15, bit 15
//     of a row and bits 60-63 of the value are in use
//   * episodes of fifteen and more small states whose true lengths pass 15: every field is min(true, 15), also BEYOND a trail of 15
//   * the known answers of tests/golden/kat_coop.json's longest_trail cases, which the test hands over as a text file (argv[2]): one case
//     per line, "expected n_edges  h b t  h b t ..."
//   * equality with lle_trails_logic::layer_update under N = 16 for up to 6 agents wherever no field reaches 15
//   * saturation: a mutual pair held over eight states; a 3-cycle inside one state, repeated: 3, 6, 9, 12, 15, 15
//   * the budget: the complete digraph on 4 agents sets dense and leaves a lower bound
//   * field_max against a loop over the fields
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../lle_amd/cooptrails/cooptrails_logic.hpp"
#include "../../lle_amd/trails/trails_logic.hpp"

namespace ct = lle_cooptrails_logic;
namespace tl = lle_trails_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

// ---- brute force: the longest trail that ends at each agent, over temporal edges
struct Edge {
    int h, b, t;
};
static void extend(const std::vector<Edge>& edges, int at, int time, uint64_t used, int len, int* best) {
    for (size_t k = 0; k < edges.size(); k++) {
        const Edge& e = edges[k];
        if (e.h != at || e.t < time || ((used >> k) & 1u)) continue;
        if (len + 1 > best[e.b]) best[e.b] = len + 1;
        extend(edges, e.b, e.t, used | (uint64_t)1 << k, len + 1, best);
    }
}
static void brute(const std::vector<Edge>& edges, int* best) {
    for (int a = 0; a < 16; a++) best[a] = 0;
    for (int a = 0; a < 16; a++) extend(edges, a, -1, 0, 0, best);
}
static ct::Arcs arcs_of(const std::vector<Edge>& edges, int t, int A) {
    uint32_t rows[16] = {0};
    for (const Edge& e : edges)
        if (e.t == t) rows[e.h] |= 1u << e.b;
    ct::Arcs arcs = ct::no_arcs();
    for (int h = 0; h < 16; h++) arcs = ct::with_bits(arcs, h, ct::clean_row(rows[h] | 0xFFFF0000u, h, A), true);  // (the high half of a stored row is dropped)
    return arcs;
}
static uint64_t narrow_arcs(const std::vector<Edge>& edges, int t) {
    uint64_t arcs = 0;
    for (const Edge& e : edges)
        if (e.t == t) arcs |= (uint64_t)1 << (8 * e.h + e.b);
    return arcs;
}
static uint64_t run_layers(const std::vector<Edge>& edges, int A, int T, bool* dense) {
    uint64_t L = 0ull;
    *dense = false;
    for (int t = 0; t <= T; t++) L = ct::layer_update(L, arcs_of(edges, t, A), A, dense);
    return L;
}
static uint64_t slow_field_max(uint64_t a, uint64_t b) {
    uint64_t out = 0ull;
    for (int f = 0; f < 16; f++) out |= (uint64_t)std::max(ct::field(a, f), ct::field(b, f)) << (4 * f);
    return out;
}

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937 rng(seed);
    std::mt19937_64 rng64(seed);
    long graphs = 0, fields = 0, agent15 = 0, bit15 = 0, top_bits = 0, same_as_narrow = 0, kat = 0, maxes = 0, chains = 0;
    int best[16];

    // ---- layer_update against the brute force
    for (int round = 0; round < 8000; round++) {
        const int A = 1 + (int)(rng() % 16u), T = (int)(rng() % 5u), n_edges = 1 + (int)(rng() % 10u);
        const int few = 2 + (int)(rng() % 4u);  // the edges among a few agents: they chain
        const int span = round % 2 ? std::min(few, A) : A;
        const int shift = (A == 16 && round % 4 == 1) ? 16 - span : 0;
        std::vector<Edge> edges;
        for (int k = 0; k < n_edges; k++) {
            Edge e{(int)(rng() % (uint32_t)span) + shift, (int)(rng() % (uint32_t)span) + shift, (int)(rng() % (uint32_t)(T + 1))};
            if (round % 5 == 0) e.t = 0;  // everything in one state: cycles inside a layer
            if (e.h == e.b) continue;
            bool dup = false;
            for (const Edge& o : edges) dup = dup || (o.h == e.h && o.b == e.b && o.t == e.t);
            if (!dup) edges.push_back(e);
        }
        brute(edges, best);
        bool dense = false;
        const uint64_t L = run_layers(edges, A, T, &dense);
        CHECK(!dense);  // at most 10 arcs in a state allow more than 4 096 extensions from one agent only when nearly all chain: none here
        if (dense) continue;
        for (int a = 0; a < 16; a++, fields++) CHECK((int)ct::field(L, a) == std::min(best[a], 15));
        CHECK((int)ct::longest(L) == std::min(*std::max_element(best, best + 16), 15));
        CHECK(A == 16 || (L >> (4 * A)) == 0ull);
        chains += *std::max_element(best, best + 16) >= 3;
        agent15 += best[15] > 0;
        top_bits += (L >> 60) != 0ull;
        for (const Edge& e : edges) bit15 += e.b == 15;
        // the narrow layer_update of the trail search: the same fields for up to 6 agents while nothing reaches 15
        if (A <= 6 && ct::longest(L) < 15u) {
            uint32_t N = 0u;
            bool narrow_dense = false;
            for (int t = 0; t <= T; t++) {
                int budget = tl::WALK_BUDGET;
                N = tl::layer_update(N, narrow_arcs(edges, t), 16, A, budget);
                narrow_dense = narrow_dense || budget < 0;
            }
            if (!narrow_dense) {
                CHECK((N & tl::REACHED) == 0u && (uint64_t)N == L);
                same_as_narrow++;
            }
        }
        graphs++;
    }
    CHECK(agent15 >= 20 && bit15 >= 20 && top_bits >= 20 && same_as_narrow >= 500 && chains >= 500);

    // ---- long episodes of small states: the true lengths pass 15, every field is min(true, 15)
    long saturated = 0, beyond = 0;
    for (int round = 0; round < 400; round++) {
        const int A = 2 + (int)(rng() % 2u), T = 14 + (int)(rng() % 8u);
        std::vector<Edge> edges;
        for (int t = 0; t <= T; t++) {
            const int n_arcs = 1 + (int)(rng() % 3u);
            for (int k = 0; k < n_arcs; k++) {
                Edge e{(int)(rng() % (uint32_t)A), (int)(rng() % (uint32_t)A), t};
                bool dup = e.h == e.b;
                for (const Edge& o : edges) dup = dup || (o.h == e.h && o.b == e.b && o.t == e.t);
                if (!dup) edges.push_back(e);
            }
        }
        if (edges.size() > 48) continue;
        brute(edges, best);
        bool dense = false;
        const uint64_t L = run_layers(edges, A, T, &dense);
        CHECK(!dense);
        for (int a = 0; a < 16; a++) {
            CHECK((int)ct::field(L, a) == std::min(best[a], 15));
            saturated += best[a] == 15;
            beyond += best[a] > 15;
        }
    }
    if (!(saturated >= 5 && beyond >= 20)) std::printf("saturated=%ld beyond=%ld\n", saturated, beyond);
    CHECK(saturated >= 5 && beyond >= 20);

    // ---- the known answers
    if (argc > 2) {
        std::FILE* f = std::fopen(argv[2], "r");
        CHECK(f != nullptr);
        int expected = 0, n = 0;
        while (f && std::fscanf(f, "%d %d", &expected, &n) == 2) {
            std::vector<Edge> edges((size_t)n);
            int T = 0;
            for (Edge& e : edges) {
                CHECK(std::fscanf(f, "%d %d %d", &e.h, &e.b, &e.t) == 3 && e.h >= 0 && e.h < 16 && e.b >= 0 && e.b < 16 && e.t >= 0);
                T = std::max(T, e.t);
            }
            edges.erase(std::remove_if(edges.begin(), edges.end(), [](const Edge& e) { return e.h == e.b; }), edges.end());  // self-loops are ignored
            bool dense = false;
            const uint64_t L = run_layers(edges, 16, T, &dense);
            CHECK(!dense && (int)ct::longest(L) == std::min(expected, 15));
            kat++;
        }
        if (f) std::fclose(f);
    }

    // ---- saturation
    {
        bool dense = false;
        ct::Arcs pair = ct::no_arcs();
        pair = ct::with_bits(pair, 14, 1u << 15, true);
        pair = ct::with_bits(pair, 15, 1u << 14, true);
        uint64_t L = 0ull;
        for (int state = 1; state <= 9; state++) {  // a mutual pair adds two edges to both trails per state
            L = ct::layer_update(L, pair, 16, &dense);
            const uint64_t want = (uint64_t)std::min(2 * state, 15);
            CHECK(L == (want << 56 | want << 60) && !dense);
        }
        ct::Arcs cycle = ct::no_arcs();
        cycle = ct::with_bits(cycle, 0, 1u << 1, true);
        cycle = ct::with_bits(cycle, 1, 1u << 2, true);
        cycle = ct::with_bits(cycle, 2, 1u << 0, true);
        L = 0ull;
        const int want[6] = {3, 6, 9, 12, 15, 15};
        for (int state = 0; state < 6; state++) {
            L = ct::layer_update(L, cycle, 3, &dense);
            CHECK(L == (uint64_t)want[state] * 0x111ull && !dense);
        }
        // beyond a saturated trail: 0 -> 1 reaches 15 inside the state and 1 -> 2 goes on from there -- agent 2 ends a trail of 16
        ct::Arcs chain = ct::with_bits(ct::with_bits(ct::no_arcs(), 0, 1u << 1, true), 1, 1u << 2, true);
        CHECK(ct::layer_update(0xEull, chain, 3, &dense) == 0xFFEull);
        // a saturated field next to others: one arc out of a 15 gives 15, nothing is carried into the neighbouring fields
        ct::Arcs one = ct::with_bits(ct::no_arcs(), 3, 1u << 5, true);
        CHECK(ct::layer_update(0xFull << 12, one, 6, &dense) == (0xFull << 12 | 0xFull << 20));
        CHECK(ct::layer_update(0xEull << 12 | 0x7ull << 16, one, 6, &dense) == (0xEull << 12 | 0x7ull << 16 | 0xFull << 20));
        CHECK(ct::layer_update(0x123456789ABCDEFull, ct::no_arcs(), 16, &dense) == 0x123456789ABCDEFull);  // no arcs: L as it is
        CHECK(!dense);
    }

    // ---- the budget: a complete digraph has a closed trail over all its arcs; on 4 agents (12 arcs) a walk cannot try them all
    {
        std::vector<Edge> edges;
        for (int h = 0; h < 4; h++)
            for (int b = 0; b < 4; b++)
                if (h != b) edges.push_back(Edge{h, b, 0});
        bool dense = false;
        const uint64_t L = ct::layer_update(0ull, arcs_of(edges, 0, 4), 4, &dense);
        CHECK(dense && (L >> 16) == 0ull);
        for (int a = 0; a < 4; a++) CHECK(ct::field(L, a) >= 4u && ct::field(L, a) <= 12u);
        // ... and on 3 agents (6 arcs) every walk finishes: exact
        edges.clear();
        for (int h = 0; h < 3; h++)
            for (int b = 0; b < 3; b++)
                if (h != b) edges.push_back(Edge{h, b, 0});
        dense = false;
        CHECK(ct::layer_update(0ull, arcs_of(edges, 0, 3), 3, &dense) == 0x666ull && !dense);
    }

    // ---- the field-wise maximum
    for (int round = 0; round < 20000; round++, maxes++) {
        uint64_t a = rng64(), b = rng64();
        if (round % 3 == 0) b = (b & 0xF0F0F0F00F0F0F0Full) | (a & ~0xF0F0F0F00F0F0F0Full);  // equal fields too
        CHECK(ct::field_max(a, b) == slow_field_max(a, b) && ct::field_max(b, a) == slow_field_max(a, b));
    }
    CHECK(ct::field_max(0ull, ~0ull) == ~0ull && ct::field_max(0xF000000000000000ull, 0x0ull) == 0xF000000000000000ull);

    if (failures) return 1;
    std::printf("OK saturated=%ld beyond=%ld graphs=%ld fields=%ld agent15=%ld bit15=%ld top_bits=%ld same_as_narrow=%ld chains=%ld kat=%ld maxes=%ld\n", saturated, beyond, graphs, fields, agent15, bit15,
                top_bits, same_as_narrow, chains, kat, maxes);
    return 0;
}
