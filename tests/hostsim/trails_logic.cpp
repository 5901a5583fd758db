// trails_logic.cpp -- the host-and-device logic of the trail search (lle_amd/trails/trails_logic.hpp) on the host, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_trails_cpu.py and checked against a brute-force longest-trail search.
//
//   * layer_update, applied state after state, against a brute-force search over the TEMPORAL edges (helper, beneficiary, t) of seeded
//     random graphs of 2 .. 6 agents: every field of L while no trail has N edges, and REACHED at the first state at which one has
//   * the known answers of tests/golden/kat_coop.json's longest_trail cases, which the test hands over as a text file (argv[2]): one case
//     per line, "expected n_edges  h b t  h b t ..."
//   * saturation: a mutual pair held state after state under N = 16 (fields never pass 15, REACHED in the eighth state) and N = 2;
//     fixed cases with fields of 8 .. 15: the boundary between N = 15 and N = 16, the clamp of a trail of 16 in the first and the last field
//   * the budget: a complete digraph on 6 agents with L = 0 and N = 16, and one on 4 agents (12 arcs, no trail of 16), either answer
//     what the brute force gives or report dense -- never a wrong answer; a state of at most 6 arcs is never dense
//   * the table code of search_logic.hpp with the trail word in the identity, the way tr_insert and tr_commit use it: candidates that
//     differ ONLY in the trail word are both stored, candidates equal in it exactly once; a candidate's trail word is never kept during
//     the insert: the comparing side works it out again from its own arcs and the other parent's pool record (sl::occupant_is over tl::TrailKind)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../lle_amd/trails/trails_logic.hpp"

namespace sl = lle_search_logic;
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
static void extend(const std::vector<Edge>& edges, int at, int time, uint64_t used, int len, int* best, long& steps) {
    for (size_t k = 0; k < edges.size(); k++) {
        const Edge& e = edges[k];
        if (e.h != at || e.t < time || ((used >> k) & 1u)) continue;
        steps++;
        if (len + 1 > best[e.b]) best[e.b] = len + 1;
        extend(edges, e.b, e.t, used | (uint64_t)1 << k, len + 1, best, steps);
    }
}
static long brute(const std::vector<Edge>& edges, int A, int* best) {
    long steps = 0;
    for (int a = 0; a < 8; a++) best[a] = 0;
    for (int a = 0; a < A; a++) extend(edges, a, -1, 0, 0, best, steps);
    return steps;
}
static uint64_t arcs_of(const std::vector<Edge>& edges, int t) {
    uint64_t arcs = 0;
    for (const Edge& e : edges)
        if (e.t == t) arcs |= (uint64_t)1 << (8 * e.h + e.b);
    return arcs;
}
// L over the states 0 .. T of `edges` by layer_update; returns the first t at which REACHED came back (T + 1: never)
static int run_layers(const std::vector<Edge>& edges, int A, int T, int N, uint32_t* L_out, bool* dense) {
    uint32_t L = 0u;
    *dense = false;
    for (int t = 0; t <= T; t++) {
        int budget = tl::WALK_BUDGET;
        const uint32_t next = tl::layer_update(L, arcs_of(edges, t), N, A, budget);
        if (budget < 0) {
            *dense = true;
            return t;
        }
        CHECK(tl::violates_sequence(next, N, A) == ((next & tl::REACHED) != 0u));  // fields below N unless REACHED says so
        if (next & tl::REACHED) {
            *L_out = next;
            return t;
        }
        L = next;
    }
    *L_out = L;
    return T + 1;
}

struct FakeBatch {  // a batch of n environments in exactly sized vectors (pitches as include/lle_hip.h allows them)
    std::vector<uint8_t> pos, avail, actions, err;
    std::vector<uint64_t> bits;
    std::vector<uint32_t> gems, beams;
    sl::BatchView v{};
    FakeBatch(int n, int A) : pos((size_t)n * 2 * A), avail((size_t)n * A), actions((size_t)n * A), err((size_t)n), bits((size_t)n), gems((size_t)n), beams((size_t)n) {
        v.pos = pos.data();
        v.bits = bits.data();
        v.gems = gems.data();
        v.beams = beams.data();
        v.avail = avail.data();
        v.actions = actions.data();
        v.err = err.data();
        v.pos_stride = 2 * A;
        v.pos_agent_stride = 2;
        v.beam_stride = 1;
        v.avail_stride = v.act_stride = A;
    }
};

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937 rng(seed);
    long graphs = 0, fields = 0, reached = 0, same_time_cycles = 0, kat = 0, dense = 0, answered = 0, dense_graphs = 0;
    int best[8];

    // ---- layer_update against the brute force
    for (int round = 0; round < 6000; round++) {
        const int A = 2 + (int)(rng() % 5u), T = (int)(rng() % 5u), n_edges = 1 + (int)(rng() % 10u);
        std::vector<Edge> edges;
        for (int k = 0; k < n_edges; k++) {
            Edge e{(int)(rng() % (uint32_t)A), (int)(rng() % (uint32_t)A), (int)(rng() % (uint32_t)(T + 1))};
            if (round % 4 == 0) e.t = 0;  // everything in one state: cycles inside a layer
            if (e.h == e.b) continue;
            bool dup = false;
            for (const Edge& o : edges) dup = dup || (o.h == e.h && o.b == e.b && o.t == e.t);
            if (!dup) edges.push_back(e);
        }
        for (const Edge& e : edges)
            for (const Edge& o : edges) same_time_cycles += (e.t == o.t && e.h == o.b && e.b == o.h && e.h < e.b);
        brute(edges, A, best);
        const int longest = *std::max_element(best, best + A);
        uint32_t L = 0u;
        bool was_dense = false;
        // unrestricted: at most 10 edges, so N = 16 rejects nothing and every field is exact
        const int at = run_layers(edges, A, T, 16, &L, &was_dense);
        if (was_dense) {  // honest only when the arcs of that one state allow more extensions than the budget
            std::vector<Edge> layer;
            for (const Edge& e : edges)
                if (e.t == at) layer.push_back(e);
            int b2[8];
            CHECK(brute(layer, A, b2) > tl::WALK_BUDGET);
            dense_graphs++;
            continue;
        }
        CHECK(at == T + 1);
        for (int a = 0; a < A; a++, fields++) CHECK((int)tl::field(L, a) == best[a]);
        CHECK((int)tl::longest(L, A) == longest && (L >> (4 * A)) == 0u);
        // every N: REACHED at the first state whose prefix holds a trail of N edges, exact fields otherwise
        for (int N = 2; N <= longest + 1 && N <= 16; N++) {
            int first = T + 1;
            for (int t = 0; t <= T && first > T; t++) {
                std::vector<Edge> prefix;
                for (const Edge& e : edges)
                    if (e.t <= t) prefix.push_back(e);
                int b2[8];
                brute(prefix, A, b2);
                if (*std::max_element(b2, b2 + A) >= N) first = t;
            }
            CHECK(run_layers(edges, A, T, N, &L, &was_dense) == first && !was_dense);
            CHECK(((L & tl::REACHED) != 0u) == (first <= T) && tl::violates_sequence(L, N, A) == (first <= T));
            reached += first <= T;
            if (first > T)
                for (int a = 0; a < A; a++) CHECK((int)tl::field(L, a) == best[a]);
        }
        graphs++;
    }

    // ---- the known answers
    if (argc > 2) {
        std::FILE* f = std::fopen(argv[2], "r");
        CHECK(f != nullptr);
        int expected = 0, n = 0;
        while (f && std::fscanf(f, "%d %d", &expected, &n) == 2) {
            std::vector<Edge> edges((size_t)n);
            int T = 0;
            for (Edge& e : edges) {
                CHECK(std::fscanf(f, "%d %d %d", &e.h, &e.b, &e.t) == 3 && e.h >= 0 && e.h < 6 && e.b >= 0 && e.b < 6 && e.t >= 0);
                T = std::max(T, e.t);
            }
            edges.erase(std::remove_if(edges.begin(), edges.end(), [](const Edge& e) { return e.h == e.b; }), edges.end());  // self-loops are ignored
            uint32_t L = 0u;
            bool was_dense = false;
            CHECK(run_layers(edges, 6, T, 16, &L, &was_dense) == T + 1 && !was_dense);
            CHECK((int)tl::longest(L, 6) == expected);
            brute(edges, 6, best);
            CHECK(*std::max_element(best, best + 6) == expected);
            kat++;
        }
        if (f) std::fclose(f);
    }

    // ---- saturation
    {
        const uint64_t pair = (uint64_t)1 << (8 * 0 + 1) | (uint64_t)1 << (8 * 1 + 0);
        uint32_t L = 0u;
        for (int state = 1; state <= 8; state++) {  // a mutual pair adds two edges to both trails per state
            int budget = tl::WALK_BUDGET;
            L = tl::layer_update(L, pair, 16, 2, budget);
            CHECK(budget >= 0 && tl::field(L, 0) <= 15u && tl::field(L, 1) <= 15u && (L & 0x7FFFFF00u) == 0u);
            if (state < 8) CHECK(L == (uint32_t)(2 * state) * 0x11u && !tl::violates_sequence(L, 16, 2));
            else CHECK((L & tl::REACHED) != 0u && tl::violates_sequence(L, 16, 2));
            // the eighth state: 0 -> 1 makes 15, 1 -> 0 would make 16 -- agent 0's field holds 15, not 16 & 15 = 0 with a carry into agent 1's
            if (state == 8) CHECK(L == (0xFFu | tl::REACHED));
        }
        {  // fixed cases: fields of 8 .. 15, the boundary between N = 15 and N = 16 (what long-trails stores on the device)
            int b15 = tl::WALK_BUDGET, b16 = tl::WALK_BUDGET;
            CHECK(tl::layer_update(0xDDu, pair, 16, 2, b16) == 0xFFu && !tl::violates_sequence(0xFFu, 16, 2));  // (13, 13): two more each, stored under N = 16
            CHECK((tl::layer_update(0xDDu, pair, 15, 2, b15) & tl::REACHED) != 0u && tl::violates_sequence(0xFFu, 15, 2));  // ... and a sequence of 15
            CHECK(b16 == tl::WALK_BUDGET - 4 && b15 == tl::WALK_BUDGET - 2);  // N = 15 stops at its second extension, 1 -> 0 at length 15
            for (int N = 9; N <= 16; N++) {  // one arc from a trail of N - 2: N - 1 is stored, whatever the field; one more arc is a sequence
                int budget = tl::WALK_BUDGET;
                const uint32_t before = (uint32_t)(N - 2) << 12;
                const uint32_t after = tl::layer_update(before, (uint64_t)1 << (8 * 3 + 5), N, 6, budget);
                CHECK(after == (before | (uint32_t)(N - 1) << 20) && !tl::violates_sequence(after, N, 6) && tl::violates_sequence(after, N - 1, 6));
                const uint32_t over = tl::layer_update(after, (uint64_t)1 << (8 * 5 + 4), N, 6, budget);
                CHECK((over & tl::REACHED) != 0u && tl::field(over, 4) == (uint32_t)(N < 15 ? N : 15) && (over & 0x7F000000u) == 0u);
            }
            // a trail of 16 into agent 5's field, bits 20-23: clamped to 15, nothing carried into bit 24
            int budget = tl::WALK_BUDGET;
            CHECK(tl::layer_update(0xFu << 12, (uint64_t)1 << (8 * 3 + 5), 16, 6, budget) == (0xFu << 12 | 0xFu << 20 | tl::REACHED));
        }
        int budget = tl::WALK_BUDGET;
        L = tl::layer_update(0u, (uint64_t)1 << (8 * 3 + 5), 2, 6, budget);  // one edge: length 1, in agent 5's field
        CHECK(L == 1u << 20 && !tl::violates_sequence(L, 2, 6) && budget == tl::WALK_BUDGET - 1);
        L = tl::layer_update(L, (uint64_t)1 << (8 * 5 + 2), 2, 6, budget);   // 3 -> 5, then 5 -> 2: a sequence
        CHECK((L & tl::REACHED) != 0u && tl::violates_sequence(L, 2, 6));
        L = tl::layer_update(1u << 20, (uint64_t)1 << (8 * 2 + 5), 2, 6, budget);  // 3 -> 5, then 2 -> 5: no chain
        CHECK(L == 1u << 20);
        budget = 7;
        CHECK(tl::layer_update(0x00123456u, 0ull, 7, 6, budget) == 0x00123456u && budget == 7);  // no arcs: L as it is, no walk
        CHECK(tl::violates_sequence(0x00600000u, 6, 6) && !tl::violates_sequence(0x00600000u, 7, 6) && tl::longest(0x00600000u, 5) == 0u);
    }

    // ---- the budget
    for (int A : {6, 5, 4, 3}) {
        std::vector<Edge> edges;
        for (int h = 0; h < A; h++)
            for (int b = 0; b < A; b++)
                if (h != b) edges.push_back(Edge{h, b, 0});
        for (int N : {16, 13, 12, 7}) {
            int budget = tl::WALK_BUDGET;
            const uint32_t L = tl::layer_update(0u, arcs_of(edges, 0), N, A, budget);
            const int eulerian = A * (A - 1);  // a complete digraph has a closed trail over all its arcs
            if (budget < 0) {
                dense++;
                continue;
            }
            answered++;
            CHECK(((L & tl::REACHED) != 0u) == (eulerian >= N));
            if (!(L & tl::REACHED))
                for (int a = 0; a < A; a++) CHECK((int)tl::field(L, a) == eulerian);  // closed at every agent
        }
    }
    for (int round = 0; round < 300; round++) {  // at most 6 arcs: never dense, whatever N
        const int A = 2 + (int)(rng() % 5u);
        std::vector<Edge> edges;
        while ((int)edges.size() < 6) {
            Edge e{(int)(rng() % (uint32_t)A), (int)(rng() % (uint32_t)A), 0};
            bool dup = e.h == e.b;
            for (const Edge& o : edges) dup = dup || (o.h == e.h && o.b == e.b);
            if (!dup) edges.push_back(e);
            if (A == 2 && edges.size() == 2) break;
        }
        int budget = tl::WALK_BUDGET;
        const uint32_t L = tl::layer_update(0u, arcs_of(edges, 0), 16, A, budget);
        const long steps = brute(edges, A, best);
        CHECK(budget >= 0 && tl::WALK_BUDGET - budget == steps && steps <= 1956);  // one unit per arc extension, as the brute force counts them
        for (int a = 0; a < A; a++) CHECK((int)tl::field(L, a) == best[a]);
    }

    // ---- the table with the trail word in the identity: three equal states under parents whose L differs, in ONE piece (tag against
    // tag), then again (tag against pool)
    long stored = 0, duplicates = 0;
    for (int variant = 0; variant < 2; variant++) {
        const int A = 2;
        const sl::RecordLayout r = sl::make_layout(A, 1, false);
        const uint32_t cap = 16, slots = (uint32_t)sl::table_slots(cap, 8), n_joint = 1;  // (n_joint = 1: candidate k expands parent k)
        std::vector<uint32_t> table(slots, sl::SLOT_EMPTY), pool((size_t)(r.n_words + 1) * cap, 0u);
        const uint64_t edges = variant == 0 ? 0ull : (uint64_t)1 << (8 * 0 + 1);  // no arcs: L as the parent's; 0 -> 1: L[1] = max(L[1], L[0] + 1)
        tl::store_pool_trail(pool.data(), cap, r, 0, 0x01u);  // parent 0: a trail of 1 ends at agent 0
        tl::store_pool_trail(pool.data(), cap, r, 1, 0x10u);  // parent 1: ... at agent 1
        tl::store_pool_trail(pool.data(), cap, r, 2, variant == 0 ? 0x01u : 0x21u);  // parent 2: as parent 0 / another L that the arc makes equal: (1, 2)
        uint32_t n_states = 3;
        auto load = [](uint32_t* slot) { return *slot; };
        auto cas = [](uint32_t* slot, uint32_t expected, uint32_t desired) {
            const uint32_t v = *slot;
            if (v == expected) *slot = desired;
            return v;
        };
        for (int piece = 0; piece < 2; piece++) {
            FakeBatch fb(3, A);  // three equal states
            for (int k = 0; k < 3; k++) fb.bits[(size_t)k] = 3u | (uint64_t)3u << 32;
            const sl::Piece who{fb.v, 0, 3u, pool.data(), cap, cap, 0, 0, 3, n_joint};
            const tl::TrailKind kind{{}, 5};  // (the arcs are given: no edge rule is read)
            int64_t win[3];
            uint32_t trail[3];
            for (int k = 0; k < 3; k++) {
                const sl::EnvRecord rec{fb.v, r, k};
                CHECK(kind.successor(pool.data(), cap, r, (uint64_t)k, edges, &trail[k]));
                const auto me = tl::key_with_trail(rec, r.n_key, trail[k]);
                auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, kind, edges, occupant, me); };
                win[k] = sl::table_insert(table.data(), slots - 1, 5u /* one hash for all: they meet */, sl::TAG_BIT | (uint32_t)k, load, cas, same_as);
                stored += win[k] >= 0;
                duplicates += win[k] == sl::INSERT_DUPLICATE;
            }
            CHECK(trail[0] == (variant == 0 ? 0x01u : 0x21u) && trail[1] == 0x10u && trail[2] == trail[0]);
            // piece 0: candidates 0 and 1 differ only in the trail word (both stored), candidate 2 equals candidate 0 (a tag); piece 1: all known (pool)
            CHECK(piece == 0 ? (win[0] >= 0 && win[1] >= 0 && win[2] == sl::INSERT_DUPLICATE) : (win[0] < 0 && win[1] < 0 && win[2] < 0));
            for (int k = 0; k < 3; k++)
                if (win[k] >= 0) {
                    const uint32_t idx = n_states++;
                    sl::copy_record(fb.v, r, k, pool.data(), cap, idx);
                    tl::store_pool_trail(pool.data(), cap, r, idx, trail[k]);
                    CHECK(tl::pool_trail(pool.data(), cap, r, idx) == trail[k]);
                    table[(size_t)win[k]] = idx;
                }
        }
        CHECK(n_states == 5);
    }
    if (failures) return 1;
    std::printf("OK graphs=%ld fields=%ld reached=%ld same_time_cycles=%ld kat=%ld dense=%ld answered=%ld dense_graphs=%ld stored=%ld duplicates=%ld\n", graphs, fields,
                reached, same_time_cycles, kat, dense, answered, dense_graphs, stored, duplicates);
    return 0;
}
