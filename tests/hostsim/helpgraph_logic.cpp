// helpgraph_logic.cpp -- the host-and-device logic of the help-graph search (lle_amd/helpgraph/helpgraph_logic.hpp) on the host, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_helpgraph_cpu.py and checked against naive loops.
//
//   * violates / accepts against loops over an edge MATRIX, for every matrix without self-loops of A = 2, 3, 4 agents (4, 64, 4 096) and
//     10 000 seeded random ones of A = 5, 6, every mode, every parameter 2 .. A + 1
//   * state_edges against a loop over sources on seeded random cell tables, colours, flags, positions and occupant bits
//   * the table code of search_logic.hpp with help words in the identity, the way hg_insert and hg_commit use it: candidates that differ
//     ONLY in a help word -- tag against tag inside a piece, and tag against pool across pieces -- must both be stored; candidates that
//     are equal, help words included, must be stored exactly once.  A candidate's help words are never kept during the insert: the
//     comparing side works them out again from its own edges (equal key words, equal edges) and the candidate's parent's pool record (sl::occupant_is over hl::HelpKind).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../lle_amd/helpgraph/helpgraph_logic.hpp"

namespace sl = lle_search_logic;
namespace hl = lle_helpgraph_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

// ---- the modes, naively: e[h][b] = h has helped b
struct Matrix {
    bool e[6][6];
};
static Matrix matrix_of(uint64_t help, int A) {
    Matrix m{};
    for (int h = 0; h < A; h++)
        for (int b = 0; b < A; b++) m.e[h][b] = (help >> (8 * h + b)) & 1u;
    return m;
}
static bool naive_violates(const Matrix& m, int mode, int param, int A) {
    if (mode == hl::NO_CONVERGENCE) {
        for (int b = 0; b < A; b++) {
            int n = 0;
            for (int h = 0; h < A; h++) n += m.e[h][b];
            if (n >= param) return true;
        }
    } else if (mode == hl::NO_DIVERGENCE) {
        for (int h = 0; h < A; h++) {
            int n = 0;
            for (int b = 0; b < A; b++) n += m.e[h][b];
            if (n >= param) return true;
        }
    } else if (mode == hl::NO_MUTUAL) {
        for (int a = 0; a < A; a++)
            for (int b = 0; b < A; b++)
                if (a != b && m.e[a][b] && m.e[b][a]) return true;
    } else if (mode == hl::NO_FULLY_COUPLED) {
        int n = 0;
        for (int a = 0; a < A; a++)
            for (int b = 0; b < A; b++) n += (a != b && m.e[a][b]);
        return A >= 2 && n == A * (A - 1);
    }
    return false;
}
static bool naive_accepts(const Matrix& m, int mode, int A) {
    if (mode != hl::NO_ASYMMETRIC) return true;
    for (int h = 0; h < A; h++)
        for (int b = 0; b < A; b++) {
            if (!m.e[h][b]) continue;
            bool helped = false;  // is h anybody's beneficiary?
            for (int g = 0; g < A; g++) helped = helped || m.e[g][h];
            if (!helped) return false;
        }
    return true;
}
static long check_modes(uint64_t help, int A) {
    const Matrix m = matrix_of(help, A);
    long n = 0;
    for (int mode = 0; mode < hl::N_MODES; mode++) {
        CHECK(hl::accepts(help, mode, A) == naive_accepts(m, mode, A));
        for (int param = 2; param <= A + 1; param++, n++) CHECK(hl::violates(help, mode, param, A) == naive_violates(m, mode, param, A));
    }
    return n;
}
// matrix number `code` of A agents: one bit per ordered pair h != b
static uint64_t help_of_code(uint32_t code, int A) {
    uint64_t help = 0;
    int bit = 0;
    for (int h = 0; h < A; h++)
        for (int b = 0; b < A; b++)
            if (h != b && ((code >> bit++) & 1u)) help |= (uint64_t)1 << (8 * h + b);
    return help;
}

// ---- the edge rule, naively: per enabled source, its colour among the occupants of its tiles
static uint64_t naive_edges(int A, int H, int W, const std::vector<uint32_t>& cells, const std::vector<int>& colour, uint32_t enabled, const int (*pos)[2],
                            uint32_t occupant) {
    uint64_t help = 0;
    for (int l = 0; l < (int)colour.size(); l++) {
        if (!((enabled >> l) & 1u)) continue;
        uint32_t on_beam = 0;  // the agents that occupy a tile of source l
        for (int a = 0; a < A; a++)
            if (((occupant >> a) & 1u) && pos[a][0] < H && pos[a][1] < W && ((cells[(size_t)pos[a][0] * W + pos[a][1]] >> l) & 1u)) on_beam |= 1u << a;
        const int c = colour[(size_t)l];
        if (c < 0 || c >= A || !((on_beam >> c) & 1u)) continue;
        for (int b = 0; b < A; b++)
            if (b != c && ((on_beam >> b) & 1u)) help |= (uint64_t)1 << (8 * c + b);
    }
    return help;
}

// ---- a fake batch of n environments in exactly sized vectors (pitches as include/lle_hip.h allows them)
struct FakeBatch {
    std::vector<uint8_t> pos, avail, actions, err;
    std::vector<uint64_t> bits;
    std::vector<uint32_t> gems, beams;
    sl::BatchView v{};
    FakeBatch(int n, int A, int Lw) : pos((size_t)n * 2 * A), avail((size_t)n * A), actions((size_t)n * A), err((size_t)n), bits((size_t)n), gems((size_t)n), beams((size_t)n * (Lw ? Lw : 1)) {
        v.pos = pos.data();
        v.bits = bits.data();
        v.gems = gems.data();
        v.beams = beams.data();
        v.avail = avail.data();
        v.actions = actions.data();
        v.err = err.data();
        v.pos_stride = 2 * A;
        v.pos_agent_stride = 2;
        v.beam_stride = Lw ? Lw : 1;
        v.avail_stride = v.act_stride = A;
    }
};

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937 rng(seed);
    long matrices = 0, mode_checks = 0, states = 0, edges_seen = 0, stored = 0, duplicates = 0;

    // ---- violates / accepts
    for (int A = 2; A <= 4; A++)
        for (uint32_t code = 0; code < (1u << (A * (A - 1))); code++, matrices++) mode_checks += check_modes(help_of_code(code, A), A);
    for (int A = 5; A <= 6; A++)
        for (int n = 0; n < 10000; n++, matrices++) {
            uint32_t code = rng();
            if (n % 3 == 1) code &= rng();        // sparse
            if (n % 3 == 2) code |= rng() | rng();  // dense
            if (n == 0) code = 0xFFFFFFFFu;
            mode_checks += check_modes(help_of_code(code, A), A);
        }
    CHECK(hl::violates(0, hl::NO_FULLY_COUPLED, 2, 1) == false && hl::accepts(0, hl::NO_ASYMMETRIC, 6));
    CHECK(hl::help_of(hl::help_lo(0x0000A1B2C3D4E5F6ull), hl::help_hi(0x0000A1B2C3D4E5F6ull)) == 0x0000A1B2C3D4E5F6ull);

    // ---- state_edges
    for (int round = 0; round < 4000; round++) {
        const int A = 1 + (int)(rng() % 6u), H = 1 + (int)(rng() % 7u), W = 1 + (int)(rng() % 7u), L = (int)(rng() % 33u);
        const sl::RecordLayout r = sl::make_layout(A, L, false);
        std::vector<uint32_t> cells((size_t)H * W, 0u);
        for (auto& c : cells)
            for (int l = 0; l < L; l++)
                if (rng() % 3u == 0) c |= 1u << l;
        std::vector<int> colour((size_t)L);
        hl::EdgeRule rule{};
        rule.A = A;
        rule.H = H;
        rule.W = W;
        for (int l = 0; l < L; l++) {
            colour[(size_t)l] = (int)(rng() % 8u);  // colours 6 and 7 are nobody's
            if (colour[(size_t)l] < sl::MAX_AGENTS) rule.mine[colour[(size_t)l]] |= 1u << l;
            if (rng() % 4u) rule.enabled |= 1u << l;
        }
        int pos[6][2];
        std::vector<uint32_t> rec((size_t)r.n_words, 0u);
        const uint32_t occupant = rng() % 4u ? sl::agents_mask(A) : rng() & sl::agents_mask(A);
        for (int a = 0; a < A; a++) {
            pos[a][0] = (int)(rng() % (uint32_t)(H + (round % 50 == 0)));  // now and then a row outside the map: no cell, no edge
            pos[a][1] = (int)(rng() % (uint32_t)W);
            if (round % 3 == 0 && a > 0 && rng() % 2u) pos[a][0] = pos[0][0];  // crowd a row: beams run along rows and columns
            rec[(size_t)(a >> 1)] |= ((uint32_t)pos[a][0] | (uint32_t)pos[a][1] << 8) << (16 * (a & 1));
        }
        rec[(size_t)r.w_bits] = sl::agents_mask(A);
        rec[(size_t)r.w_bits + 1] = occupant | 0xFFFF0000u;  // (the bits above the occupants are somebody else's)
        const uint64_t got = hl::state_edges([&](int w) { return rec[(size_t)w]; }, r, rule, [&](int c) { return cells[(size_t)c]; });
        const uint64_t want = naive_edges(A, H, W, cells, colour, rule.enabled, pos, occupant);
        CHECK(got == want);
        states++;
        edges_seen += got != 0;
    }

    // ---- the table with help words in the identity
    for (int round = 0; round < 60; round++) {
        const int A = 1 + (int)(rng() % 6u), Lw = (int)(rng() % 3u);
        const bool collect = rng() % 2u;
        const sl::RecordLayout r = sl::make_layout(A, Lw, collect);
        const uint32_t n_joint = sl::pow5(A), cap = 512, slots = (uint32_t)sl::table_slots(cap, 64);
        // a map of one row and two sources of colour 0 and 1 over its cells, so that positions decide the edges
        const int W = 8;
        std::vector<uint32_t> cells((size_t)W);
        for (auto& c : cells) c = rng() % 4u;
        hl::EdgeRule rule{};
        rule.A = A;
        rule.H = 1;
        rule.W = W;
        rule.enabled = 3u;
        rule.mine[0] = 1u;
        if (A > 1) rule.mine[1] = 2u;
        auto cell = [&](int c) { return cells[(size_t)c]; };
        std::vector<uint32_t> table(slots, sl::SLOT_EMPTY), pool((size_t)(r.n_words + 2) * cap, 0u);
        std::set<std::vector<uint32_t>> seen;  // identities: key words, then help words
        uint32_t n_states = 0;
        // the pool starts with a few parents that are equal but for their help words
        const int n_parents = 2 + (int)(rng() % 3u);
        for (int s = 0; s < n_parents; s++) hl::store_pool_help(pool.data(), cap, r, (uint64_t)s, (uint64_t)(rng() % 4u) << (8 * (A - 1)) | (rng() % 2u ? 2u : 0u));
        n_states = (uint32_t)n_parents;
        auto load = [](uint32_t* slot) { return *slot; };
        auto cas = [](uint32_t* slot, uint32_t expected, uint32_t desired) {
            const uint32_t v = *slot;
            if (v == expected) *slot = desired;
            return v;
        };
        for (int piece = 0; piece < 4 && n_states + 64 <= cap; piece++) {
            const int n = 2 + (int)(rng() % 62u);
            FakeBatch fb(n, A, Lw);
            // candidate k expands parent first_state + (item0 + k) / n_joint: spread the candidates over the parents
            const uint64_t first_state = 0, item0 = rng() % n_joint;
            const uint64_t last_parent = first_state + (item0 + (uint64_t)n - 1) / n_joint;
            if (last_parent >= (uint64_t)n_parents) continue;
            const int variants = 1 + (int)(rng() % 3u);
            for (int k = 0; k < n; k++) {  // few distinct states, so that equal ones meet; the same state under parents of different help
                const uint32_t v = rng() % (uint32_t)variants;
                for (int a = 0; a < A; a++) {
                    fb.pos[(size_t)k * 2 * A + 2 * a] = 0;
                    fb.pos[(size_t)k * 2 * A + 2 * a + 1] = (uint8_t)((v + (uint32_t)a) % (uint32_t)W);
                }
                fb.bits[(size_t)k] = (uint64_t)sl::agents_mask(A) | (uint64_t)sl::agents_mask(A) << 32;
                fb.gems[(size_t)k] = v & 1u;
                for (int w = 0; w < Lw; w++) fb.beams[(size_t)k * Lw + w] = 7u;
            }
            const sl::Piece who{fb.v, 0, (uint32_t)n, pool.data(), cap, cap, first_state, item0, item0 + (uint64_t)n, n_joint};
            const hl::HelpKind kind{rule, hl::STANDARD, 0};
            std::vector<int64_t> win((size_t)n, -1);
            std::vector<uint64_t> help((size_t)n, 0);
            for (int k = 0; k < n; k++) {
                const sl::EnvRecord rec{fb.v, r, k};
                const uint64_t parent = first_state + (item0 + (uint64_t)k) / n_joint;
                const uint64_t edges = kind.state(rec, r, cell);
                CHECK(kind.successor(pool.data(), cap, r, parent, edges, &help[(size_t)k]));
                const auto me = hl::key_with_help(rec, r.n_key, help[(size_t)k]);
                auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, kind, edges, occupant, me); };
                const int64_t slot = sl::table_insert(table.data(), slots - 1, sl::hash_record(me, r.n_key + 2), sl::TAG_BIT | (uint32_t)k, load, cas, same_as);
                std::vector<uint32_t> id;
                for (int w = 0; w < r.n_key + 2; w++) id.push_back(me(w));
                const bool fresh = seen.insert(id).second;
                CHECK(slot != sl::INSERT_FULL && (slot >= 0) == fresh);  // differ only in a help word: both stored; equal: exactly one
                win[(size_t)k] = slot;
                stored += fresh;
                duplicates += !fresh;
            }
            for (int k = 0; k < n; k++) {  // commit
                if (win[(size_t)k] < 0) continue;
                const uint32_t idx = n_states++;
                sl::copy_record(fb.v, r, k, pool.data(), cap, idx);
                hl::store_pool_help(pool.data(), cap, r, idx, help[(size_t)k]);
                CHECK(hl::pool_help(pool.data(), cap, r, idx) == help[(size_t)k]);
                table[(size_t)win[(size_t)k]] = idx;
            }
            uint32_t occupied = 0;
            for (uint32_t v : table) {
                CHECK(v == sl::SLOT_EMPTY || v < n_states);
                occupied += v != sl::SLOT_EMPTY;
            }
            CHECK(occupied == seen.size() && n_states == (uint32_t)n_parents + seen.size());
        }
    }
    // two candidates with equal key words under parents whose help differs, in ONE piece (tag against tag), then again (tag against pool)
    {
        const int A = 2;
        const sl::RecordLayout r = sl::make_layout(A, 1, false);
        const uint32_t cap = 16, slots = (uint32_t)sl::table_slots(cap, 8), n_joint = 1;  // (n_joint = 1: candidate k expands parent k)
        std::vector<uint32_t> table(slots, sl::SLOT_EMPTY), pool((size_t)(r.n_words + 2) * cap, 0u), cells(4, 0u);
        hl::EdgeRule rule{};
        rule.A = A;
        rule.H = 1;
        rule.W = 4;
        auto cell = [&](int c) { return cells[(size_t)c]; };
        hl::store_pool_help(pool.data(), cap, r, 0, 0x0002u);  // parent 0: 0 has helped 1
        hl::store_pool_help(pool.data(), cap, r, 1, 0x0100u);  // parent 1: 1 has helped 0
        hl::store_pool_help(pool.data(), cap, r, 2, 0x0002u);  // parent 2: as parent 0
        uint32_t n_states = 3;
        auto load = [](uint32_t* slot) { return *slot; };
        auto cas = [](uint32_t* slot, uint32_t expected, uint32_t desired) {
            const uint32_t v = *slot;
            if (v == expected) *slot = desired;
            return v;
        };
        for (int piece = 0; piece < 2; piece++) {
            FakeBatch fb(3, A, 1);  // three equal states
            for (int k = 0; k < 3; k++) fb.bits[(size_t)k] = 3u | (uint64_t)3u << 32;
            const sl::Piece who{fb.v, 0, 3u, pool.data(), cap, cap, 0, 0, sl::ALL_ITEMS, n_joint};
            const hl::HelpKind kind{rule, hl::STANDARD, 0};
            int winners = 0;
            int64_t win[3];
            for (int k = 0; k < 3; k++) {
                const sl::EnvRecord rec{fb.v, r, k};
                const uint64_t edges = kind.state(rec, r, cell);
                uint64_t help = 0;
                CHECK(kind.successor(pool.data(), cap, r, (uint64_t)k, edges, &help));
                const auto me = hl::key_with_help(rec, r.n_key, help);
                auto same_as = [&](uint32_t occupant) { return sl::occupant_is(who, r, kind, edges, occupant, me); };
                win[k] = sl::table_insert(table.data(), slots - 1, 5u /* one hash for all: they meet */, sl::TAG_BIT | (uint32_t)k, load, cas, same_as);
                winners += win[k] >= 0;
            }
            // piece 0: candidates 0 and 1 differ only in a help word (both stored), candidate 2 equals candidate 0 (a tag); piece 1: all known (pool)
            CHECK(piece == 0 ? (win[0] >= 0 && win[1] >= 0 && win[2] == sl::INSERT_DUPLICATE) : winners == 0);
            for (int k = 0; k < 3; k++)
                if (win[k] >= 0) {
                    const uint32_t idx = n_states++;
                    sl::copy_record(fb.v, r, k, pool.data(), cap, idx);
                    hl::store_pool_help(pool.data(), cap, r, idx, hl::pool_help(pool.data(), cap, r, (uint64_t)k));
                    table[(size_t)win[k]] = idx;
                }
        }
        CHECK(n_states == 5);
    }
    if (failures) return 1;
    std::printf("OK matrices=%ld mode_checks=%ld states=%ld with_edges=%ld stored=%ld duplicates=%ld\n", matrices, mode_checks, states, edges_seen, stored, duplicates);
    return 0;
}
