// record_io.cpp -- the record I/O of the shortest-plan search (lle_amd/search/search_logic.hpp: BatchView, env_word, PoolRecord,
// scatter_item, same_record, occupant_is, copy_record, is_goal, root_on_foreign_beam, table_slots) on the host, built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_search_cpu.py and run as a child process.
//
// A fake batch of a few environments lies in std::vectors that end with the last byte the layout uses, filled with a sentinel, so
// the address sanitizer sees a write or read one past it and a comparison of the whole buffers sees a write into the padding between
// agents and rows.  For every A in 1..6, Lw in {0, 1, 2, 32}, agent pitch 2 and 4 and both key widths: a pool record scattered into an
// environment reads back word for word and changes nothing else; every joint action code (a fixed sample above three agents) is
// taken exactly when joint_available says so and leaves its base-5 digits; the occupant comparer takes an equal record by tag and by
// pool index, refuses one that differs in a single key word, looks at the gem word exactly when gems are collected, and refuses tags
// and pool indices out of range; PoolRecord on a base moved to a map's segment reads what forest_logic.hpp's pool_index names.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../lle_amd/forest/forest_logic.hpp"
#include "../../lle_amd/search/search_logic.hpp"

namespace sl = lle_search_logic;
namespace fl = lle_forest_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static long cases = 0, codes_tried = 0, codes_valid = 0, compared = 0;

constexpr int E = 5;        // environments of the fake batch
constexpr int MAPS = 3;     // segments of the pool, as the forest lays them out
constexpr uint64_t CAP = 7; // states per segment
constexpr uint8_t SENTINEL = 0xA5;

struct FakeBatch {
    int A, Lw;
    std::vector<uint8_t> pos, avail, actions, err;
    std::vector<uint64_t> bits;
    std::vector<uint32_t> gems, beams;
    sl::BatchView view{};

    FakeBatch(int A_, int Lw_, int64_t agent_pitch) : A(A_), Lw(Lw_) {
        view.pos_agent_stride = agent_pitch;
        view.pos_stride = A * agent_pitch + 3;  // > 2 A
        view.avail_stride = A + 2;
        view.act_stride = A + 1;
        view.beam_stride = Lw + 1;
        pos.assign((size_t)((E - 1) * view.pos_stride + (A - 1) * agent_pitch + 2), SENTINEL);
        avail.assign((size_t)((E - 1) * view.avail_stride + A), SENTINEL);
        actions.assign((size_t)((E - 1) * view.act_stride + A), SENTINEL);
        err.assign((size_t)E, 0);
        bits.assign((size_t)E, 0xA5A5A5A5A5A5A5A5ull);
        gems.assign((size_t)E, 0xA5A5A5A5u);
        beams.assign((size_t)((E - 1) * view.beam_stride + Lw), 0xA5A5A5A5u);
        view.pos = pos.data();
        view.bits = bits.data();
        view.gems = gems.data();
        view.beams = beams.data();
        view.avail = avail.data();
        view.actions = actions.data();
        view.err = err.data();
    }
    bool same_buffers(const FakeBatch& o) const {
        return pos == o.pos && avail == o.avail && actions == o.actions && bits == o.bits && gems == o.gems && beams == o.beams;
    }
};

// What scatter_item must leave in environment k, written agent by agent from the unpacked fields of a record.
struct Fields {
    std::vector<uint8_t> ij, avail;  // [2 A], [A]
    uint64_t bits;
    uint32_t gems;
    std::vector<uint32_t> beams;
};

static std::vector<uint32_t> pack(const Fields& f, const sl::RecordLayout& r) {
    std::vector<uint32_t> rec((size_t)r.n_words, 0u);
    for (int a = 0; a < r.A; a++) {
        rec[(size_t)(a / 2)] |= ((uint32_t)f.ij[(size_t)2 * a] | (uint32_t)f.ij[(size_t)2 * a + 1] << 8) << (16 * (a % 2));
        rec[(size_t)(r.w_avail + a / 4)] |= (uint32_t)f.avail[(size_t)a] << (8 * (a % 4));
    }
    rec[(size_t)r.w_bits] = (uint32_t)f.bits;
    rec[(size_t)r.w_bits + 1] = (uint32_t)(f.bits >> 32);
    for (int w = 0; w < r.Lw; w++) rec[(size_t)(r.w_beams + w)] = f.beams[(size_t)w];
    rec[(size_t)r.w_gems] = f.gems;
    return rec;
}

static void expect_scatter(FakeBatch& b, const Fields& f, int k, uint32_t code) {
    const sl::BatchView& v = b.view;
    for (int a = 0; a < b.A; a++) {
        b.pos[(size_t)(k * v.pos_stride + a * v.pos_agent_stride)] = f.ij[(size_t)2 * a];
        b.pos[(size_t)(k * v.pos_stride + a * v.pos_agent_stride + 1)] = f.ij[(size_t)2 * a + 1];
        b.avail[(size_t)(k * v.avail_stride + a)] = f.avail[(size_t)a];
        b.actions[(size_t)(k * v.act_stride + a)] = (uint8_t)(code % 5u);
        code /= 5u;
    }
    b.bits[(size_t)k] = f.bits;
    b.gems[(size_t)k] = f.gems;
    for (int w = 0; w < b.Lw; w++) b.beams[(size_t)(k * v.beam_stride + w)] = f.beams[(size_t)w];
}

static bool available(const Fields& f, int A, uint32_t code) {
    for (int a = 0; a < A; a++) {
        if (!((f.avail[(size_t)a] >> (code % 5u)) & 1u)) return false;
        code /= 5u;
    }
    return true;
}

static void one_shape(int A, int Lw, int64_t agent_pitch, bool collect, std::mt19937& rng) {
    const sl::RecordLayout r = sl::make_layout(A, Lw, collect);
    const uint32_t n_joint = sl::pow5(A);
    // ---- a pool of MAPS segments of CAP states; the records of segment `map`
    const int map = (int)(rng() % MAPS);
    std::vector<uint32_t> pool((size_t)MAPS * r.n_words * CAP, 0xDEADBEEFu);
    std::vector<Fields> fields((size_t)CAP);
    for (uint64_t s = 0; s < CAP; s++) {
        Fields& f = fields[(size_t)s];
        f.ij.resize((size_t)2 * A);
        f.avail.resize((size_t)A);
        f.beams.resize((size_t)Lw);
        for (auto& x : f.ij) x = (uint8_t)(rng() % 256u);
        for (auto& x : f.avail) x = (uint8_t)(1u + rng() % 31u);
        for (auto& x : f.beams) x = (uint32_t)rng();
        f.bits = (uint64_t)rng() << 32 | rng();
        f.gems = (uint32_t)rng();
        const std::vector<uint32_t> rec = pack(f, r);
        for (int w = 0; w < r.n_words; w++) pool[(size_t)fl::pool_index(map, r.n_words, w, CAP, s)] = rec[(size_t)w];
    }
    uint32_t* const segment = pool.data() + (size_t)map * r.n_words * CAP;
    for (int w = 0; w < r.n_words; w++)
        for (uint64_t s : {(uint64_t)0, CAP / 2, CAP - 1})
            CHECK((sl::PoolRecord{segment, CAP, s}(w)) == pool[(size_t)fl::pool_index(map, r.n_words, w, CAP, s)]);

    // ---- every code: taken exactly when available; a taken one reads back and touches nothing else
    FakeBatch got(A, Lw, agent_pitch), want(A, Lw, agent_pitch);
    std::vector<uint32_t> codes;
    if (A <= 3) {
        for (uint32_t c = 0; c < n_joint; c++) codes.push_back(c);
    } else {
        codes = {0u, n_joint - 1u, n_joint / 2u};
        for (uint32_t n = 1; n <= 200; n++) codes.push_back((uint32_t)((uint64_t)n * 2654435761u % n_joint));
    }
    for (size_t n = 0; n < codes.size(); n++) {
        const uint32_t code = codes[n];
        const uint64_t s = n % CAP;
        const int k = (int)(n % E);
        const sl::PoolRecord rec{segment, CAP, s};
        const bool valid = sl::scatter_item(got.view, r, rec, k, code);
        CHECK(valid == available(fields[(size_t)s], A, code));
        CHECK(valid == sl::joint_available(code, A, [&](int a) { return (uint32_t)fields[(size_t)s].avail[(size_t)a]; }));
        if (valid) {
            expect_scatter(want, fields[(size_t)s], k, code);
            for (int w = 0; w < r.n_words; w++) CHECK(sl::env_word(got.view, r, k, w) == rec(w));
            for (int w = 0; w <= r.w_gems; w++) CHECK(sl::env_word(got.view.key(), r, k, w) == rec(w));
        }
        CHECK(got.same_buffers(want));  // the padding keeps its sentinel; an unavailable code writes nothing
        codes_tried++;
        codes_valid += valid;
    }

    // ---- the occupant comparer: environments 0 and 1 hold state 2, environment 2 holds state 3
    auto put = [&](int k, uint64_t s) {
        const Fields& f = fields[(size_t)s];
        uint32_t code = 0;
        for (int a = A - 1; a >= 0; a--) {
            int digit = 0;
            while (!((f.avail[(size_t)a] >> digit) & 1u)) digit++;
            code = code * 5u + (uint32_t)digit;
        }
        CHECK(sl::scatter_item(got.view, r, sl::PoolRecord{segment, CAP, s}, k, code));
    };
    put(0, 2);
    put(1, 2);
    put(2, 3);
    const sl::EnvRecord me{got.view, r, 0};
    const sl::Occupants who{got.view.key(), 0, (uint32_t)E, segment, CAP, CAP};
    CHECK(sl::same_record(me, sl::PoolRecord{segment, CAP, 2}, r.n_words) && sl::same_record(me, sl::EnvRecord{got.view, r, 1}, r.n_words));
    CHECK(sl::occupant_is(who, r, sl::TAG_BIT | 1u, me) && sl::occupant_is(who, r, sl::TAG_BIT | 0u, me) && sl::occupant_is(who, r, 2u, me));
    CHECK(!sl::occupant_is(who, r, sl::TAG_BIT | 2u, me) && !sl::occupant_is(who, r, 3u, me));
    // a tag counts from env0: tag 0 of a block that begins at environment 1 is environment 1
    const sl::Occupants block{got.view.key(), 1, 2u, segment, CAP, CAP};
    CHECK(sl::occupant_is(block, r, sl::TAG_BIT | 0u, me) && !sl::occupant_is(block, r, sl::TAG_BIT | 1u, me));
    // out of range: a tag at or above the tag count, a pool index at or above the capacity (far ones would read outside the vectors)
    CHECK(!sl::occupant_is(block, r, sl::TAG_BIT | 2u, me) && !sl::occupant_is(who, r, sl::TAG_BIT | (uint32_t)E, me));
    CHECK(!sl::occupant_is(who, r, sl::TAG_BIT | 0x3FFFFFFFu, me) && !sl::occupant_is(who, r, (uint32_t)CAP, me) && !sl::occupant_is(who, r, 0x7FFFFFFFu, me));
    const sl::Occupants two_states{got.view.key(), 0, (uint32_t)E, segment, CAP, 2};
    CHECK(!sl::occupant_is(two_states, r, 2u, me));
    // one word off: state 4 and environment 3 become state 2 with a single word changed
    for (int w = 0; w < r.n_words; w++) {
        for (int x = 0; x < r.n_words; x++) segment[(size_t)x * CAP + 4] = segment[(size_t)x * CAP + 2];
        const uint32_t flip = w < r.n_pos ? 1u << (8 * (int)(rng() % (uint32_t)std::min(4, 2 * A - 4 * w)))  // (a byte that exists)
                              : w >= r.w_avail ? 0u : 1u << (rng() % 32u);
        segment[(size_t)w * CAP + 4] ^= flip;
        Fields f = fields[2];
        if (w < r.n_pos) f.ij[(size_t)(4 * w) + (size_t)(__builtin_ctz(flip) / 8)] ^= 1u;
        else if (w == r.w_bits) f.bits ^= flip;
        else if (w == r.w_bits + 1) f.bits ^= (uint64_t)flip << 32;
        else if (w < r.w_gems) f.beams[(size_t)(w - r.w_beams)] ^= flip;
        else if (w == r.w_gems) f.gems ^= flip;
        expect_scatter(got, f, 3, 0);  // (written field by field: the changed record need not be anybody's pool record)
        const bool in_key = w < r.n_key;
        if (w < r.w_avail) {
            CHECK(sl::occupant_is(who, r, 4u, me) == !in_key);
            CHECK(sl::occupant_is(who, r, sl::TAG_BIT | 3u, me) == !in_key);
            CHECK(sl::same_record(me, sl::PoolRecord{segment, CAP, 4}, r.n_words) == false);
            CHECK(in_key == (w != r.w_gems || collect));  // the gem word is looked at exactly when gems are collected
            compared += 2;
        } else {
            CHECK(sl::occupant_is(who, r, 4u, me));  // the availability words are carried, never compared
        }
    }

    // ---- copy_record: environment 2 into state 5 of a pool that ends with its last word
    std::vector<uint32_t> small((size_t)(r.n_words - 1) * 6 + 6, 0xDEADBEEFu);  // stride 6: word w of state 5 at w * 6 + 5
    sl::copy_record(got.view, r, 2, small.data(), 6, 5);
    for (size_t at = 0; at < small.size(); at++)
        CHECK(small[at] == (at % 6 == 5 ? sl::env_word(got.view, r, 2, (int)(at / 6)) : 0xDEADBEEFu));
    CHECK(sl::same_record(sl::PoolRecord{small.data(), 6, 5}, sl::PoolRecord{segment, CAP, 3}, r.n_words));
    cases++;
}

static void meanings() {
    const sl::RecordLayout r = sl::make_layout(3, 1, true);
    const uint32_t all = 7u | 7u << 16;
    CHECK(sl::is_goal(all, 0x1Fu, r, true, 5) && !sl::is_goal(all, 0x0Fu, r, true, 5) && sl::is_goal(all, 0x0Fu, r, false, 5));
    CHECK(!sl::is_goal(7u | 3u << 16, 0x1Fu, r, false, 5) && sl::is_goal(all, 0xFFFFFFFFu, r, true, 32) && sl::is_goal(all, 0u, r, true, 0));
    // three agents at (0, 1), (1, 2), (2, 0) on a 3 x 3 map
    const uint32_t root[2] = {0u | 1u << 8 | 1u << 16 | 2u << 24, 2u | 0u << 8};
    std::vector<uint8_t> foreign(9, 0);
    CHECK(!sl::root_on_foreign_beam(root, r, foreign.data(), 3, 3));
    foreign[0 * 3 + 1] = sl::foreign_bit(0);  // agent 0 on its own colour
    foreign[1 * 3 + 2] = sl::foreign_bit(1);
    CHECK(!sl::root_on_foreign_beam(root, r, foreign.data(), 3, 3));
    foreign[2 * 3 + 0] = sl::foreign_bit(0);  // agent 2 on agent 0's
    CHECK(sl::root_on_foreign_beam(root, r, foreign.data(), 3, 3));
    CHECK(!sl::root_on_foreign_beam(root, r, foreign.data(), 2, 3));  // (a position outside the map is on no beam)
    foreign[2 * 3 + 0] = 0;
    foreign[1 * 3 + 2] |= sl::foreign_bit(9);  // a colour no agent has
    CHECK(sl::root_on_foreign_beam(root, r, foreign.data(), 3, 3));
    // the table of a pool of `cap` states searched in pieces of `chunk`: the loop lle_search_create used to spell out
    for (uint64_t cap : {1u, 3u, 64u, 65536u})
        for (uint64_t chunk : {1u, 3u, 64u, 65536u}) {
            uint64_t slots = 8;
            while (slots < std::max<uint64_t>(2 * cap, cap + chunk + 1)) slots <<= 1;
            CHECK(sl::table_slots(cap, chunk) == slots && fl::table_slots(cap, chunk) == slots);
        }
}

int main(int argc, char** argv) {
    std::mt19937 rng(argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u);
    for (int A = 1; A <= sl::MAX_AGENTS; A++)
        for (int Lw : {0, 1, 2, sl::MAX_BEAM_WORDS})
            for (int64_t agent_pitch : {2, 4})
                for (int collect = 0; collect < 2; collect++) one_shape(A, Lw, agent_pitch, collect != 0, rng);
    meanings();
    if (failures) {
        std::printf("FAILED %d checks\n", failures);
        return 1;
    }
    std::printf("OK cases=%ld codes=%ld valid=%ld compared=%ld\n", cases, codes_tried, codes_valid, compared);
    return 0;
}
