// policy_values.cpp -- what lle_amd/policy/policy_logic.hpp adds to the search's table code, on the host, built with AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_policy_cpu.py: the packing of a value, the exactness rule at its boundary, and table_find
// on tables built with table_insert (hit, miss, wrap-around, a full table with no match), checked against a std::map.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../lle_amd/policy/policy_logic.hpp"

namespace sl = lle_search_logic;
namespace pl = lle_policy_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static void packing() {
    for (uint32_t steps : {0u, 1u, 32767u, pl::MAX_STEPS})
        for (uint32_t code : {0u, 1u, 15624u}) {
            const uint32_t v = pl::pack_value(steps, code);
            CHECK(v != pl::NO_PLAN && pl::value_steps(v) == steps && pl::value_code(v) == code);
        }
    // the 32-bit minimum is the smallest (steps, code) pair
    CHECK(pl::pack_value(3, 15624) < pl::pack_value(4, 0) && pl::pack_value(3, 7) < pl::pack_value(3, 8) && pl::pack_value(pl::MAX_STEPS, 15624) < pl::NO_PLAN);
    CHECK(pl::stay_code(1) == 4u && pl::stay_code(2) == 24u && pl::stay_code(6) == 15624u);
    for (int A = 1; A <= 6; A++) {  // every digit of the all-STAY code is STAY
        uint32_t code = pl::stay_code(A);
        for (int a = 0; a < A; a++, code /= 5u) CHECK(code % 5u == pl::STAY);
        CHECK(code == 0u);
    }
    bool saturated = false;
    CHECK(pl::relaxed_value(pl::NO_PLAN, 9, &saturated) == pl::NO_PLAN && !saturated);
    CHECK(pl::relaxed_value(pl::pack_value(0, 24), 9, &saturated) == pl::pack_value(1, 9) && !saturated);
    CHECK(pl::relaxed_value(pl::pack_value(32767, 0), 15624, &saturated) == pl::pack_value(32768, 15624) && !saturated);
    CHECK(pl::relaxed_value(pl::pack_value(pl::MAX_STEPS - 1, 0), 3, &saturated) == pl::pack_value(pl::MAX_STEPS, 3) && !saturated);
    CHECK(pl::relaxed_value(pl::pack_value(pl::MAX_STEPS, 0), 3, &saturated) == pl::NO_PLAN && saturated);
}

static void exactness() {
    for (int32_t horizon : {0, 1, 7, 32767})
        for (uint32_t depth = 0; depth <= (uint32_t)horizon && depth < 40; depth++) {
            const uint32_t at = (uint32_t)horizon - depth;  // depth + steps == horizon
            CHECK(pl::value_exact(pl::pack_value(at, 0), depth, horizon, false));
            CHECK(pl::answer_of(pl::pack_value(at, 11), depth, horizon, false) == (int32_t)at);
            CHECK(!pl::value_exact(pl::pack_value(at + 1, 0), depth, horizon, false));  // horizon + 1
            CHECK(pl::answer_of(pl::pack_value(at + 1, 11), depth, horizon, false) == pl::ANSWER_UNKNOWN);
            CHECK(pl::value_exact(pl::pack_value(at + 1, 0), depth, horizon, true));    // complete: every value is exact
            CHECK(pl::answer_of(pl::pack_value(at + 1, 11), depth, horizon, true) == (int32_t)at + 1);
            CHECK(pl::answer_of(pl::NO_PLAN, depth, horizon, false) == pl::ANSWER_UNKNOWN && pl::answer_of(pl::NO_PLAN, depth, horizon, true) == pl::ANSWER_DEAD_END);
            CHECK(!pl::value_exact(pl::NO_PLAN, depth, horizon, false) && pl::value_exact(pl::NO_PLAN, depth, horizon, true));
        }
    CHECK(pl::answer_of(pl::pack_value(pl::MAX_STEPS, 0), 32767, 32767, false) == pl::ANSWER_UNKNOWN);  // (no overflow in depth + steps)
    CHECK(pl::answer_of(pl::pack_value(pl::MAX_STEPS, 0), 32767, 32767, true) == (int32_t)pl::MAX_STEPS);
}

// A table of `slots` slots over records of n_words words (all of them the key), filled with table_insert and committed the way the
// kernels do; then every stored record and as many fresh ones are looked up with table_find.
static void finds(std::mt19937& rng, uint32_t slots, uint32_t n_records, bool degenerate, long& hits, long& misses, long& wraps) {
    const int n_words = 1 + (int)(rng() % 6u);
    std::vector<uint32_t> table(slots, sl::SLOT_EMPTY), pool;  // pool[s * n_words + w]
    std::map<std::vector<uint32_t>, uint32_t> index;
    auto load = [](uint32_t* slot) { return *slot; };
    auto cas = [](uint32_t* slot, uint32_t expected, uint32_t desired) {
        const uint32_t v = *slot;
        if (v == expected) *slot = desired;
        return v;
    };
    auto hash_of = [&](const std::vector<uint32_t>& rec) {
        if (degenerate) return (uint64_t)(slots - 2u);  // every probe sequence starts near the end: it wraps around
        return sl::hash_record([&](int w) { return rec[(size_t)w]; }, n_words);
    };
    auto same = [&](const std::vector<uint32_t>& rec) {
        return [&](uint32_t occupant) {
            CHECK(!(occupant & sl::TAG_BIT) && occupant < index.size());
            for (int w = 0; w < n_words; w++)
                if (pool[(size_t)occupant * n_words + w] != rec[(size_t)w]) return false;
            return true;
        };
    };
    while (index.size() < n_records) {
        std::vector<uint32_t> rec((size_t)n_words);
        for (auto& v : rec) v = rng() % 5u;
        if (rng() % 2u) rec[rng() % (uint32_t)n_words] = rng();
        const int64_t slot = sl::table_insert(table.data(), slots - 1, hash_of(rec), sl::TAG_BIT | 0u, load, cas, [&](uint32_t occupant) {
            return (occupant & sl::TAG_BIT) ? false : same(rec)(occupant);
        });
        CHECK((slot >= 0) == (index.count(rec) == 0));
        if (slot < 0) continue;
        const uint32_t idx = (uint32_t)index.size();
        pool.insert(pool.end(), rec.begin(), rec.end());
        index[rec] = idx;
        table[(size_t)slot] = idx;  // commit
    }
    auto find_load = [](const uint32_t* slot) { return *slot; };
    for (const auto& kv : index) {
        const uint32_t first = (uint32_t)hash_of(kv.first) & (slots - 1);
        const int64_t got = pl::table_find(table.data(), slots - 1, hash_of(kv.first), find_load, same(kv.first));
        CHECK(got == (int64_t)kv.second);
        hits++;
        uint32_t at = 0;
        while (table[at] != kv.second) at++;
        wraps += at < first;  // found behind the end of the table
    }
    for (uint32_t k = 0; k < n_records + 4u; k++) {  // fresh records: the first empty slot ends the probe; in a full table, mask + 1 steps do
        std::vector<uint32_t> rec((size_t)n_words);
        for (auto& v : rec) v = rng();
        if (index.count(rec)) continue;
        CHECK(pl::table_find(table.data(), slots - 1, hash_of(rec), find_load, same(rec)) == pl::FIND_MISSING);
        misses++;
    }
    // a slot that still holds a tag is nobody's record
    if (n_records < slots) {
        std::vector<uint32_t> tagged = table;
        for (auto& v : tagged)
            if (v == sl::SLOT_EMPTY) v = sl::TAG_BIT | 5u;
        const std::vector<uint32_t> rec((size_t)n_words, 0xABCDEF01u);
        if (!index.count(rec)) CHECK(pl::table_find(tagged.data(), slots - 1, hash_of(rec), find_load, same(rec)) == pl::FIND_MISSING);
    }
}

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937 rng(seed);
    packing();
    exactness();
    long hits = 0, misses = 0, wraps = 0, full_tables = 0;
    for (uint32_t slots : {1u, 2u, 8u, 64u, 1024u})
        for (int degenerate = 0; degenerate < 2; degenerate++)
            for (int round = 0; round < 12; round++) {
                const bool full = round % 3 == 0;  // a full table: no empty slot ends a probe
                const uint32_t n_records = full ? slots : (slots == 1u ? 0u : 1u + rng() % (slots - 1u));
                finds(rng, slots, n_records, degenerate != 0, hits, misses, wraps);
                full_tables += full;
            }
    if (failures) return 1;
    std::printf("OK hits=%ld misses=%ld wraps=%ld full=%ld\n", hits, misses, wraps, full_tables);
    return 0;
}
