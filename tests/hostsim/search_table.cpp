// search_table.cpp -- the table code of the shortest-plan search (lle_amd/search/search_logic.hpp: record hash, probe step, insert) on the
// host, built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_search_cpu.py and checked against a std::set.
//
// Seeded inserts of records of 3 to 40 words into tables of 8, 64 and 4 096 slots, the way the kernels use them: a piece of candidates
// is inserted with tags (TAG_BIT | k, records in a "batch" array), then committed (the winners' records appended to a pool stored as
// structure of arrays, their tags replaced by pool indices).  The records include pairs that differ only in their last key word and,
// with a degenerate hash, records whose hashes are all equal, which forces probing past other records.  Checked: a candidate wins iff
// the std::set has not seen its key, a full table reports INSERT_FULL and nothing else, no slot keeps a tag after a commit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../lle_amd/search/search_logic.hpp"

namespace sl = lle_search_logic;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

struct Run {
    int n_words, n_key;
    uint32_t slots, max_states;
    bool degenerate_hash;
    std::vector<uint32_t> table, pool;  // pool[w * max_states + s]
    uint32_t n_states = 0;
    std::set<std::vector<uint32_t>> seen;

    Run(int n_words_, int n_key_, uint32_t slots_, bool degenerate)
        : n_words(n_words_), n_key(n_key_), slots(slots_), max_states(slots_), degenerate_hash(degenerate), table(slots_, sl::SLOT_EMPTY),
          pool((size_t)n_words_ * slots_, 0u) {}

    // One piece: `batch` holds n records of n_words words.  Returns the number of winners.
    int piece(const std::vector<uint32_t>& batch, int n, bool expect_room) {
        std::vector<int64_t> win((size_t)n, -1);
        auto load = [](uint32_t* slot) { return *slot; };
        auto cas = [](uint32_t* slot, uint32_t expected, uint32_t desired) {
            const uint32_t seen_value = *slot;
            if (seen_value == expected) *slot = desired;
            return seen_value;
        };
        int winners = 0;
        for (int k = 0; k < n; k++) {
            auto me = [&](int w) { return batch[(size_t)k * n_words + w]; };
            auto same_as = [&](uint32_t occupant) {
                for (int w = 0; w < n_key; w++) {
                    const uint32_t other = (occupant & sl::TAG_BIT) ? batch[(size_t)(occupant & ~sl::TAG_BIT) * n_words + w] : pool[(size_t)w * max_states + occupant];
                    if (other != me(w)) return false;
                }
                return true;
            };
            const uint64_t h = degenerate_hash ? 3u : sl::hash_record(me, n_key);
            const int64_t slot = sl::table_insert(table.data(), slots - 1, h, sl::TAG_BIT | (uint32_t)k, load, cas, same_as);
            const std::vector<uint32_t> key(batch.begin() + (size_t)k * n_words, batch.begin() + (size_t)k * n_words + n_key);
            const bool fresh = seen.count(key) == 0;
            if (slot == sl::INSERT_FULL) {
                CHECK(!expect_room && fresh);
                continue;
            }
            CHECK((slot >= 0) == fresh);
            if (slot >= 0) {
                CHECK((uint64_t)slot < slots && table[(size_t)slot] == (sl::TAG_BIT | (uint32_t)k));
                seen.insert(key);
                win[(size_t)k] = slot;
                winners++;
            } else {
                CHECK(slot == sl::INSERT_DUPLICATE);
            }
        }
        for (int k = 0; k < n; k++) {  // commit
            if (win[(size_t)k] < 0) continue;
            const uint32_t idx = n_states++;
            CHECK(idx < max_states);
            for (int w = 0; w < n_words; w++) pool[(size_t)w * max_states + idx] = batch[(size_t)k * n_words + w];
            table[(size_t)win[(size_t)k]] = idx;
        }
        uint32_t occupied = 0;
        for (uint32_t v : table) {
            CHECK(v == sl::SLOT_EMPTY || v < n_states);
            occupied += v != sl::SLOT_EMPTY;
        }
        CHECK(occupied == n_states && n_states == seen.size());
        return winners;
    }
};

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    std::mt19937 rng(seed);
    long inserts = 0, duplicates = 0, full = 0;
    // layouts of real records: A agents, Lw beam words, gems in the key or not -- 3 words (A = 1, Lw = 0) to 40 (A = 6, Lw = 32)
    CHECK(sl::make_layout(1, 0, false).n_key == 3 && sl::make_layout(1, 0, false).n_words == 5);
    CHECK(sl::make_layout(6, 32, true).n_words == sl::MAX_RECORD_WORDS && sl::make_layout(6, 32, true).n_key == 38);
    CHECK(sl::pow5(6) == 15625u && sl::mix64(0) == 0 && sl::mix64(1) != sl::mix64(2));
    for (uint32_t slots : {8u, 64u, 4096u})
        for (int degenerate = 0; degenerate < 2; degenerate++)
            for (int round = 0; round < (slots == 4096u ? (degenerate ? 1 : 6) : 40); round++) {
                const int n_words = 3 + (int)(rng() % 38u);             // 3 .. 40
                const int n_key = 1 + (int)(rng() % (uint32_t)n_words);  // the last words may be carried only
                Run run(n_words, n_key, slots, degenerate != 0);
                const int values = 1 + (int)(rng() % 3u);  // few distinct values per word: many duplicates
                while (run.n_states < slots) {
                    const int room = (int)(slots - run.n_states);
                    const int n = 1 + (int)(rng() % (uint32_t)std::min(room, 300));  // never more fresh records than free slots
                    std::vector<uint32_t> batch((size_t)n * n_words);
                    for (int k = 0; k < n; k++) {
                        const uint32_t how = rng() % 4u;
                        for (int w = 0; w < n_words; w++) batch[(size_t)k * n_words + w] = rng() % (uint32_t)values;
                        if (how == 0 && k > 0) {  // the record before, different in the last key word only
                            for (int w = 0; w < n_words; w++) batch[(size_t)k * n_words + w] = batch[(size_t)(k - 1) * n_words + w];
                            batch[(size_t)k * n_words + n_key - 1] ^= 1u + rng() % 7u;
                        } else if (how == 1) {  // a fresh record for sure
                            batch[(size_t)k * n_words + (rng() % (uint32_t)n_key)] = rng();
                        } else if (how == 2 && k > 0) {  // equal key, other carried words
                            for (int w = 0; w < n_key; w++) batch[(size_t)k * n_words + w] = batch[(size_t)(k - 1) * n_words + w];
                        }
                    }
                    const uint32_t before = run.n_states;
                    const int winners = run.piece(batch, n, true);
                    inserts += n;
                    duplicates += n - winners;
                    CHECK(run.n_states == before + (uint32_t)winners);
                }
                // the table is full now: a fresh record finds no slot, a known one is still a duplicate
                std::vector<uint32_t> batch((size_t)2 * n_words, 0xABCDEF01u);
                const uint32_t known = rng() % slots;
                for (int w = 0; w < n_words; w++) batch[(size_t)n_words + w] = run.pool[(size_t)w * run.max_states + known];
                std::vector<uint32_t> table_before = run.table;
                auto load = [](uint32_t* slot) { return *slot; };
                auto cas = [](uint32_t* slot, uint32_t expected, uint32_t desired) {
                    const uint32_t v = *slot;
                    if (v == expected) *slot = desired;
                    return v;
                };
                for (int k = 0; k < 2; k++) {
                    auto me = [&](int w) { return batch[(size_t)k * n_words + w]; };
                    auto same_as = [&](uint32_t occupant) {
                        for (int w = 0; w < n_key; w++)
                            if (run.pool[(size_t)w * run.max_states + occupant] != me(w)) return false;
                        return true;
                    };
                    const uint64_t h = degenerate ? 3u : sl::hash_record(me, n_key);
                    const int64_t slot = sl::table_insert(run.table.data(), slots - 1, h, sl::TAG_BIT | (uint32_t)k, load, cas, same_as);
                    const std::vector<uint32_t> key(batch.begin() + (size_t)k * n_words, batch.begin() + (size_t)k * n_words + n_key);
                    CHECK(slot == (run.seen.count(key) ? (int64_t)sl::INSERT_DUPLICATE : (int64_t)sl::INSERT_FULL));
                    full += slot == sl::INSERT_FULL;
                }
                CHECK(run.table == table_before);
            }
    if (failures) return 1;
    std::printf("OK inserts=%ld duplicates=%ld full=%ld\n", inserts, duplicates, full);
    return 0;
}
