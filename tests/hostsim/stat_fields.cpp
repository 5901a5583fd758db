// stat_fields.cpp -- the packed counters of a single step (lle_amd/csrc/step_logic.hpp: stat_pack_reward, stat_pack_flags, stat_unpack,
// stat_fields_fit) on the host: the same helpers the step kernels pack with and kernel_common.hpp's flush_stats_packed unpacks with.  Built
// with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_step_epilogue_cpu.py and run as a child process.
//
// A wavefront sums the two words of its lead lanes as they are: for every G in {1, 2, 4, 8, 16} -- 64 / G environments per wavefront,
// per-environment counts of at most G, flags of at most 1 -- the sum of 64 / G packed environments unpacks to the seven plain sums with
// each field in turn at its maximum (the others zero), with all of them at their maxima together, with the hard bound of the event list
// (2 G events) in the three event counts, and with random values below the bounds; one count beyond the 8-bit field does carry, which is
// what stat_fields_fit refuses.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../lle_amd/csrc/step_logic.hpp"

using namespace lle;

static int failures = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            if (++failures > 20) std::exit(1);                                  \
        }                                                                       \
    } while (0)

static long cases = 0;

// order of the fields below: steps, gems, exits, died, invalid, resets, bonus (StepCounts)
struct Counts7 { uint32_t f[7]; };

static void sum_and_compare(const Counts7* envs, int n) {
    uint32_t reward_sum = 0, flags_sum = 0;  // what wave_sum_u32 returns for the two words
    uint64_t plain[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < n; e++) {
        const uint32_t* f = envs[e].f;
        reward_sum += stat_pack_reward(f[1], f[2], f[3], f[6]);
        flags_sum += stat_pack_flags(f[0], f[4], f[5]);
        for (int q = 0; q < 7; q++) plain[q] += f[q];
    }
    const StepCounts c = stat_unpack(reward_sum, flags_sum);
    const uint32_t got[7] = {c.steps, c.gems, c.exits, c.died, c.invalid, c.resets, c.bonus};
    for (int q = 0; q < 7; q++) CHECK(got[q] == plain[q]);
    cases++;
}

int main(int argc, char** argv) {
    std::mt19937 rng(argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u);
    static_assert(stat_fields_fit(64, 1) && stat_fields_fit(4, 16) && stat_fields_fit(4, 32) && stat_fields_fit(1, 255), "");
    static_assert(!stat_fields_fit(64, 4) && !stat_fields_fit(1, 256), "");
    for (uint32_t G : {1u, 2u, 4u, 8u, 16u}) {
        const int n = (int)(64u / G);
        CHECK(stat_fields_fit((uint32_t)n, G) && stat_fields_fit((uint32_t)n, 2u * G));
        Counts7 envs[64];
        for (uint32_t cap : {G, 2u * G}) {  // the bound of the rules, and the bound of the event list's capacity
            const uint32_t top[7] = {1u, cap, cap, cap, 1u, 1u, 1u};
            for (int q = 0; q < 7; q++) {  // one field at its maximum in every environment
                for (int e = 0; e < n; e++)
                    for (int k = 0; k < 7; k++) envs[e].f[k] = k == q ? top[k] : 0u;
                sum_and_compare(envs, n);
            }
            for (int e = 0; e < n; e++)  // all of them together
                for (int k = 0; k < 7; k++) envs[e].f[k] = top[k];
            sum_and_compare(envs, n);
            for (int round = 0; round < 200; round++) {  // anything below, in wavefronts of every size
                const int m = 1 + (int)(rng() % (uint32_t)n);
                for (int e = 0; e < m; e++)
                    for (int k = 0; k < 7; k++) envs[e].f[k] = rng() % (top[k] + 1u);
                sum_and_compare(envs, m);
            }
        }
    }
    // 64 packed words of one environment each, the very sum the issue of the field width is about: 64 in every field
    {
        Counts7 envs[64];
        for (int e = 0; e < 64; e++)
            for (int k = 0; k < 7; k++) envs[e].f[k] = 1u;
        sum_and_compare(envs, 64);
        const StepCounts c = stat_unpack(64u * stat_pack_reward(1, 1, 1, 1), 64u * stat_pack_flags(1, 1, 1));
        CHECK(c.steps == 64 && c.gems == 64 && c.exits == 64 && c.died == 64 && c.invalid == 64 && c.resets == 64 && c.bonus == 64);
    }
    // beyond the bound a field carries into its neighbour: 256 gems read as one exit
    {
        const StepCounts c = stat_unpack(64u * stat_pack_reward(4, 0, 0, 0), 0u);
        CHECK(c.gems == 0 && c.exits == 1);
    }
    if (failures) {
        std::printf("FAILED %d checks\n", failures);
        return 1;
    }
    std::printf("OK cases=%ld\n", cases);
    return 0;
}
