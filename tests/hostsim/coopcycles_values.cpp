// coopcycles_values.cpp -- the values of the closed-trail cooperation tracker (lle_amd/coopcycles/coopcycles.hip) on the host, under
// AddressSanitizer and UndefinedBehaviorSanitizer: its own main, built and run as a child process by tests/test_coopcycles_cpu.py.
// TEST INFRASTRUCTURE.
//
//   coopcycles_values CASES
// CASES is a text file the test writes from the restatement (tests/coopcycles_ref.py), one case per line:
//   W A L  then per layer: the 48-bit arc word (hex) and the W words (hex) the restatement's encoder makes of R after that layer
// Every case is walked through cl::layer_update<W> as the tracker's kernel calls it: the order {A, every mask, none} that never prunes
// and never closes, a fresh budget per layer, `out` another array than `old`.  The words must be the file's, bit for bit, after every
// layer; the budget may not run out and `closed` may not be set.
// Then, without the file's help: the complete digraph on 4 agents runs out of budget in both word classes, and a layer without an arc
// copies the value and spends nothing.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../lle_amd/cycles/cycles_logic.hpp"

namespace cl = lle_cycles_logic;

#define CHECK(...)                                                                       \
    do {                                                                                 \
        if (!(__VA_ARGS__)) {                                                            \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

namespace {

struct Plain {  // somebody's words as layer_update reads them
    const uint32_t* w;
    uint32_t operator()(int i) const { return w[i]; }
};

struct Counts {
    long cases = 0, layers = 0, max_spent = 0, last_word = 0, closed_triples = 0;
};

template <int W>
void run_case(std::istringstream& in, int A, int L, int line_no, Counts& counts) {
    std::vector<uint32_t> now(W, 0u), next(W, 0u);
    const cl::Order order{A, ~0ull, 0ull};
    for (int l = 0; l < L; l++) {
        uint64_t edges = 0;
        in >> std::hex >> edges;
        std::vector<uint32_t> want(W, 0u);
        for (int i = 0; i < W; i++) in >> std::hex >> want[(size_t)i];
        CHECK(!in.fail());
        int budget = cl::WALK_BUDGET;
        bool closed = false;
        cl::layer_update<W>(Plain{now.data()}, cl::Words{next.data(), 1}, edges, order, A, budget, closed);
        CHECK(budget >= 0 && !closed);
        for (int i = 0; i < W; i++) {
            if (next[(size_t)i] != want[(size_t)i]) {
                std::fprintf(stderr, "line %d layer %d: word %d is %08x, the restatement says %08x\n", line_no, l, i, next[(size_t)i], want[(size_t)i]);
                std::exit(1);
            }
        }
        if (cl::WALK_BUDGET - budget > counts.max_spent) counts.max_spent = cl::WALK_BUDGET - budget;
        now.swap(next);
        counts.layers++;
    }
    counts.last_word += now[(size_t)(W - 1)] != 0u;
    for (int a = 0; a < A; a++) counts.closed_triples += cl::supports<W>(Plain{now.data()}, a, a) != 0ull;
    counts.cases++;
}

template <int W>
void complete_digraph_runs_out(int A) {
    uint64_t edges = 0;
    for (int h = 0; h < 4; h++)
        for (int b = 0; b < 4; b++)
            if (h != b) edges |= (uint64_t)1 << (8 * h + b);
    std::vector<uint32_t> old(W, 0u), out(W, 0u);
    int budget = cl::WALK_BUDGET;
    bool closed = false;
    cl::layer_update<W>(Plain{old.data()}, cl::Words{out.data(), 1}, edges, cl::Order{A, ~0ull, 0ull}, A, budget, closed);
    CHECK(budget < 0 && !closed);
    // a layer without an arc: the value copied, nothing spent
    old[0] = 0x00010203u;
    old[(size_t)(W - 1)] = 0x7u;
    budget = cl::WALK_BUDGET;
    cl::layer_update<W>(Plain{old.data()}, cl::Words{out.data(), 1}, 0ull, cl::Order{A, ~0ull, 0ull}, A, budget, closed);
    CHECK(budget == cl::WALK_BUDGET && out == old);
}

}  // namespace

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream file(argv[1]);
    CHECK(file.good());
    Counts small, large;
    std::string line;
    int line_no = 0;
    while (std::getline(file, line)) {
        line_no++;
        if (line.empty()) continue;
        std::istringstream in(line);
        int W = 0, A = 0, L = 0;
        in >> W >> A >> L;
        CHECK(!in.fail() && A >= 1 && A <= 6 && L >= 0 && (W == cl::SMALL_WORDS || W == cl::LARGE_WORDS) && (W == cl::LARGE_WORDS || A <= cl::SMALL_AGENTS));
        if (W == cl::SMALL_WORDS) run_case<cl::SMALL_WORDS>(in, A, L, line_no, small);
        else run_case<cl::LARGE_WORDS>(in, A, L, line_no, large);
    }
    complete_digraph_runs_out<cl::SMALL_WORDS>(4);
    complete_digraph_runs_out<cl::LARGE_WORDS>(4);
    complete_digraph_runs_out<cl::LARGE_WORDS>(6);
    std::printf("OK small=%ld large=%ld layers=%ld max_spent=%ld last_word=%ld closed=%ld dense=3\n", small.cases, large.cases, small.layers + large.layers,
                std::max(small.max_spent, large.max_spent), small.last_word + large.last_word, small.closed_triples + large.closed_triples);
    return 0;
}
