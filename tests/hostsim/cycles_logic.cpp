// cycles_logic.cpp -- lle_amd/cycles/cycles_logic.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: its own main,
// built and run as a child process by tests/test_cycles_cpu.py.  TEST INFRASTRUCTURE.
//
//   cycles_logic CASES
// CASES is a text file the test writes from the restatement (tests/cycles_ref.py), one case per line:
//   A N L  then per layer: m h b ... (m arcs)  then: closed  then (closed = 0): k  a c mask ... (k triples)
// Every case is walked through the packed layer_update in the word class of its agents (A <= 4: 3 words and, every such case again,
// 21 words; above: 21 words), layer by layer as the search does; `closed` must come out at the same layer or never, and the words of
// the last value must be, bit for bit, those an encoder written here from the header's comment makes of the restatement's triples.
// Then, without a file's help: the fold / unfold round trip of every support of every pair, the packed stack at every level, the
// closure at the deepest arc, and a dense made-up state whose first descent is 29 arcs deep and whose walk runs out of budget.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
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

// The layout in the words of the header's comment, with loops over single bits: no code of the header.
int drop_bit(int mask, int k) { return ((mask >> (k + 1)) << k) | (mask & ((1 << k) - 1)); }
void encode(std::vector<uint32_t>& words, int ac, int a, int c, int mask) {
    const int closed_bits = 1 << (ac - 1), open_bits = 1 << (ac - 2);
    CHECK((mask >> a) & 1 && (mask >> c) & 1 && mask < (1 << ac));
    int at, p;
    if (a == c) {
        at = a * closed_bits;
        p = drop_bit(mask, a);
    } else {
        at = ac * closed_bits + (a * (ac - 1) + c - (c > a ? 1 : 0)) * open_bits;
        p = drop_bit(drop_bit(mask, a > c ? a : c), a > c ? c : a);
    }
    words[(size_t)((at + p) >> 5)] |= 1u << ((at + p) & 31);
}

uint64_t arcs_of(const std::vector<std::pair<int, int>>& arcs) {
    uint64_t e = 0;
    for (const auto& hb : arcs) e |= (uint64_t)1 << (8 * hb.first + hb.second);
    return e;
}

struct Case {
    int A, N;
    std::vector<std::vector<std::pair<int, int>>> layers;
    int closed;
    std::vector<std::tuple<int, int, int>> triples;
};

template <int W>
void run_case(const Case& c, long& closed_seen, long& triples_seen) {
    constexpr int AC = cl::Layout<W>::AC;
    const cl::Order order = cl::make_order(c.N);
    std::vector<uint32_t> cur((size_t)W, 0u), next((size_t)W, 0u);
    bool closed = false;
    for (const auto& layer : c.layers) {
        int budget = cl::WALK_BUDGET;
        cl::layer_update<W>([&](int i) { return cur[(size_t)i]; }, cl::Words{next.data(), 1}, arcs_of(layer), order, c.A, budget, closed);
        CHECK(budget >= 0);  // (the test sends no dense case here)
        if (closed) break;
        cur = next;
    }
    CHECK((closed ? 1 : 0) == c.closed);
    if (closed) {
        closed_seen++;
        return;
    }
    std::vector<uint32_t> want((size_t)W, 0u);
    for (const auto& t : c.triples) encode(want, AC, std::get<0>(t), std::get<1>(t), std::get<2>(t));
    CHECK(want == cur);
    triples_seen += (long)c.triples.size();
    // decode: the unfolded supports of every pair are the restatement's masks
    std::set<std::tuple<int, int, int>> got;
    for (int a = 0; a < AC; a++)
        for (int b = 0; b < AC; b++) {
            const uint64_t set = cl::supports<W>([&](int i) { return cur[(size_t)i]; }, a, b);
            for (int m = 0; m < 64; m++)
                if ((set >> m) & 1u) got.insert(std::make_tuple(a, b, m));
        }
    CHECK(got == std::set<std::tuple<int, int, int>>(c.triples.begin(), c.triples.end()));
}

template <int W>
void round_trips() {
    constexpr int AC = cl::Layout<W>::AC;
    for (int a = 0; a < AC; a++)
        for (int b = 0; b < AC; b++)
            for (int mask = 0; mask < (1 << AC); mask++) {
                if (!((mask >> a) & 1) || !((mask >> b) & 1)) continue;
                std::vector<uint32_t> mine((size_t)W, 0u), want((size_t)W, 0u);
                cl::merge_supports<W>(cl::Words{mine.data(), 1}, a, b, (uint64_t)1 << mask);
                encode(want, AC, a, b, mask);
                CHECK(mine == want);
                for (int x = 0; x < AC; x++)
                    for (int y = 0; y < AC; y++)
                        CHECK(cl::supports<W>([&](int i) { return mine[(size_t)i]; }, x, y) == (x == a && y == b ? (uint64_t)1 << mask : 0ull));
            }
    // every field full: all bits of the layout and no other
    std::vector<uint32_t> all((size_t)W, 0u);
    for (int a = 0; a < AC; a++)
        for (int b = 0; b < AC; b++) {
            uint64_t set = 0ull;
            for (int mask = 0; mask < (1 << AC); mask++)
                if (((mask >> a) & 1) && ((mask >> b) & 1)) set |= (uint64_t)1 << mask;
            cl::merge_supports<W>(cl::Words{all.data(), 1}, a, b, set);
        }
    long bits = 0;
    for (uint32_t w : all) bits += __builtin_popcount(w);
    CHECK(bits == cl::Layout<W>::BITS);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    CHECK(in.good());
    long cases = 0, closed_seen = 0, triples_seen = 0, both = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        Case c;
        int L = 0;
        ls >> c.A >> c.N >> L;
        for (int l = 0; l < L; l++) {
            int m = 0;
            ls >> m;
            std::vector<std::pair<int, int>> arcs;
            for (int k = 0; k < m; k++) {
                int h = 0, b = 0;
                ls >> h >> b;
                arcs.emplace_back(h, b);
            }
            c.layers.push_back(arcs);
        }
        int k = 0;
        ls >> c.closed;
        if (!c.closed) {
            ls >> k;
            for (int i = 0; i < k; i++) {
                int a = 0, b = 0, m = 0;
                ls >> a >> b >> m;
                c.triples.emplace_back(a, b, m);
            }
        }
        CHECK(!ls.fail() && c.A >= 2 && c.A <= 6 && c.N >= 2 && c.N <= 6);
        if (c.A <= cl::SMALL_AGENTS) {
            run_case<cl::SMALL_WORDS>(c, closed_seen, triples_seen);
            both++;
        }
        run_case<cl::LARGE_WORDS>(c, closed_seen, triples_seen);
        cases++;
    }

    round_trips<cl::SMALL_WORDS>();
    round_trips<cl::LARGE_WORDS>();
    CHECK(cl::words_of(1) == 3 && cl::words_of(4) == 3 && cl::words_of(5) == 21 && cl::words_of(6) == 21);
    const cl::Order six = cl::make_order(6), three = cl::make_order(3);
    CHECK(six.upto == ~0ull && six.exactly == (uint64_t)1 << 63 && __builtin_popcountll(three.exactly) == 20 && __builtin_popcountll(three.upto) == 1 + 6 + 15 + 20);

    // the packed stack at every level, across the word boundary
    cl::Stack st{0ull, 0ull};
    for (int d = 0; d < 2 * cl::LEVELS_PER_WORD; d++) st.set(d, (d * 5 + 3) & 7);
    for (int d = 0; d < 2 * cl::LEVELS_PER_WORD; d++) CHECK(st.get(d) == ((d * 5 + 3) & 7));
    for (int d = 0; d < 2 * cl::LEVELS_PER_WORD; d += 2) st.set(d, 0);
    for (int d = 0; d < 2 * cl::LEVELS_PER_WORD; d++) CHECK(st.get(d) == (d % 2 ? (d * 5 + 3) & 7 : 0));

    // the REACHED exit: a ring over all six agents closes order 6 at its last arc, and order 5 never (out-of-order: nothing closes)
    uint32_t work[cl::LARGE_WORDS];
    std::vector<std::pair<int, int>> ring;
    for (int a = 0; a < 6; a++) ring.emplace_back(a, (a + 1) % 6);
    for (int n = 2; n <= 6; n++) {
        int budget = cl::WALK_BUDGET;
        bool closed = false;
        cl::layer_update<cl::LARGE_WORDS>(cl::NoWords{}, cl::Words{work, 1}, arcs_of(ring), cl::make_order(n), 6, budget, closed);
        CHECK(budget >= 0 && closed == (n == 6));
    }
    // every arc but 5 -> 0: the first descent from agent 0 is 29 arcs deep (back to 0 from 1, 2, 3 and 4 before agent 5 is met, then
    // every arc among 1 .. 5), nothing closes order 6 on it, and the walk behind it runs out of budget: DENSE, whatever the order allows
    std::vector<std::pair<int, int>> dense;
    for (int h = 0; h < 6; h++)
        for (int b = 0; b < 6; b++)
            if (h != b && !(h == 5 && b == 0)) dense.emplace_back(h, b);
    int dense_runs = 0;
    {
        int budget = cl::WALK_BUDGET;
        bool closed = false;
        cl::layer_update<cl::LARGE_WORDS>(cl::NoWords{}, cl::Words{work, 1}, arcs_of(dense), cl::make_order(6), 6, budget, closed);
        CHECK(budget < 0 && !closed);
        dense_runs++;
        // through the kind: false, no value
        cl::CycleRule rule{};
        rule.order = cl::make_order(6);
        rule.work = work;
        rule.work_stride = 1;
        const cl::CycleKind<cl::LARGE_WORDS> kind(rule);
        cl::CycleKind<cl::LARGE_WORDS>::Value value;
        CHECK(!kind.update(cl::NoWords{}, arcs_of(dense), 6, &value));
        CHECK(kind.update(cl::NoWords{}, arcs_of(ring), 6, &value) && kind.violates(value, 6));
        rule.order = cl::make_order(5);
        const cl::CycleKind<cl::LARGE_WORDS> five(rule);
        CHECK(five.update(cl::NoWords{}, arcs_of(ring), 6, &value) && !five.violates(value, 6) && five.accepts(value, 6));
        CHECK(cl::CycleKind<cl::LARGE_WORDS>::words(value).w[20] == value.w[20] && cl::CycleKind<cl::LARGE_WORDS>::words(value).pick(20) == value.w[20]);
        dense_runs++;
    }
    // the complete digraph of four agents under order 4 closes at once; under order 2 on six agents the pruning keeps the walk short
    std::vector<std::pair<int, int>> k6;
    for (int h = 0; h < 6; h++)
        for (int b = 0; b < 6; b++)
            if (h != b) k6.emplace_back(h, b);
    {
        int budget = cl::WALK_BUDGET;
        bool closed = false;
        cl::layer_update<cl::LARGE_WORDS>(cl::NoWords{}, cl::Words{work, 1}, arcs_of(k6), cl::make_order(2), 6, budget, closed);
        CHECK(budget >= 0 && closed);
    }
    std::printf("OK cases=%ld small_and_large=%ld closed=%ld triples=%ld dense=%d\n", cases, both, closed_seen, triples_seen, dense_runs);
    return 0;
}
