// episode_ops.cpp -- lle_amd/coop/episode_ops.hpp on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: its own main,
// built and run as a child process by tests/test_coop_cpu.py.  TEST INFRASTRUCTURE.
//
//   episode_ops CASES
// CASES is a text file the test writes, one case per line:
//   ops OPS FLAGS EVCOUNT ERR S0 S1 S2   the operations, the flags and the environment's two bytes of one update call (hex), and the
//                                         operations the environment runs in stages 0, 1 and 2 by the order of tests/cooptrails_ref.py
//   layout K SIZE...                      K array sizes in bytes; the offsets and the total of guarded_layout go to stdout as
//                                         "layout K OFFSET... TOTAL" for the test to judge
// A byte whose flag is not set is handed over as a NULL address: the decode may not read it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../lle_amd/coop/episode_ops.hpp"

namespace eo = lle_episode_ops;

#define CHECK(...)                                                                       \
    do {                                                                                 \
        if (!(__VA_ARGS__)) {                                                            \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream file(argv[1]);
    CHECK(file.good());
    long decoded = 0, layouts = 0, unread = 0;
    std::string line;
    for (int line_no = 1; std::getline(file, line); line_no++) {
        std::istringstream in(line);
        std::string kind;
        in >> kind;
        if (kind == "ops") {
            uint32_t ops = 0, flags = 0, evcount = 0, err = 0, want[eo::STAGES] = {0, 0, 0};
            in >> std::hex >> ops >> flags >> evcount >> err >> want[0] >> want[1] >> want[2];
            CHECK(!in.fail() && evcount < 256u && err < 256u);
            // each byte alone on the heap, so that a read beside it is caught; no address at all where the flag does not ask
            std::vector<uint8_t> ev(1, (uint8_t)evcount), er(1, (uint8_t)err);
            const uint8_t* ev_at = (flags & eo::HONOUR_AUTO_RESET) ? ev.data() : nullptr;
            const uint8_t* er_at = (flags & eo::SKIP_REFUSED) ? er.data() : nullptr;
            unread += (ev_at == nullptr) + (er_at == nullptr);
            const uint32_t reset_ops = eo::reset_ops(flags, ev_at), own_ops = eo::own_ops(ops, flags, er_at);
            for (int stage = 0; stage < eo::STAGES; stage++) {
                const uint32_t got = eo::stage_ops(reset_ops, own_ops, stage);
                if (got != want[stage]) {
                    std::fprintf(stderr, "line %d stage %d: %x, expected %x\n", line_no, stage, got, want[stage]);
                    return 1;
                }
            }
            // a library without SKIP_REFUSED (coop.hip) runs stages 1 and 2 as one: the caller's operations whole
            CHECK((eo::stage_ops(reset_ops, ops, 1) | eo::stage_ops(reset_ops, ops, 2)) == ops && eo::stage_ops(reset_ops, ops, 0) == reset_ops);
            decoded++;
        } else if (kind == "layout") {
            int k = 0;
            in >> std::dec >> k;
            CHECK(!in.fail() && k >= 1 && k <= 16);
            std::vector<size_t> sizes((size_t)k), offsets((size_t)k);
            for (auto& s : sizes) in >> s;
            CHECK(!in.fail());
            const size_t total = eo::guarded_layout(sizes.data(), k, 256, offsets.data());
            std::printf("layout %d", k);
            for (size_t o : offsets) std::printf(" %zu", o);
            std::printf(" %zu\n", total);
            layouts++;
        } else {
            CHECK(kind.empty());
        }
    }
    CHECK(eo::clean_row(0xFFFFFFFFu, 0, 1) == 0u && eo::clean_row(0xFFFFFFFFu, 2, 3) == 3u && eo::clean_row(0xFFFFFFFFu, 15, 16) == 0x7FFFu);
    CHECK(eo::ALL_OPS == (eo::FINISH | eo::CLEAR | eo::MARK_STARTS | eo::MARK_POS));
    std::printf("OK decoded=%ld layouts=%ld unread=%ld\n", decoded, layouts, unread);
    return 0;
}
