// helpforest_logic.hpp -- the parts of the help forest (helpforest.hip, liblle_helpforest.so) that run the same on the host and on the
// device, beyond what ../forest/forest_logic.hpp (lanes, segments, fates), ../helpgraph/helpgraph_logic.hpp (edge rule, modes, help
// words) and ../trails/trails_logic.hpp (layer_update, the trail word) give: the kinds by number, a map's pool segment, and the one
// fate the trail kind adds.  tests/hostsim/helpforest_pieces.cpp drives all of it under sanitizers.
//
// A tag is LOCAL: TAG_BIT | (k % E), the index of the candidate inside its map's block.  The candidate itself lies in environment
// map * E + tag of the batch, and it expands record desc[map].first_state + (piece * E + tag) / n_joint of the map's own pool segment.
// sl::Piece takes both apart (env0 = map * E, n_tags = E, items = desc[map].items, pool and cap the map's segment), and
// sl::occupant_is over hl::HelpKind or tl::TrailKind compares: nothing of that is the forest's own.
#ifndef LLE_HELPFOREST_LOGIC_HPP
#define LLE_HELPFOREST_LOGIC_HPP

#include <stdint.h>

#include "../forest/forest_logic.hpp"
#include "../helpgraph/helpgraph_logic.hpp"
#include "../search/search_logic.hpp"
#include "../trails/trails_logic.hpp"

namespace lle_helpforest_logic {

namespace sl = lle_search_logic;
namespace fl = lle_forest_logic;
namespace hl = lle_helpgraph_logic;
namespace tl = lle_trails_logic;

enum { KIND_HELP = 0, KIND_TRAIL = 1 };
constexpr int NO_SEQUENCE = hl::N_MODES;  // include/lle_helpforest.h: LLE_HELPFOREST_NO_SEQUENCE, the mode after helpgraph's six
constexpr int N_MODES = hl::N_MODES + 1;
constexpr int EXTRA_WORDS = 2;            // words of a pool record behind the search's: both kinds' segments are laid out for two
constexpr int CNT_DENSE = 5;              // the first counter slot forest_logic.hpp leaves free: work items whose walk ran out of budget
static_assert(CNT_DENSE > fl::CNT_STEP_ERRORS && CNT_DENSE < fl::N_COUNTERS, "forest_logic.hpp has taken the slot");
enum { FATE_DENSE = fl::FATE_STEP_ERROR + 1 };

LLE_SEARCH_HD int kind_of(int mode) { return mode == NO_SEQUENCE ? KIND_TRAIL : KIND_HELP; }
LLE_SEARCH_HD int extra_words(int kind) { return kind == KIND_TRAIL ? 1 : 2; }

// ---- a map's segment of the pool: (n_words + EXTRA_WORDS) arrays of `cap` words
LLE_SEARCH_HD uint64_t pool_segment_offset(int64_t map, int n_words, uint64_t cap) { return (uint64_t)map * (uint64_t)(n_words + EXTRA_WORDS) * cap; }

// ---- per-map fates: fl::advance, and a map whose walk ran out of budget (the trail kind).  Capacity goes first, as in trails.hip:
// a map over capacity AND dense reports capacity.  A dense map ends with `dense_status`, no answer and n_states 1, like a single
// trail search; it reads no counter but its own.
LLE_SEARCH_HD int advance(fl::MapProgress& p, const uint64_t* counters, uint64_t cap, int depth, int capacity_status, int dense_status, int64_t* frontier_new,
                          int64_t* expanded_new) {
    const bool overflow = counters[fl::CNT_OVERFLOW] != 0u || counters[fl::CNT_STATES] > cap;
    if (!overflow && counters[CNT_DENSE] != 0u) {
        p.depth_reached = depth;
        p.active = 0;
        p.status = dense_status;
        p.n_states = 1;
        return FATE_DENSE;
    }
    return fl::advance(p, counters, cap, depth, capacity_status, frontier_new, expanded_new);
}

// A map the caller's mask leaves out: idle from the first level, nothing stored.
LLE_SEARCH_HD fl::MapProgress skipped_progress() {
    fl::MapProgress p = fl::fresh_progress(false);
    p.n_states = 0;
    return p;
}

}  // namespace lle_helpforest_logic
#endif  // LLE_HELPFOREST_LOGIC_HPP
