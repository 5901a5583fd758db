// helpforest_logic.hpp -- the parts of the help forest (helpforest.hip, liblle_helpforest.so) that run the same on the host and on the
// device, beyond what ../forest/forest_logic.hpp (lanes, segments, fates -- the dense one of the trail kind among them),
// ../helpgraph/helpgraph_logic.hpp (edge rule, modes, help words) and ../trails/trails_logic.hpp (layer_update, the trail word) give:
// the kinds by number, the extra words of a segment and a map left out.  tests/hostsim/helpforest_pieces.cpp drives all of it under
// sanitizers.
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

LLE_SEARCH_HD int kind_of(int mode) { return mode == NO_SEQUENCE ? KIND_TRAIL : KIND_HELP; }
LLE_SEARCH_HD int extra_words(int kind) { return kind == KIND_TRAIL ? 1 : 2; }

// A map the caller's mask leaves out: idle from the first level, nothing stored.
LLE_SEARCH_HD fl::MapProgress skipped_progress() {
    fl::MapProgress p = fl::fresh_progress(false);
    p.n_states = 0;
    return p;
}

}  // namespace lle_helpforest_logic
#endif  // LLE_HELPFOREST_LOGIC_HPP
