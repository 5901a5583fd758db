// helpforest_logic.hpp -- the parts of the help forest (helpforest.hip, liblle_helpforest.so) that run the same on the host and on the
// device, beyond what ../forest/forest_logic.hpp (lanes, segments, fates), ../helpgraph/helpgraph_logic.hpp (edge rule, modes, help
// words) and ../trails/trails_logic.hpp (layer_update, the trail word) give: whom the occupant of a slot of ONE MAP's table segment
// names, and the one fate the trail kind adds.  tests/hostsim/helpforest_pieces.cpp drives all of it under sanitizers.
//
// A tag is LOCAL: TAG_BIT | (k % E), the index of the candidate inside its map's block.  The candidate itself lies in environment
// map * E + tag of the batch, and it expands record desc[map].first_state + (piece * E + tag) / n_joint of the map's own pool segment.
// hl::HelpOccupants and tl::TrailOccupants take the environment index for the tag; the functors here take both apart.
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

// ---- the candidates of one map in the piece in flight
struct MapPiece {
    sl::BatchView batch;
    int64_t env0;          // map * E: the first environment of the map's block
    uint32_t n_tags;       // E
    const uint32_t* pool;  // the map's pool segment
    uint64_t stride, cap;  // both `cap`: a segment is as long as its stride
    uint64_t first_state;  // desc[map].first_state
    uint64_t item0;        // piece * E: the first work item of the piece inside the map's level
    uint64_t items;        // desc[map].items: a tag at or past items - item0 names nobody
    uint32_t n_joint;
    int32_t N;             // trail kind: no trail of N edges
};

// The record candidate `tag` expands, in the map's own segment (may be >= cap for a tag that names nobody: the callers check).
LLE_SEARCH_HD uint64_t tag_parent(const MapPiece& o, uint32_t tag) { return o.first_state + (o.item0 + (uint64_t)tag) / o.n_joint; }
LLE_SEARCH_HD bool tag_in_piece(const MapPiece& o, uint32_t tag) { return tag < o.n_tags && o.item0 + (uint64_t)tag < o.items; }

// Is `occupant` the record `me` (a hl::KeyWithHelp over the caller's own record)?  As hl::help_occupant_is, with the tag taken apart:
// the other candidate's key words are read from environment env0 + tag, its help words worked out AGAIN from that environment and the
// candidate's own parent in this map's segment.  Both were written by earlier launches: no lane waits for another.
template <class Me, class Cell>
LLE_SEARCH_HD bool help_occupant_is(const MapPiece& o, const sl::RecordLayout& r, const hl::EdgeRule& e, const Cell& cell, uint32_t occupant, const Me& me) {
    if (occupant & sl::TAG_BIT) {
        const uint32_t tag = occupant & ~sl::TAG_BIT;
        if (!tag_in_piece(o, tag)) return false;
        const int64_t k = o.env0 + (int64_t)tag;
        const sl::EnvRecord other{o.batch, r, k};
        if (!sl::same_record(other, me, r.n_key)) return false;
        const uint64_t parent = tag_parent(o, tag);
        if (parent >= o.cap) return false;
        const uint64_t help = hl::successor_help(o.batch, r, e, cell, o.pool, o.stride, parent, k);
        return hl::help_lo(help) == me(r.n_key) && hl::help_hi(help) == me(r.n_key + 1);
    }
    if (occupant >= o.cap) return false;
    return sl::same_record(hl::PoolKeyWithHelp{o.pool, o.stride, occupant, r.n_key, r.n_words}, me, r.n_key + 2);
}

// Is `occupant` the record `me` (a tl::KeyWithTrail over the caller's own record, whose state has the arcs `edges`)?  As
// tl::trail_occupant_is: equal key words mean equal arcs, so the caller's `edges` are applied to the other candidate's parent.
template <class Me>
LLE_SEARCH_HD bool trail_occupant_is(const MapPiece& o, const sl::RecordLayout& r, uint32_t occupant, const Me& me, uint64_t edges) {
    if (occupant & sl::TAG_BIT) {
        const uint32_t tag = occupant & ~sl::TAG_BIT;
        if (!tag_in_piece(o, tag)) return false;
        const sl::EnvRecord other{o.batch, r, o.env0 + (int64_t)tag};
        if (!sl::same_record(other, me, r.n_key)) return false;
        const uint64_t parent = tag_parent(o, tag);
        if (parent >= o.cap) return false;
        int budget = tl::WALK_BUDGET;
        const uint32_t trail = tl::successor_trail(o.pool, o.stride, r, parent, edges, o.N, budget);
        return budget >= 0 && trail == me(r.n_key);
    }
    if (occupant >= o.cap) return false;
    return sl::same_record(tl::PoolKeyWithTrail{o.pool, o.stride, occupant, r.n_key, r.n_words}, me, r.n_key + 1);
}

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
