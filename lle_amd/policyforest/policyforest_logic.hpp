// policyforest_logic.hpp -- what the forest of steps-to-go tables (policyforest.hip, liblle_policyforest.so) adds to the forest's
// lane arithmetic (../forest/forest_logic.hpp) and the table's values (../policy/policy_logic.hpp), the same on the host and on the
// device: which (map, work item) a lane of a relaxation level serves, read from the level-start array; how many pieces such a level
// takes; which maps still relax; which map an environment of a caller's batch belongs to; what a lookup answers from a map's facts.
// tests/hostsim/policyforest_pieces.cpp drives all of it under sanitizers.
//
// After the exploration map m has expanded the levels 0 .. depth_reached[m] - 1; level d is the local pool records
// [level_start[m * stride + d], level_start[m * stride + d + 1]).  Entries past depth_reached[m] + 1 repeat the map's state count, so a
// level the map never expanded has no items.  Every index that combines a map number with a local index is 64-bit.
#ifndef LLE_POLICYFOREST_LOGIC_HPP
#define LLE_POLICYFOREST_LOGIC_HPP

#include <stdint.h>

#include "../forest/forest_logic.hpp"
#include "../policy/policy_logic.hpp"

namespace lle_policyforest_logic {

namespace fl = lle_forest_logic;
namespace pl = lle_policy_logic;

// What the lookup and the relaxation know of one map: written by the host once per build, read by every lane of the map.
struct MapFacts {
    uint64_t pool_offset;    // words before the map's pool segment (fl::pool_segment_offset)
    uint64_t state_offset;   // entries before the map's depth and value segments (fl::state_index of local state 0)
    uint64_t table_offset;   // slots before the map's table segment (fl::table_base)
    uint32_t n_states;       // states stored; 0: no table
    uint32_t complete;       // 1: the map's frontier ran empty
    int32_t status;          // 0, or the capacity status: no table
    uint32_t depth_reached;  // levels expanded
};

// What a relaxation pass knows of one map and leaves behind for it: read back and rewritten once per pass, all maps in one copy.
struct MapPass {
    uint32_t relaxing;   // 1: the map takes part in this pass
    uint32_t changed;    // set by the pass: a value of the map fell
    uint32_t saturated;  // set by the pass: a plan of the map would not fit a value
    uint32_t pad;
};

LLE_SEARCH_HD MapFacts make_facts(int64_t map, int seg_words, uint64_t cap, uint64_t slots, uint32_t n_states, bool complete, int32_t status, uint32_t depth_reached) {
    MapFacts f;
    f.pool_offset = fl::pool_segment_offset(map, seg_words, cap);
    f.state_offset = fl::state_index(map, cap, 0);
    f.table_offset = fl::table_base(map, slots);
    f.n_states = status == 0 ? n_states : 0u;
    f.complete = status == 0 && complete ? 1u : 0u;
    f.status = status;
    f.depth_reached = status == 0 ? depth_reached : 0u;
    return f;
}
LLE_SEARCH_HD bool has_table(const MapFacts& f) { return f.status == 0 && f.n_states > 0u; }

// ---- the relaxation
// Does map m take part in level d of a pass?
LLE_SEARCH_HD bool relaxes_at(const MapFacts& f, const MapPass& pass, uint32_t level) { return pass.relaxing != 0u && has_table(f) && level < f.depth_reached; }
// Work items of level d of map m: its states of depth d times the joint actions.
LLE_SEARCH_HD uint64_t relax_items(const MapFacts& f, const MapPass& pass, const uint32_t* level_start, int64_t stride, int64_t map, uint32_t level, uint32_t n_joint) {
    if (!relaxes_at(f, pass, level)) return 0u;
    const uint32_t* ls = level_start + map * stride;
    return (uint64_t)(ls[level + 1u] - ls[level]) * (uint64_t)n_joint;
}

struct RelaxWork {
    int64_t map, local;    // k / E, k % E
    uint64_t item;         // q * E + local
    uint32_t first_state;  // local pool index of the level's first state of the map
    bool idle;
};
// Lane k of piece q of level d (k < n_maps * E <= 2^30, E <= 2^30: the lane arithmetic fits 32 bits).
LLE_SEARCH_HD RelaxWork relax_work(int64_t k, uint64_t piece, int64_t E, uint32_t level, uint32_t n_joint, const MapFacts* facts, const MapPass* pass,
                                   const uint32_t* level_start, int64_t stride) {
    RelaxWork w;
    const uint32_t map = (uint32_t)k / (uint32_t)E;
    w.map = (int64_t)map;
    w.local = (int64_t)((uint32_t)k - map * (uint32_t)E);
    w.item = piece * (uint64_t)E + (uint64_t)w.local;
    w.first_state = 0u;
    w.idle = true;
    if (!relaxes_at(facts[w.map], pass[w.map], level)) return w;
    const uint32_t* ls = level_start + w.map * stride;
    w.first_state = ls[level];
    w.idle = w.item >= (uint64_t)(ls[level + 1u] - w.first_state) * (uint64_t)n_joint;
    return w;
}
// Pieces of level d of a pass: the most any map that takes part needs.  *items: the lanes that serve an item.
LLE_SEARCH_HD uint64_t relax_piece_count(const MapFacts* facts, const MapPass* pass, const uint32_t* level_start, int64_t stride, int64_t n_maps, int64_t E,
                                         uint32_t level, uint32_t n_joint, uint64_t* items) {
    uint64_t pieces = 0, total = 0;
    for (int64_t m = 0; m < n_maps; m++) {
        const uint64_t n = relax_items(facts[m], pass[m], level_start, stride, m, level, n_joint);
        const uint64_t need = n / (uint64_t)E + (n % (uint64_t)E ? 1u : 0u);
        if (need > pieces) pieces = need;
        total += n;
    }
    if (items) *items = total;
    return pieces;
}
// The deepest level any relaxing map expanded, plus one: a pass walks the levels below it, downwards (0: nobody relaxes).
LLE_SEARCH_HD uint32_t relax_depth(const MapFacts* facts, const MapPass* pass, int64_t n_maps) {
    uint32_t depth = 0;
    for (int64_t m = 0; m < n_maps; m++)
        if (relaxes_at(facts[m], pass[m], 0u) && facts[m].depth_reached > depth) depth = facts[m].depth_reached;
    return depth;
}
// After a pass: a map whose values did not move has converged and leaves; the others clear their flag.  Returns whether the map goes on.
LLE_SEARCH_HD bool next_pass(MapPass& pass) {
    if (pass.relaxing && !pass.changed) pass.relaxing = 0u;
    pass.changed = 0u;
    return pass.relaxing != 0u;
}

// ---- the lookup
// The map of environment e of a caller's batch of n_envs environments: map_index when the batch is that map's alone, otherwise
// e / envs_per_map (envs_per_map = n_envs / n_maps, ANY positive number).  32-bit division where the batch allows it.
LLE_SEARCH_HD int64_t lookup_map(int64_t e, int64_t n_envs, int64_t envs_per_map, int64_t map_index) {
    if (map_index >= 0) return map_index;
    if (n_envs <= (int64_t)0xFFFFFFFFll) return (int64_t)((uint32_t)e / (uint32_t)envs_per_map);
    return e / envs_per_map;
}
// What a lookup answers for an environment of map `f` in which nobody is dead: `found` says whether its state is stored, with value v
// at `depth`.
LLE_SEARCH_HD int32_t map_answer(const MapFacts& f, bool found, uint32_t v, uint32_t depth, int32_t horizon) {
    if (!has_table(f) || !found) return pl::ANSWER_UNKNOWN;
    return pl::answer_of(v, depth, horizon, f.complete != 0u);
}

}  // namespace lle_policyforest_logic
#endif  // LLE_POLICYFOREST_LOGIC_HPP
