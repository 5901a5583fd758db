// forest_logic.hpp -- the parts of the forest search (forest.hip, liblle_forest.so) that run the same on the host and on the device:
// which (map, work item) a lane of a piece serves, how many pieces a level takes, where a map's segment of every array begins, and
// what the host makes of a map's counters after a level.  tests/hostsim/forest_pieces.cpp drives them under sanitizers.
//
// The forest searches n_maps maps in lock-step, one tree per map.  The batch has E = envs_per_map environments per map; map m owns
// the environments [m * E, (m + 1) * E).  A level of map m has items_m = frontier_m * 5^A work items; piece q of the level is one
// launch over all n_maps * E lanes, in which lane k serves map k / E and item q * E + k % E of that map -- or nothing, when that item
// is past items_m or the map has stopped.  Every index that combines a map number with a local index is 64-bit.
#ifndef LLE_FOREST_LOGIC_HPP
#define LLE_FOREST_LOGIC_HPP

#include <stdint.h>

#include "../search/search_logic.hpp"

namespace lle_forest_logic {

constexpr int64_t MAX_ENVS_PER_MAP = (int64_t)lle_search_logic::MAX_CHUNK;    // a tag is TAG_BIT | index inside the map's block
constexpr int64_t MAX_STATES_PER_MAP = (int64_t)lle_search_logic::MAX_STATES;
constexpr int64_t MAX_LANES = (int64_t)1 << 30;                                // n_maps * envs_per_map
constexpr uint64_t MAX_TABLE_SLOTS = (uint64_t)1 << 31;                        // per segment: no slot number is SLOT_EMPTY
constexpr int N_COUNTERS = 8;
enum { CNT_STATES = 0, CNT_EXPANDED, CNT_GOAL, CNT_OVERFLOW, CNT_STEP_ERRORS };
constexpr int CNT_DENSE = 5;  // work items whose walk ran out of budget: written and read only where the kind has a walk (the trail kind)
static_assert(CNT_DENSE > CNT_STEP_ERRORS && CNT_DENSE < N_COUNTERS, "the slot is taken");
constexpr uint64_t NO_GOAL = ~(uint64_t)0;

// What the kernels of a level know of one map (one async copy per level).
struct MapDescriptor {
    uint32_t first_state;  // local pool index of the frontier's first state (for forest_plans: the goal state)
    uint32_t active;       // 0: every lane of the map is idle
    uint64_t items;        // frontier size * 5^A (for forest_plans: the plan's length)
};

struct LaneWork {
    int64_t map;      // k / E
    int64_t local;    // k % E: the environment inside the map's block, and the candidate's tag
    uint64_t item;    // q * E + local
    bool idle;        // nothing to do: the item is past the map's items, or the map has stopped
};

LLE_SEARCH_HD LaneWork lane_work(int64_t k, uint64_t piece, int64_t E, const MapDescriptor* desc) {
    LaneWork w;
    w.map = k / E;
    w.local = k % E;
    w.item = piece * (uint64_t)E + (uint64_t)w.local;
    const MapDescriptor& d = desc[w.map];
    w.idle = !d.active || w.item >= d.items;
    return w;
}

// Pieces of a level: the most any active map needs.
LLE_SEARCH_HD uint64_t piece_count(const MapDescriptor* desc, int64_t n_maps, int64_t E) {
    uint64_t pieces = 0;
    for (int64_t m = 0; m < n_maps; m++) {
        if (!desc[m].active) continue;
        const uint64_t need = desc[m].items / (uint64_t)E + (desc[m].items % (uint64_t)E ? 1u : 0u);
        if (need > pieces) pieces = need;
    }
    return pieces;
}

// Lanes of a level that serve an item (the numerator of the occupancy).
LLE_SEARCH_HD uint64_t level_items(const MapDescriptor* desc, int64_t n_maps) {
    uint64_t items = 0;
    for (int64_t m = 0; m < n_maps; m++)
        if (desc[m].active) items += desc[m].items;
    return items;
}

// ---- a map's segment of every array
LLE_SEARCH_HD int64_t env_index(int64_t map, int64_t E, int64_t local) { return map * E + local; }
// word w of local state s: pool[(map * n_words + w) * cap + s] -- structure of arrays inside the segment, as in search.hip
LLE_SEARCH_HD uint64_t pool_index(int64_t map, int n_words, int w, uint64_t cap, uint64_t s) { return ((uint64_t)map * (uint64_t)n_words + (uint64_t)w) * cap + s; }
// a map's segment of the pool: seg_words arrays of `cap` words (the record's n_words, then the library's extra words)
LLE_SEARCH_HD uint64_t pool_segment_offset(int64_t map, int seg_words, uint64_t cap) { return (uint64_t)map * (uint64_t)seg_words * cap; }
LLE_SEARCH_HD uint64_t state_index(int64_t map, uint64_t cap, uint64_t s) { return (uint64_t)map * cap + s; }      // parent, action
LLE_SEARCH_HD uint64_t table_base(int64_t map, uint64_t slots) { return (uint64_t)map * slots; }
LLE_SEARCH_HD uint64_t counter_index(int64_t map, int which) { return (uint64_t)map * N_COUNTERS + (uint64_t)which; }
LLE_SEARCH_HD uint64_t foreign_base(int64_t map, int H, int W) { return (uint64_t)map * (uint64_t)H * (uint64_t)W; }
using lle_search_logic::table_slots;  // (cap, E): a map's table segment is the single search's table with chunk = E

// ---- the host's view of one map during a run
enum { FATE_CONTINUE = 0, FATE_SOLVED, FATE_EMPTY, FATE_CAPACITY, FATE_STEP_ERROR, FATE_DENSE };

struct MapProgress {
    uint64_t level_start, level_end;  // the frontier: local pool indices [level_start, level_end)
    uint64_t expanded_before;
    int32_t active;
    int32_t status;         // 0, the capacity status or the dense status
    int32_t length;         // -1: no plan (yet)
    int32_t depth_reached;
    int64_t n_states;
    uint64_t goal;          // local pool index of the goal state when solved
};

LLE_SEARCH_HD MapProgress fresh_progress(bool searching) {
    MapProgress p;
    p.level_start = 0;
    p.level_end = 1;
    p.expanded_before = 0;
    p.active = searching ? 1 : 0;
    p.status = 0;
    p.length = -1;
    p.depth_reached = 0;
    p.n_states = 1;
    p.goal = NO_GOAL;
    return p;
}

LLE_SEARCH_HD MapDescriptor level_descriptor(const MapProgress& p, uint32_t n_joint) {
    MapDescriptor d;
    d.first_state = (uint32_t)p.level_start;
    d.active = p.active ? 1u : 0u;
    d.items = p.active ? (p.level_end - p.level_start) * (uint64_t)n_joint : 0u;
    return d;
}

// After level `depth` (1-based) of an active map: read its counters, move its frontier on and say what became of it.
// *frontier_new / *expanded_new: the level's entries of the per-depth statistics (written for no fate that ends without an answer).
// dense_status: 0 when the kind has no walk -- the dense counter is not read then.  Otherwise a map whose walk ran out of budget ends
// with it, no answer and n_states 1, like a single trail search.  Capacity goes first: a map over capacity AND dense reports capacity.
LLE_SEARCH_HD int advance(MapProgress& p, const uint64_t* counters, uint64_t cap, int depth, int capacity_status, int dense_status, int64_t* frontier_new,
                          int64_t* expanded_new) {
    p.depth_reached = depth;
    if (counters[CNT_OVERFLOW] != 0u || counters[CNT_STATES] > cap) {
        p.active = 0;
        p.status = capacity_status;
        p.n_states = (int64_t)cap;
        return FATE_CAPACITY;
    }
    if (dense_status != 0 && counters[CNT_DENSE] != 0u) {
        p.active = 0;
        p.status = dense_status;
        p.n_states = 1;
        return FATE_DENSE;
    }
    if (counters[CNT_STEP_ERRORS] != 0u) {
        p.active = 0;
        return FATE_STEP_ERROR;
    }
    *expanded_new = (int64_t)(counters[CNT_EXPANDED] - p.expanded_before);
    p.expanded_before = counters[CNT_EXPANDED];
    const uint64_t new_end = counters[CNT_STATES];
    *frontier_new = (int64_t)(new_end - p.level_end);
    p.n_states = (int64_t)new_end;
    if (counters[CNT_GOAL] != NO_GOAL) {  // the level was finished first: the counters do not depend on E
        p.active = 0;
        p.length = depth;
        p.goal = counters[CNT_GOAL];
        return FATE_SOLVED;
    }
    p.level_start = p.level_end;
    p.level_end = new_end;
    if (p.level_end == p.level_start) {
        p.active = 0;
        return FATE_EMPTY;
    }
    return FATE_CONTINUE;
}

}  // namespace lle_forest_logic
#endif  // LLE_FOREST_LOGIC_HPP
