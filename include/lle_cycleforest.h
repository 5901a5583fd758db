/*
 * lle_cycleforest.h -- C ABI of liblle_cycleforest.so: the solve mode no-interdependence-N (include/lle_cycles.h: no closed trail of
 * help events over exactly N distinct agents) for MANY equally shaped maps at once, one breadth-first tree per map, all trees walked
 * depth by depth in the same launches.
 *
 * What include/lle_helpforest.h is to include/lle_helpgraph.h and include/lle_trails.h, for the records that carry the trail triples
 * of their trajectory: a generator that keeps the candidate worlds which REQUIRE a closed chain of help over N agents
 * (Interdependent(3)) runs hundreds of closed-trail searches of a few thousand work items each, and one handle per map turns them
 * into tens of thousands of tiny launches.  Here a piece of a level is four launches for the whole forest.
 *
 * A twelfth library over the public ABI of include/lle_hip.h: it owns ONE lle_batch made with lle_batch_create_multi(maps, n_maps,
 * envs_per_map); map m owns the environments [m * E, (m + 1) * E).  Per map it keeps a segment of the pool (the search's record, then
 * the W value words of include/lle_cycles.h: 3 for maps of up to 4 agents, LLE_CYCLES_VALUE_WORDS = 21 for 5 or 6 -- the maps of a
 * batch agree on their agents, so one W holds for the forest), parent and action per record, a table of a power of two >=
 * max(2 cap, cap + E + 1) slots, eight counters, and the map's own static data: its cell table (one u32 per cell: the sources that own
 * a laser tile there) and its edge rule (the sources of every colour, the enabled sources).  Per map the answer, the per-depth
 * counters and the number of stored records are exactly what lle_cycles_run gives for that map alone.  A tag in a table is the index
 * of the candidate inside its map's block: a table segment only ever names records of its own map.  Link both (-llle_cycleforest
 * -llle_hip; no symbol of liblle_cycles.so is used).
 *
 * Threading, streams and devices as in lle_forest.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at
 * creation with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_CYCLEFOREST_H
#define LLE_CYCLEFOREST_H

#include <stddef.h>
#include <stdint.h>

#include "lle_cycles.h"
#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_cycleforest lle_cycleforest;

typedef struct lle_cycleforest_options {
    uint32_t struct_bytes;      /* sizeof(lle_cycleforest_options) */
    int32_t device;             /* HIP device, or -1: the current one */
    int64_t envs_per_map;       /* E: environments per map = work items of a map per piece; 0: 256; 1 .. 2^30, n_maps * E <= 2^30 */
    int64_t max_states_per_map; /* records of every map's pool segment; 0: 65 536; 1 .. 2^30, max_states_per_map + E < 2^31 */
    void* stream;               /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_cycleforest_options;

/* One batch of n_maps * E environments (lle_batch_create_multi) and a segment of every array per map.  The maps are read now; the
 * handle keeps no pointer to them.  They must agree on whatever lle_batch_create_multi requires: its refusal is passed on with its
 * message.  At most LLE_CYCLES_MAX_AGENTS agents and LLE_CYCLES_MAX_SOURCES sources.  NULL on failure, and
 * lle_cycleforest_last_error says why. */
lle_cycleforest* lle_cycleforest_create(const lle_map* const* maps, int n_maps, const lle_cycleforest_options* opt);
void lle_cycleforest_free(lle_cycleforest* f);

typedef struct lle_cycleforest_args {
    uint32_t struct_bytes; /* sizeof(lle_cycleforest_args) */
    int32_t order_n;       /* N: no closed trail over exactly N agents; LLE_CYCLES_MIN_ORDER .. LLE_CYCLES_MAX_ORDER, at most the maps' agents */
    int32_t collect_gems;  /* != 0: a plan also collects every gem; the gem mask is then part of a record's identity */
    int32_t t_max;         /* longest plan looked for, >= 0 */
} lle_cycleforest_args;

typedef struct lle_cycleforest_result {
    int32_t status;        /* 0; LLE_CYCLES_CAPACITY: THIS map met more distinct records than max_states_per_map; LLE_CYCLES_DENSE: the
                              arcs of one state of THIS map allowed more trail extensions than the walk's budget.  Either way no answer */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max (or no answer, or the map was not searched) */
    int64_t n_states;      /* distinct records stored for the map (0: not searched) */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    int32_t value_words;   /* words of the map's value: 3 or 21, by the maps' agents */
} lle_cycleforest_result;

/* Every map with search[m] != 0 (search == NULL: every map) from its reset state, with the same arguments; levels, pieces, fates and
 * the maps left out exactly as lle_helpforest_run describes them (a piece: cf_expand, lle_batch_step, cf_insert, cf_commit over all
 * n_maps * E lanes).  A reset state whose own arcs run the walk out of budget gives its map LLE_CYCLES_DENSE at once; a reset state
 * that holds a closed trail of order N, or a dead agent, no plan; a reset state that is a goal, length 0.  Synchronises the stream.
 * The arguments are judged before the handle.  LLE_OK however the maps ended; a negative status when the call itself failed. */
int lle_cycleforest_run(lle_cycleforest* f, const lle_cycleforest_args* args, const uint8_t* search /* n_maps entries, or NULL */,
                        lle_cycleforest_result* per_map /* n_maps entries */);
/* The plan of map `map_index` in the last run: out[t * A + a] = action of agent a at step t (host memory, `cap` bytes).  Returns the
 * length (or a negative status; LLE_ERR_ARG when the map has no plan). */
int lle_cycleforest_plan(const lle_cycleforest* f, int map_index, uint8_t* out, int64_t cap);
/* The value of the last state of that plan (include/lle_cycles.h: THE VALUE), as the device stores it: out[0 .. value_words), zeros
 * behind them up to LLE_CYCLES_VALUE_WORDS; all zeros for a map without a plan.  Returns value_words (or a negative status). */
int lle_cycleforest_value(const lle_cycleforest* f, int map_index, uint32_t* out /* LLE_CYCLES_VALUE_WORDS entries */);
/* Per-depth counters of map `map_index` in the last run, as lle_cycles_stats gives them.  Returns the number of frontier entries. */
int lle_cycleforest_stats(const lle_cycleforest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap);
/* The last run: lanes that served a work item, and lanes launched (pieces * n_maps * E, summed over the levels). */
int lle_cycleforest_occupancy(const lle_cycleforest* f, int64_t* valid_items, int64_t* launched_lanes);

/* Message of the last failed call of this library on this thread. */
const char* lle_cycleforest_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("cf_roots", "cf_expand", and
 * "cf_seed<3>", "cf_insert<3>", "cf_commit<3>", "cf_plans<3>" with their twins for 21), NUL-terminated, truncated to `cap`; returns
 * the bytes needed.  lle_cycleforest_debug_compiled lists every kernel the library holds. */
size_t lle_cycleforest_debug_launched(char* buf, size_t cap);
size_t lle_cycleforest_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_CYCLEFOREST_H */
