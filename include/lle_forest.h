/*
 * lle_forest.h -- C ABI of liblle_forest.so: the exact shortest joint plans of MANY equally shaped maps at once, one breadth-first
 * tree per map, all trees walked depth by depth in the same launches.
 *
 * What include/lle_search.h answers for one map per handle, for the workload of a filtered generator (python/lle/generator/ of
 * yamoling/lle: sample candidate layouts by the hundred, keep those a Constraint accepts): hundreds of searches of a few thousand work
 * items each, which one handle per map turns into tens of thousands of tiny launches.  Here a piece of a level is four launches for
 * the whole forest.
 *
 * A sixth library over the public ABI of include/lle_hip.h: it owns ONE lle_batch made with lle_batch_create_multi(maps, n_maps,
 * envs_per_map); map m owns the environments [m * E, (m + 1) * E).  Per map it keeps a segment of everything lle_search keeps: pool
 * records (structure of arrays), parent and action per state, a table of a power of two >= max(2 cap, cap + E + 1) slots, eight
 * counters and the foreign-beam table.  Table, tags (the index of the candidate inside its map's block), whole-record comparison and
 * the record layout are those of lle_search: per map the answer, the per-depth counters and the number of stored states are exactly
 * what lle_search_run gives for that map alone.  Link both (-llle_forest -llle_hip; the modes, lle_search_args and
 * LLE_SEARCH_CAPACITY come from lle_search.h, no symbol of liblle_search.so is used).
 *
 * Threading, streams and devices as in lle_search.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at
 * creation with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_FOREST_H
#define LLE_FOREST_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"
#include "lle_search.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_forest lle_forest;

typedef struct lle_forest_options {
    uint32_t struct_bytes;      /* sizeof(lle_forest_options) */
    int32_t device;             /* HIP device, or -1: the current one */
    int64_t envs_per_map;       /* E: environments per map = work items of a map per piece; 0: 256; 1 .. 2^30, n_maps * E <= 2^30 */
    int64_t max_states_per_map; /* records of every map's pool segment; 0: 65 536; 1 .. 2^30, max_states_per_map + E < 2^31 */
    void* stream;               /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_forest_options;

/* One batch of n_maps * E environments (lle_batch_create_multi) and a segment of every array per map.  The maps are read now; the
 * handle keeps no pointer to them.  They must agree on whatever lle_batch_create_multi requires (height, width, numbers of agents,
 * sources and gems, the layout of the beam words, the row alignment): its refusal is passed on with its message.  At most
 * LLE_SEARCH_MAX_AGENTS agents.  NULL on failure, and lle_forest_last_error says why. */
lle_forest* lle_forest_create(const lle_map* const* maps, int n_maps, const lle_forest_options* opt);
void lle_forest_free(lle_forest* f);

typedef struct lle_forest_result {
    int32_t status;        /* 0, or LLE_SEARCH_CAPACITY: THIS map met more distinct states than max_states_per_map and has no answer */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max (or no answer) */
    int64_t n_states;      /* distinct states stored for the map */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    int32_t pad;
} lle_forest_result;

/* Every map from its reset state, with the same t_max, mode and collect_gems.  A level: the host reads every map's counters in one
 * copy, decides each map's fate, writes one descriptor per map in one copy and launches max over the active maps of
 * ceil(items_m / E) pieces; a piece is four launches (expand, lle_batch_step, insert, commit) over all n_maps * E lanes, in which
 * lane k serves map k / E and item piece * E + k % E of it, or idles.  A map stops when it is solved (its level is finished first,
 * so the counters do not depend on E), when its frontier runs empty, at t_max, or when its pool overflows: that map alone then has
 * status LLE_SEARCH_CAPACITY, no other map is touched.  The plans of the solved maps are walked on the device in one launch and
 * come back in one copy.  Synchronises the stream.  LLE_OK however the maps ended; a negative status when the call itself failed
 * (a step that refused an allowed joint action, a HIP error). */
int lle_forest_run(lle_forest* f, const lle_search_args* args, lle_forest_result* per_map /* n_maps entries */);
/* The plan of map `map_index` in the last run: out[t * A + a] = action of agent a at step t (host memory, `cap` bytes).  Returns the
 * length (or a negative status; LLE_ERR_ARG when the map has no plan). */
int lle_forest_plan(const lle_forest* f, int map_index, uint8_t* out, int64_t cap);
/* Per-depth counters of map `map_index` in the last run, as lle_search_stats gives them.  Returns the number of frontier entries. */
int lle_forest_stats(const lle_forest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap);
/* The last run: lanes that served a work item, and lanes launched (pieces * n_maps * E, summed over the levels). */
int lle_forest_occupancy(const lle_forest* f, int64_t* valid_items, int64_t* launched_lanes);

/* Message of the last failed call of this library on this thread. */
const char* lle_forest_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("forest_roots", "forest_seed",
 * "forest_expand", "forest_insert<false>", "forest_insert<true>": mode no-cooperation, "forest_commit", "forest_plans"),
 * NUL-terminated, truncated to `cap`; returns the bytes needed.  lle_forest_debug_compiled lists every kernel the library holds. */
size_t lle_forest_debug_launched(char* buf, size_t cap);
size_t lle_forest_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_FOREST_H */
