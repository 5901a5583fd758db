/*
 * lle_helpforest.h -- C ABI of liblle_helpforest.so: the solve modes over the help graph (include/lle_helpgraph.h) and the mode
 * no-sequence-N (include/lle_trails.h) for MANY equally shaped maps at once, one breadth-first tree per map, all trees walked depth
 * by depth in the same launches.
 *
 * What include/lle_forest.h is to include/lle_search.h, for the records that carry a trajectory's past: a filtered generator that
 * keeps the candidates which REQUIRE a shape of cooperation (Asymmetric() & ~Sequential(3), ...) runs hundreds of searches of a few
 * thousand work items each, and one handle per map turns them into tens of thousands of tiny launches.  Here a piece of a level is
 * four launches for the whole forest.
 *
 * A tenth library over the public ABI of include/lle_hip.h: it owns ONE lle_batch made with lle_batch_create_multi(maps, n_maps,
 * envs_per_map); map m owns the environments [m * E, (m + 1) * E).  Per map it keeps a segment of the pool (the search's record, then
 * two more words), parent and action per record, a table of a power of two >= max(2 cap, cap + E + 1) slots, eight counters, and the
 * map's own static data: its cell table (one u32 per cell: the sources that own a laser tile there) and its edge rule (the sources of
 * every colour, the enabled sources).  Two KINDS of record:
 *   help kind   modes LLE_HELPGRAPH_STANDARD .. LLE_HELPGRAPH_NO_DIVERGENCE: the record's two extra words are the help value of
 *               include/lle_helpgraph.h, its identity the search's key words and both of them
 *   trail kind  mode LLE_HELPFOREST_NO_SEQUENCE, param = N (2 .. 16): the one extra word is the trail value of include/lle_trails.h,
 *               the identity the search's key words and that word
 * Per map the answer, the per-depth counters and the number of stored records are exactly what lle_helpgraph_run / lle_trails_run
 * give for that map alone.  A tag in a table is the index of the candidate inside its map's block: a table segment only ever names
 * records of its own map.  Link both (-llle_helpforest -llle_hip; no symbol of the single-map libraries is used).
 *
 * Threading, streams and devices as in lle_forest.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at
 * creation with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_HELPFOREST_H
#define LLE_HELPFOREST_H

#include <stddef.h>
#include <stdint.h>

#include "lle_helpgraph.h"
#include "lle_hip.h"
#include "lle_trails.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_helpforest lle_helpforest;

enum { LLE_HELPFOREST_NO_SEQUENCE = 6 }; /* the mode after the six of include/lle_helpgraph.h: no trail of `param` help edges */
enum { LLE_HELPFOREST_MAX_AGENTS = 6, LLE_HELPFOREST_MAX_SOURCES = 32 };

typedef struct lle_helpforest_options {
    uint32_t struct_bytes;      /* sizeof(lle_helpforest_options) */
    int32_t device;             /* HIP device, or -1: the current one */
    int64_t envs_per_map;       /* E: environments per map = work items of a map per piece; 0: 256; 1 .. 2^30, n_maps * E <= 2^30 */
    int64_t max_states_per_map; /* records of every map's pool segment; 0: 65 536; 1 .. 2^30, max_states_per_map + E < 2^31 */
    void* stream;               /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_helpforest_options;

/* One batch of n_maps * E environments (lle_batch_create_multi) and a segment of every array per map.  The maps are read now; the
 * handle keeps no pointer to them.  They must agree on whatever lle_batch_create_multi requires: its refusal is passed on with its
 * message.  At most LLE_HELPFOREST_MAX_AGENTS agents and LLE_HELPFOREST_MAX_SOURCES sources.  NULL on failure, and
 * lle_helpforest_last_error says why. */
lle_helpforest* lle_helpforest_create(const lle_map* const* maps, int n_maps, const lle_helpforest_options* opt);
void lle_helpforest_free(lle_helpforest* f);

typedef struct lle_helpforest_args {
    uint32_t struct_bytes; /* sizeof(lle_helpforest_args) */
    int32_t mode;          /* LLE_HELPGRAPH_* or LLE_HELPFOREST_NO_SEQUENCE */
    int32_t param;         /* k of no-convergence / no-divergence (>= 2), N of no-sequence (2 .. 16); ignored otherwise */
    int32_t collect_gems;  /* != 0: a plan also collects every gem; the gem mask is then part of a record's identity */
    int32_t t_max;         /* longest plan looked for, >= 0 */
} lle_helpforest_args;

typedef struct lle_helpforest_result {
    int32_t status;        /* 0; LLE_HELPGRAPH_CAPACITY: THIS map met more distinct records than max_states_per_map; LLE_TRAILS_DENSE: the
                              arcs of one state of THIS map allowed more trail extensions than the walk's budget.  Either way no answer */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max (or no answer, or the map was not searched) */
    int64_t n_states;      /* distinct records stored for the map (0: not searched) */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    uint32_t help_lo, help_hi; /* help kind: the help value of the plan's last state (0 without a plan) */
    uint32_t trail;        /* trail kind: the trail value of the plan's last state (0 without a plan) */
} lle_helpforest_result;

/* Every map with search[m] != 0 (search == NULL: every map) from its reset state, with the same arguments.  A level: the host reads
 * every map's counters in one copy, decides each map's fate, writes one descriptor per map in one copy and launches max over the
 * active maps of ceil(items_m / E) pieces; a piece is four launches (hf_expand, lle_batch_step, hf_insert, hf_commit) over all
 * n_maps * E lanes, in which lane k serves map k / E and item piece * E + k % E of it, or idles.  A map stops when it is solved (its
 * level is finished first, so the counters do not depend on E), when its frontier runs empty, at t_max, when its pool overflows or
 * when a walk runs out of budget: that map alone then has a status, no other map is touched.  A map that is not searched is idle from
 * the first level and reports length -1, n_states 0, depth_reached 0, status 0.  The plans of the solved maps are walked on the
 * device in one launch.  Synchronises the stream.  LLE_OK however the maps ended; a negative status when the call itself failed. */
int lle_helpforest_run(lle_helpforest* f, const lle_helpforest_args* args, const uint8_t* search /* n_maps entries, or NULL */,
                       lle_helpforest_result* per_map /* n_maps entries */);
/* The plan of map `map_index` in the last run: out[t * A + a] = action of agent a at step t (host memory, `cap` bytes).  Returns the
 * length (or a negative status; LLE_ERR_ARG when the map has no plan). */
int lle_helpforest_plan(const lle_helpforest* f, int map_index, uint8_t* out, int64_t cap);
/* Per-depth counters of map `map_index` in the last run, as lle_helpgraph_stats gives them.  Returns the number of frontier entries. */
int lle_helpforest_stats(const lle_helpforest* f, int map_index, int64_t* frontier, int64_t* expanded, int cap);
/* The last run: lanes that served a work item, and lanes launched (pieces * n_maps * E, summed over the levels). */
int lle_helpforest_occupancy(const lle_helpforest* f, int64_t* valid_items, int64_t* launched_lanes);

/* Message of the last failed call of this library on this thread. */
const char* lle_helpforest_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("hf_roots", "hf_seed<help>",
 * "hf_seed<trail>", "hf_expand", "hf_insert<help>", "hf_insert<trail>", "hf_commit<help>", "hf_commit<trail>", "hf_plans"),
 * NUL-terminated, truncated to `cap`; returns the bytes needed.  lle_helpforest_debug_compiled lists every kernel the library holds. */
size_t lle_helpforest_debug_launched(char* buf, size_t cap);
size_t lle_helpforest_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_HELPFOREST_H */
