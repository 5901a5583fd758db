/*
 * lle_policyforest.h -- C ABI of liblle_policyforest.so: one steps-to-go table per map for MANY equally shaped maps, built in the
 * same launches, and a lookup that answers a whole batch of several maps in ONE launch.
 *
 * What include/lle_policy.h answers for one map per handle -- how far from solved is each environment NOW, and which joint action
 * would an expert take there -- for the batch a curriculum steps: lle_batch_create_multi(maps, n_maps, E), map m owning the
 * environments [m * E, (m + 1) * E).  One handle per map turns the build into launches of a few hundred work items and a step into
 * n_maps lookups; here a piece of the build is four launches for all maps and a lookup is one.
 *
 * A fourteenth library over the public ABI of include/lle_hip.h: it owns ONE lle_batch made with lle_batch_create_multi(maps, n_maps,
 * envs_per_map) and keeps, per map, a segment of everything lle_policy keeps: pool records (structure of arrays inside the segment),
 * depth (u16) and value (u32) per state, a table of a power of two >= max(2 cap, cap + E + 1) slots, eight u64 counters, and after
 * the exploration the level starts (u32, at most horizon + 2 per map).  State identity, hashing, tags, the whole-record comparison,
 * the value packing and the EXACTNESS rule are those of lle_policy.h: the table of map m in a forest IS the table lle_policy_build
 * gives for that map alone -- the same states, depths, per-depth counters and, at the fixpoint, the same values.  Link
 * -llle_policyforest -llle_policy -llle_hip (lle_policy_args, the answers, LLE_POLICY_CAPACITY and lle_policy_map_fingerprint come
 * from lle_policy.h; of liblle_policy.so only the host-only fingerprint is called).
 *
 * Threading, streams and devices as in lle_policy.h: a handle is NOT thread-safe; the build's device work is enqueued on the stream
 * given at creation and the build synchronises it, a lookup runs on the stream given to the call; the caller's current device is
 * put back before a call returns.
 */
#ifndef LLE_POLICYFOREST_H
#define LLE_POLICYFOREST_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"
#include "lle_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_policyforest lle_policyforest;

typedef struct lle_policyforest_options {
    uint32_t struct_bytes;      /* sizeof(lle_policyforest_options) */
    int32_t device;             /* HIP device, or -1: the current one */
    int64_t envs_per_map;       /* E: environments per map = work items of a map per piece; 0: 256; 1 .. 2^30, n_maps * E <= 2^30 */
    int64_t max_states_per_map; /* records of every map's pool segment; 0: 65 536; 1 .. 2^30, max_states_per_map + E < 2^31 */
    void* stream;               /* hipStream_t of every launch of the build (NULL: the default stream) */
} lle_policyforest_options;

/* One batch of n_maps * E environments (lle_batch_create_multi) and a segment of every array per map.  The maps are read now; the
 * handle keeps no pointer to them, only lle_policy_map_fingerprint of each.  They must agree on whatever lle_batch_create_multi
 * requires: its refusal is passed on with its message.  At most LLE_POLICY_MAX_AGENTS agents.  NULL on failure, and
 * lle_policyforest_last_error says why. */
lle_policyforest* lle_policyforest_create(const lle_map* const* maps, int n_maps, const lle_policyforest_options* opt);
void lle_policyforest_free(lle_policyforest* pf);

typedef struct lle_policyforest_result {
    int32_t status;        /* 0, or LLE_POLICY_CAPACITY: THIS map met more distinct states than max_states_per_map and has no table */
    int32_t depth_reached; /* levels expanded: the depth at which the frontier ran empty, or horizon (over capacity: where it overflowed) */
    int64_t n_states;      /* distinct states stored for the map (over capacity: max_states_per_map) */
    int32_t complete;      /* 1: the frontier ran empty -- every reachable state is stored and every value is exact */
    int32_t root_steps;    /* what a lookup gives for the reset state: steps >= 0, LLE_POLICY_UNKNOWN or LLE_POLICY_DEAD_END */
    int32_t passes;        /* relaxation passes this map took part in, the last one (which changed nothing for it) included */
    int32_t pad;
} lle_policyforest_result;
typedef struct lle_policyforest_summary {
    uint32_t struct_bytes; /* sizeof(lle_policyforest_summary) */
    int32_t pad;
    int64_t step_errors;   /* work items whose step refused a joint action the availability mask allowed: must be 0 */
    double explore_ms;     /* host wall time of phase A and of phase B (both synchronise) */
    double relax_ms;
    int64_t explore_items; /* phase A: lanes that served a work item, and lanes launched (pieces * n_maps * E) */
    int64_t explore_lanes;
    int64_t relax_items;   /* phase B: the same, over every pass */
    int64_t relax_lanes;
} lle_policyforest_summary;

/* Builds every map's table with one horizon and one collect_gems (replacing the tables of an earlier build).
 * Phase A is the lock-step level loop of lle_forest_run in which a map does not stop at a goal: in piece q lane k serves map k / E and
 * item q * E + k % E of it, or idles; a piece is four launches (pf_expand, lle_batch_step, pf_insert, pf_commit); the host reads every
 * map's counters in one copy per level.  A map stops when its frontier runs empty (complete = 1), at `horizon`, or when its pool
 * overflows: that map alone has status LLE_POLICY_CAPACITY and no table, no other map is touched.  Whole levels are always
 * finished: no per-map figure depends on E.
 * Phase B relaxes all maps in the same launches (pf_expand, lle_batch_step, pf_relax per piece), levels from the deepest expanded one
 * down to 0; at level d the maps with d < depth_reached that have not converged take part, and a lane finds its map's level in the
 * level-start array uploaded once after phase A.  The host reads a changed flag per map once per pass, all maps in one copy; a map
 * leaves the relaxation after a pass that changed nothing for it.  `summary` may be NULL.  Synchronises the stream.
 * LLE_OK however the maps ended; a negative status when the call itself failed (a refused joint action, a plan of more than 65 534
 * steps, a HIP error): then the handle holds no table at all. */
int lle_policyforest_build(lle_policyforest* pf, const lle_policy_args* args, lle_policyforest_result* per_map /* n_maps entries */,
                           lle_policyforest_summary* summary);
/* Per-depth counters of map `map_index` in the last build, as lle_policy_stats gives them.  Returns the number of frontier entries. */
int lle_policyforest_stats(const lle_policyforest* pf, int map_index, int64_t* frontier, int64_t* expanded, int cap);

/* The hot path: ONE launch (pf_lookup, a lane per environment of `batch`) on `stream`, on the handle's device.
 *   map_index == -1   `batch` holds exactly n_maps maps, in the forest's order, with ANY number of environments per map (it need not
 *                     be the forest's E; a wavefront may straddle maps): environment e belongs to map e / (n_envs / n_maps)
 *   map_index >= 0    `batch` is a single-map batch of that map, of any size
 * Environment e answers as lle_policy_lookup does, inside its map's segments: an agent is dead: LLE_POLICY_DEAD_END; its map is over
 * capacity, or its state is not in the map's table: LLE_POLICY_UNKNOWN; otherwise the stored value under the EXACTNESS rule with the
 * map's own `complete`.  For a negative answer every agent's action is STAY (4).  steps_out: int32 [n] device memory, or NULL;
 * actions_out: uint8 device memory with a pitch of action_stride >= n_agents bytes, or NULL (the batch's own LLE_BUF_ACTIONS makes
 * the next lle_batch_step take the expert's actions without a copy).  Nothing but steps_out[e] and the bytes [0, n_agents) of every
 * action row is written; the batch's state buffers are only read.  The batch's strides are queried once per (handle, batch) pair
 * and kept; at every call the kept entry is checked against the batch's LLE_BUF_POS and LLE_BUF_BEAMS descriptors.
 * Refused: no build yet (or a failed one), another number of maps, another agent or beam-word count, another device, map_index out
 * of range.  The MAPS themselves are not compared here: compare lle_policyforest_fingerprints with the batch's maps. */
int lle_policyforest_lookup(lle_policyforest* pf, const lle_batch* batch, int map_index, int32_t* steps_out, uint8_t* actions_out, int64_t action_stride,
                            void* stream);

/* lle_policy_map_fingerprint of every map, as kept at creation: up to `cap` entries into `out` (host memory); returns n_maps. */
int lle_policyforest_fingerprints(const lle_policyforest* pf, uint64_t* out, int cap);

/* Message of the last failed call of this library on this thread. */
const char* lle_policyforest_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("pf_roots", "pf_seed",
 * "pf_expand", "pf_insert", "pf_commit", "pf_relax", "pf_lookup"), NUL-terminated, truncated to `cap`; returns the bytes needed.
 * lle_policyforest_debug_compiled lists every kernel the library holds, the same way. */
size_t lle_policyforest_debug_launched(char* buf, size_t cap);
size_t lle_policyforest_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_POLICYFOREST_H */
