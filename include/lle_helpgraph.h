/*
 * lle_helpgraph.h -- C ABI of liblle_helpgraph.so: the exact shortest joint plan of a map under a restriction on who may help whom,
 * by breadth-first search over (world state, help relation) through the step kernel of liblle_hip.so.
 *
 * What yamoling/lle answers with the solve modes no-asymmetric, no-mutual (= no-interdependence-2), no-fully-coupled, no-convergence-k
 * and no-divergence-k of its SAT encoding (src/solver/solve_mode.rs; python/lle/characterization/world_characterization.py:
 * is_asymmetric / is_mutual / is_fully_coupled / is_convergent / is_divergent): is there a plan whose trajectory avoids that shape of
 * cooperation.  These five modes depend only on the FLATTENED help relation E of a trajectory -- the set of ordered pairs (helper,
 * beneficiary) over all its states, the reset state included (TemporalCooperationGraph.flattened_edges) -- so a breadth-first search
 * whose states carry E, with whole-record deduplication, is exact: the future of a trajectory depends on nothing else.
 *
 * An eighth library over the public ABI of include/lle_hip.h, like liblle_search.so: it owns an lle_batch of `chunk` environments made
 * with lle_batch_create, writes and reads its five dynamic-state buffers and LLE_BUF_ACTIONS, reads LLE_BUF_ERR, and steps it with
 * lle_batch_step(LLE_STEP_NO_OBS).  Link both (-llle_helpgraph -llle_hip).
 *
 * HELP EDGES of one state are the coop library's (include/lle_coop.h): for every enabled source of colour c whose beam tiles agent c
 * occupies, c helps every other agent that occupies a tile of that source.  Source colours and flags are the map's.
 * A HELP VALUE is 48 bits in two 32-bit words (lo = bits 0-31, hi = bits 32-47): byte h holds the beneficiaries of helper h, bit
 * 8 h + b is set iff h has helped b in some state of the trajectory.
 *
 * A PLAN is as in include/lle_search.h: joint actions from the reset state that World.step accepts, nobody dies, everybody arrives
 * (with collect_gems: and every gem is collected) -- and the help value of its last state is one the mode allows.
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at creation
 * with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_HELPGRAPH_H
#define LLE_HELPGRAPH_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_helpgraph lle_helpgraph;

/* status codes beyond those of lle_hip.h: LLE_SEARCH_CAPACITY of include/lle_search.h, the same value */
#define LLE_HELPGRAPH_CAPACITY (-20) /* more distinct records than max_states: the search has NO answer (never a partial one) */

enum {
    LLE_HELPGRAPH_STANDARD = 0,         /* no restriction: the lengths of lle_search_run(LLE_SEARCH_STANDARD), over more records */
    LLE_HELPGRAPH_NO_ASYMMETRIC = 1,    /* at the END no edge of E has a helper that is nobody's beneficiary (judged at the goal only:
                                           a later edge can repair an earlier one) */
    LLE_HELPGRAPH_NO_MUTUAL = 2,        /* E never holds both (a, b) and (b, a): no-mutual = no-interdependence-2 */
    LLE_HELPGRAPH_NO_FULLY_COUPLED = 3, /* E never holds all A (A - 1) ordered pairs (A >= 2; a map of one agent is never coupled) */
    LLE_HELPGRAPH_NO_CONVERGENCE = 4,   /* no beneficiary ever has `param` or more distinct helpers; param >= 2 */
    LLE_HELPGRAPH_NO_DIVERGENCE = 5     /* no helper ever has `param` or more distinct beneficiaries; param >= 2 */
};
enum { LLE_HELPGRAPH_MAX_AGENTS = 6, LLE_HELPGRAPH_MAX_SOURCES = 32 }; /* 5^6 joint actions per state; one bit per source in a cell's word */

typedef struct lle_helpgraph_options {
    uint32_t struct_bytes; /* sizeof(lle_helpgraph_options) */
    int32_t device;        /* HIP device, or -1: the current one */
    int64_t chunk;         /* environments of the handle's batch = work items per piece; 0: 65 536; 1 .. 2^30 */
    int64_t max_states;    /* records of the pool; 0: 4 194 304; 1 .. 2^30 */
    void* stream;          /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_helpgraph_options;

/* A batch of `chunk` environments of `map`, the pool (one array per record word and two for the help value, parent u32 and action
 * u16 per record), the table (u32 slots, a power of two >= 2 * max_states) and the map's cell table (one u32 per cell: the sources
 * that own a laser tile there).  The map is read now; the handle keeps no pointer to it.  NULL on failure -- no HIP device, more than
 * LLE_HELPGRAPH_MAX_AGENTS agents, more than LLE_HELPGRAPH_MAX_SOURCES sources, out of memory -- and lle_helpgraph_last_error says why. */
lle_helpgraph* lle_helpgraph_create(const lle_map* map, const lle_helpgraph_options* opt);
void lle_helpgraph_free(lle_helpgraph* s);

typedef struct lle_helpgraph_args {
    uint32_t struct_bytes; /* sizeof(lle_helpgraph_args) */
    int32_t mode;          /* LLE_HELPGRAPH_* */
    int32_t param;         /* k of NO_CONVERGENCE / NO_DIVERGENCE, >= 2; ignored by the other modes */
    int32_t collect_gems;  /* != 0: a plan also collects every gem; the gem mask is then part of a record's identity */
    int32_t t_max;         /* longest plan looked for, >= 0 */
} lle_helpgraph_args;
typedef struct lle_helpgraph_result {
    uint32_t struct_bytes; /* sizeof(lle_helpgraph_result) */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max */
    int64_t n_states;      /* distinct records the search has stored */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    int32_t pad;
    int64_t step_errors;   /* work items whose step refused a joint action the availability mask allowed: must be 0 */
    uint32_t help_lo, help_hi; /* the help value of the plan's last state (0 without a plan) */
} lle_helpgraph_result;
/* The search from the reset state, whose help value is that of the reset state itself.  One level = the frontier x every joint action,
 * in pieces of at most `chunk` work items; a piece is four launches (hg_expand, lle_batch_step, hg_insert, hg_commit); the host reads
 * the counters once per level.  A level is always finished before the search stops on a goal, so the per-depth counters do not depend
 * on `chunk`.  Synchronises the stream.  LLE_OK with length >= 0 (solved) or -1 (a reset state the mode rejects, frontier empty, or
 * t_max reached); LLE_HELPGRAPH_CAPACITY when the pool overflowed. */
int lle_helpgraph_run(lle_helpgraph* s, const lle_helpgraph_args* args, lle_helpgraph_result* result);
/* The plan of the last solved run: out[t * A + a] = action of agent a at step t (host memory, length * A bytes, `cap` = its size in
 * bytes).  Returns length (or a negative status; LLE_ERR_ARG when the last run found no plan). */
int lle_helpgraph_plan(const lle_helpgraph* s, uint8_t* out, int64_t cap);
/* Per-depth counters of the last run, as lle_search_stats: frontier[d] = records first reached at depth d (frontier[0] = 1),
 * expanded[d] = available joint actions over the records of depth d.  Writes up to `cap` entries of each; returns the number of
 * frontier entries (depth_reached + 1; expanded has one fewer). */
int lle_helpgraph_stats(const lle_helpgraph* s, int64_t* frontier, int64_t* expanded, int cap);

/* Message of the last failed call of this library on this thread. */
const char* lle_helpgraph_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("hg_expand", "hg_insert<false>":
 * the cell table read from global memory, "hg_insert<true>": staged in LDS, "hg_commit"), NUL-terminated, truncated to `cap`; returns
 * the bytes needed.  lle_helpgraph_debug_compiled lists every kernel the library holds, the same way. */
size_t lle_helpgraph_debug_launched(char* buf, size_t cap);
size_t lle_helpgraph_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_HELPGRAPH_H */
