/*
 * lle_search.h -- C ABI of liblle_search.so: the exact shortest joint plan of a map, by breadth-first search over joint states
 * through the step kernel of liblle_hip.so.
 *
 * What yamoling/lle answers with a SAT encoding (python/lle/solver/solver.py: Solver.find_shortest / solve; python/lle/
 * characterization/world_characterization.py: is_solvable / is_cooperative / is_independent): is the map solvable within t_max, how
 * long is the shortest joint plan, is there a plan in which nobody steps into somebody else's beam.  Here the answer is exact with
 * respect to World.step itself: every successor is computed by lle_batch_step.
 *
 * A fifth library over the public ABI of include/lle_hip.h, like liblle_coop.so: it owns an lle_batch of `chunk` environments made
 * with lle_batch_create, writes and reads its five dynamic-state buffers (LLE_BUF_POS, _BITS, _GEMS, _BEAMS, _AVAIL; INTEGRATION.md
 * section 14) and LLE_BUF_ACTIONS, reads LLE_BUF_ERR, and steps it with lle_batch_step(LLE_STEP_NO_OBS).  Link both
 * (-llle_search -llle_hip).
 *
 * A PLAN is a list of joint actions from the reset state: World.step accepts every one, no agent dies at any step, and after the last
 * one every agent has arrived (with collect_gems: and every gem is collected).  A state where everybody has arrived is absorbing
 * (only STAY is available), so a shortest plan padded with all-STAY rows is a plan of any greater length.
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at creation
 * with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_SEARCH_H
#define LLE_SEARCH_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_search lle_search;

/* status codes beyond those of lle_hip.h */
#define LLE_SEARCH_CAPACITY (-20) /* more distinct states than max_states: the search has NO answer (never a partial one) */

enum {
    LLE_SEARCH_STANDARD = 0,       /* SolveMode::Standard */
    LLE_SEARCH_NO_COOPERATION = 1  /* SolveMode::NoCooperation (src/solver/solve_mode.rs:16-17): no state of the plan, the start state
                                      included, has an agent on a beam tile of a source of another colour -- the tiles
                                      lle_map_laser_tiles lists for the map as loaded, whether the beam is on or off */
};
enum { LLE_SEARCH_MAX_AGENTS = 6 }; /* 5^6 = 15 625 joint actions per state */

typedef struct lle_search_options {
    uint32_t struct_bytes; /* sizeof(lle_search_options) */
    int32_t device;        /* HIP device, or -1: the current one */
    int64_t chunk;         /* environments of the handle's batch = work items per piece; 0: 65 536; 1 .. 2^30 */
    int64_t max_states;    /* records of the state pool; 0: 4 194 304; 1 .. 2^30 */
    void* stream;          /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_search_options;

/* A batch of `chunk` environments of `map` (lle_batch_create), the pool (one array per record word, parent u32 and action u16 per
 * state) and the table (u32 slots, a power of two >= 2 * max_states).  The map is read now; the handle keeps no pointer to it.
 * NULL on failure -- no HIP device, more than LLE_SEARCH_MAX_AGENTS agents, out of memory -- and lle_search_last_error says why.
 * The handle's batch never keeps per-environment sources: colours and flags are the map's. */
lle_search* lle_search_create(const lle_map* map, const lle_search_options* opt);
void lle_search_free(lle_search* s);

typedef struct lle_search_args {
    uint32_t struct_bytes; /* sizeof(lle_search_args) */
    int32_t mode;          /* LLE_SEARCH_STANDARD / LLE_SEARCH_NO_COOPERATION */
    int32_t collect_gems;  /* != 0: a plan also collects every gem; the gem mask is then part of a state's identity */
    int32_t t_max;         /* longest plan looked for, >= 0 */
} lle_search_args;
typedef struct lle_search_result {
    uint32_t struct_bytes; /* sizeof(lle_search_result) */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max */
    int64_t n_states;      /* distinct states the search has stored */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    int32_t pad;
    int64_t step_errors;   /* work items whose step refused a joint action the availability mask allowed: must be 0 */
} lle_search_result;
/* The search from the reset state.  One level = the frontier x every joint action, in pieces of at most `chunk` work items; a piece is
 * four launches (expand, lle_batch_step, insert, commit); the host reads five counters once per level.  A level is always finished
 * before the search stops on a goal, so the per-depth counters do not depend on `chunk`.  Synchronises the stream.
 * LLE_OK with length >= 0 (solved) or -1 (frontier empty, or t_max reached); LLE_SEARCH_CAPACITY when the pool overflowed. */
int lle_search_run(lle_search* s, const lle_search_args* args, lle_search_result* result);
/* The plan of the last solved run: out[t * A + a] = action of agent a at step t (host memory, length * A bytes, `cap` = its size in
 * bytes).  Returns length (or a negative status; LLE_ERR_ARG when the last run found no plan). */
int lle_search_plan(const lle_search* s, uint8_t* out, int64_t cap);
/* Per-depth counters of the last run: frontier[d] = states first reached at depth d (frontier[0] = 1), expanded[d] = available joint
 * actions over the states of depth d (sum over states of the product over agents of popcount(avail)), for the depths that were
 * expanded.  Writes up to `cap` entries of each; returns the number of frontier entries (depth_reached + 1; expanded has one fewer). */
int lle_search_stats(const lle_search* s, int64_t* frontier, int64_t* expanded, int cap);

/* Host only (no device needed): the reference's solution_lower_bound (src/solver/context.rs:57-79, 155-180, 523-539) -- the maximum
 * over agents of the walking distance from the start to the nearest exit; walls, voids and sources are not walkable, an exit has no
 * outgoing move, an agent with no reachable exit counts 0.  Negative status on failure. */
int lle_search_lower_bound(const lle_map* map);

/* Message of the last failed call of this library on this thread. */
const char* lle_search_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("search_expand",
 * "search_insert<false>", "search_insert<true>": with the foreign-beam table in LDS, "search_commit"), NUL-terminated, truncated to
 * `cap`; returns the bytes needed.  lle_search_debug_compiled lists every kernel the library holds, the same way. */
size_t lle_search_debug_launched(char* buf, size_t cap);
size_t lle_search_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_SEARCH_H */
