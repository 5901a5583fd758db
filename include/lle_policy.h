/*
 * lle_policy.h -- C ABI of liblle_policy.so: the optimal steps-to-go and an optimal joint action of every environment of a batch,
 * looked up in a table that is built once per map by exhaustive search through the step kernel of liblle_hip.so.
 *
 * liblle_search.so answers "how long is the shortest plan from the reset state".  This library answers the question a training loop
 * asks at every step: how far from solved is each environment NOW, and which joint action would an expert take there -- regret
 * curves, expert demonstrations, exact potentials, and whether an environment can still be solved at all.
 *
 * A seventh library over the public ABI of include/lle_hip.h, like liblle_search.so: it owns an lle_batch of `chunk` environments
 * made with lle_batch_create, writes and reads its five dynamic-state buffers and LLE_BUF_ACTIONS, reads LLE_BUF_ERR and steps it
 * with lle_batch_step(LLE_STEP_NO_OBS).  A lookup only READS the caller's batch (LLE_BUF_POS, _BITS, _GEMS, _BEAMS, through that
 * batch's own descriptors).  Link both (-llle_policy -llle_hip).
 *
 * BUILD, phase A (explore): the level-by-level walk of the search from the reset state that does not stop at a goal.  It runs until
 * the frontier is empty (complete = 1) or `horizon` levels are expanded, and keeps depth[s] of every state.  State identity,
 * hashing and capacity behaviour are the search's (lle_amd/search/search_logic.hpp): successors with a dead agent are dropped, the
 * gem word is part of the identity only with collect_gems, a goal state (everybody arrived; with collect_gems: every gem collected)
 * is stored and expanded like any other -- only STAY is available there, so it finds itself.
 *
 * BUILD, phase B (relax): value[s] is one 32-bit word, (steps << 16) | code, 0xFFFFFFFF for "no plan known"; code is the joint
 * action in base 5, agent 0 the lowest digit (5^6 < 2^16).  A goal state starts at (0 << 16) | all-STAY.  A pass re-expands every
 * expanded state over every available joint action, deepest level first, finds the successor in the (now immutable) table and takes
 * the 32-bit minimum of value[s] and ((steps(successor) + 1) << 16) | code.  Passes repeat until one changes nothing: the fixpoint
 * is the shortest distance in the explored graph and, for every state, the smallest (steps, code) pair over its available joint
 * actions, whatever the order of the updates.  The number of passes depends on scheduling; it is reported, not promised.
 *
 * EXACTNESS: a stored value v of state s is exact iff the table is complete, or depth[s] + steps(v) <= horizon.  (Every state of
 * depth < horizon has been expanded.  A path of the true graph that starts at s and is shorter than steps(v) would reach only
 * states of depth <= depth[s] + its length - 1 < horizon before its last step: it lies wholly among expanded states, its last state
 * is stored, so the relaxation would have found it.)  Everything else reads LLE_POLICY_UNKNOWN; a state of a complete table from
 * which no goal can be reached reads LLE_POLICY_DEAD_END.
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; the build's device work is enqueued on the stream given at
 * creation and the build synchronises it, a lookup runs on the stream given to the call; the caller's current device is put back
 * before a call returns.
 */
#ifndef LLE_POLICY_H
#define LLE_POLICY_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_policy lle_policy;

/* status codes beyond those of lle_hip.h */
#define LLE_POLICY_CAPACITY (-20) /* more distinct states than max_states: there is NO table, and every later lookup is refused */

/* what a lookup writes into steps_out instead of a number of steps */
#define LLE_POLICY_UNKNOWN (-1)  /* the state is not in the table, or its value is not exact (see EXACTNESS) */
#define LLE_POLICY_DEAD_END (-2) /* an agent is dead, or the table is complete and no goal can be reached from the state */

enum { LLE_POLICY_MAX_AGENTS = 6 };     /* 5^6 = 15 625 joint actions per state */
enum { LLE_POLICY_MAX_HORIZON = 32767 };

typedef struct lle_policy_options {
    uint32_t struct_bytes; /* sizeof(lle_policy_options) */
    int32_t device;        /* HIP device, or -1: the current one */
    int64_t chunk;         /* environments of the handle's batch = work items per piece; 0: 65 536; 1 .. 2^30 */
    int64_t max_states;    /* records of the state pool; 0: 4 194 304; 1 .. 2^30 */
    void* stream;          /* hipStream_t of every launch of the build (NULL: the default stream) */
} lle_policy_options;

/* A batch of `chunk` environments of `map` (lle_batch_create), the pool (one array per record word, depth u16 and value u32 per
 * state) and the table (u32 slots, a power of two >= 2 * max_states).  The map is read now; the handle keeps no pointer to it.
 * NULL on failure -- no HIP device, more than LLE_POLICY_MAX_AGENTS agents, more than 32 beam words, out of memory -- and
 * lle_policy_last_error says why. */
lle_policy* lle_policy_create(const lle_map* map, const lle_policy_options* opt);
void lle_policy_free(lle_policy* p);

typedef struct lle_policy_args {
    uint32_t struct_bytes; /* sizeof(lle_policy_args) */
    int32_t collect_gems;  /* != 0: a goal also has every gem collected; the gem mask is then part of a state's identity */
    int32_t horizon;       /* levels expanded at most, 0 .. LLE_POLICY_MAX_HORIZON */
    int32_t pad;
} lle_policy_args;
typedef struct lle_policy_result {
    uint32_t struct_bytes; /* sizeof(lle_policy_result) */
    int32_t depth_reached; /* levels expanded: the depth at which the frontier ran empty, or horizon */
    int64_t n_states;      /* distinct states stored */
    int32_t complete;      /* 1: the frontier ran empty -- every reachable state is stored and every value is exact */
    int32_t passes;        /* relaxation passes, the last one (which changed nothing) included */
    int32_t root_steps;    /* what a lookup gives for the reset state: steps >= 0, LLE_POLICY_UNKNOWN or LLE_POLICY_DEAD_END */
    int32_t pad;
    int64_t step_errors;   /* work items whose step refused a joint action the availability mask allowed: must be 0 */
    double explore_ms;     /* host wall time of phase A and of phase B (both synchronise) */
    double relax_ms;
} lle_policy_result;
/* Builds the table (replacing the one of an earlier build).  A piece of phase A is four launches (policy_expand, lle_batch_step,
 * policy_insert, policy_commit), a piece of phase B three (policy_expand, lle_batch_step, policy_relax); the host reads the counters
 * once per level and once per pass.  Synchronises the stream.  LLE_OK, or LLE_POLICY_CAPACITY when the pool overflowed: then the
 * handle holds no table. */
int lle_policy_build(lle_policy* p, const lle_policy_args* args, lle_policy_result* result);
/* Per-depth counters of the last build: frontier[d] = states first reached at depth d (frontier[0] = 1), expanded[d] = available joint
 * actions over the states of depth d, for the depths that were expanded.  Writes up to `cap` entries of each; returns the number of
 * frontier entries (depth_reached + 1; expanded has one fewer). */
int lle_policy_stats(const lle_policy* p, int64_t* frontier, int64_t* expanded, int cap);

/* The hot path: ONE launch (policy_lookup, a lane per environment) on `stream`, over any lle_batch of the same map, of any size, on
 * the handle's device.  Environment e:
 *   an agent is dead                                   steps_out[e] = LLE_POLICY_DEAD_END
 *   its state is not in the table                      LLE_POLICY_UNKNOWN
 *   stored, no plan known                              LLE_POLICY_DEAD_END when the table is complete, else LLE_POLICY_UNKNOWN
 *   stored, value not exact                            LLE_POLICY_UNKNOWN
 *   otherwise                                          steps >= 0, and actions_out[e * action_stride + a] = the action of agent a
 * For a negative answer every agent's action is STAY (4).  steps_out: int32 [n] device memory, or NULL; actions_out: uint8 device
 * memory with a pitch of action_stride >= n_agents bytes per environment, or NULL -- the batch's own LLE_BUF_ACTIONS (with its own
 * stride) makes the next lle_batch_step take the expert's actions without a copy.  Nothing else is written; the batch's state
 * buffers are only read.  The batch's strides are queried once per (policy, batch) pair and kept; at every call the kept entry is
 * checked against the batch's LLE_BUF_POS and LLE_BUF_BEAMS descriptors (a freed batch's address may serve a new one).
 * Refused: no table (never built, or LLE_POLICY_CAPACITY), a batch of several maps, another agent count or beam-word count,
 * another device.  The MAP itself is not compared here: compare lle_policy_map_fingerprint of the two maps.
 * A batch of several maps (lle_batch_create_multi) is served by liblle_policyforest.so (include/lle_policyforest.h): one table per
 * map, built in the same launches, and one lookup launch over the whole batch. */
int lle_policy_lookup(lle_policy* p, const lle_batch* batch, int32_t* steps_out, uint8_t* actions_out, int64_t action_stride, void* stream);

/* Host only (no device needed): a 64-bit hash of what the public lle_map_* queries say about the map's dynamics -- dimensions and
 * counts of lle_map_info, the positions of every kind, the sources and the laser tiles.  Equal for a clone; 0 on failure. */
uint64_t lle_policy_map_fingerprint(const lle_map* map);

/* Message of the last failed call of this library on this thread. */
const char* lle_policy_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("policy_expand", "policy_insert",
 * "policy_commit", "policy_relax", "policy_lookup"), NUL-terminated, truncated to `cap`; returns the bytes needed.
 * lle_policy_debug_compiled lists every kernel the library holds, the same way. */
size_t lle_policy_debug_launched(char* buf, size_t cap);
size_t lle_policy_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_POLICY_H */
