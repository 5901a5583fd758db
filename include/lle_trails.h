/*
 * lle_trails.h -- C ABI of liblle_trails.so: the exact shortest joint plan of a map in which no SEQUENCE of N help events occurs, by
 * breadth-first search over (world state, trail lengths) through the step kernel of liblle_hip.so.
 *
 * What yamoling/lle answers with the solve mode no-sequence[-N] of its SAT encoding (src/solver/solve_mode.rs:
 * NoSequentialCooperation; python/lle/characterization/world_characterization.py: is_sequential): is there a plan whose trajectory
 * holds no trail of N help edges.  A TRAIL is a sequence of help edges (helper, beneficiary, t), each starting at the agent the one
 * before ends at, with non-decreasing times, in which no temporal edge is used twice; agents and static arcs may repeat
 * (TemporalCooperationGraph.longest_trail).  Unlike the modes of include/lle_helpgraph.h this depends on the ORDER of the help events:
 * the flattened relation does not decide it.
 *
 * What a trajectory's past means for its future is one small vector: L[a] = the length of the longest trail that ends at agent a.
 * A new state with arc set E updates it by  L'[y] = max(L[y], max over x and over trails P inside E from x to y of L[x] + |P|):
 * edges of different time steps are distinct by construction, so only the segment inside one state needs the no-edge-twice
 * bookkeeping, and that segment lives in a digraph of at most A (A - 1) = 30 arcs.  A breadth-first search whose records carry L, with
 * whole-record deduplication, is therefore exact.  L only grows: a trajectory is dropped the moment some L[a] reaches N.
 *
 * A ninth library over the public ABI of include/lle_hip.h, like liblle_helpgraph.so: it owns an lle_batch of `chunk` environments
 * made with lle_batch_create, writes and reads its five dynamic-state buffers and LLE_BUF_ACTIONS, reads LLE_BUF_ERR, and steps it
 * with lle_batch_step(LLE_STEP_NO_OBS).  Link both (-llle_trails -llle_hip).
 *
 * HELP EDGES of one state are the coop library's (include/lle_coop.h), as in include/lle_helpgraph.h; the reset state is t = 0 and its
 * edges count.
 * A TRAIL VALUE is one 32-bit word, 4 bits per agent: bits 4 a .. 4 a + 3 hold L[a].  A stored record never holds more than
 * N - 1 <= 15 in a field: a record with a field at N is dropped.
 *
 * A PLAN is as in include/lle_search.h: joint actions from the reset state that World.step accepts, nobody dies, everybody arrives
 * (with collect_gems: and every gem is collected) -- and the longest trail over its states, the reset state included, is shorter
 * than N.
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at creation
 * with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_TRAILS_H
#define LLE_TRAILS_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_trails lle_trails;

/* status codes beyond those of lle_hip.h */
#define LLE_TRAILS_CAPACITY (-20) /* more distinct records than max_states: the search has NO answer (never a partial one);
                                     LLE_SEARCH_CAPACITY of include/lle_search.h, the same value */
#define LLE_TRAILS_DENSE (-21)    /* the arcs of ONE state allowed more trail extensions than the walk's budget
                                     (LLE_TRAILS_WALK_BUDGET): the search has NO answer (never a partial one) */

enum { LLE_TRAILS_MAX_AGENTS = 6, LLE_TRAILS_MAX_SOURCES = 32 }; /* 5^6 joint actions per state; one bit per source in a cell's word */
enum { LLE_TRAILS_MIN_LENGTH = 2, LLE_TRAILS_MAX_LENGTH = 16 };  /* N of no-sequence-N: a field of the trail value has 4 bits */
enum { LLE_TRAILS_WALK_BUDGET = 4096 }; /* arc extensions of the walk over the arcs of one state; a state of at most 6 arcs never
                                           needs more than 1 956 (the ordered choices of distinct arcs) */

typedef struct lle_trails_options {
    uint32_t struct_bytes; /* sizeof(lle_trails_options) */
    int32_t device;        /* HIP device, or -1: the current one */
    int64_t chunk;         /* environments of the handle's batch = work items per piece; 0: 65 536; 1 .. 2^30 */
    int64_t max_states;    /* records of the pool; 0: 4 194 304; 1 .. 2^30 */
    void* stream;          /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_trails_options;

/* A batch of `chunk` environments of `map`, the pool (one array per record word and one for the trail value, parent u32 and action
 * u16 per record), the table (u32 slots, a power of two >= 2 * max_states) and the map's cell table (one u32 per cell: the sources
 * that own a laser tile there).  The map is read now; the handle keeps no pointer to it.  NULL on failure -- no HIP device, more than
 * LLE_TRAILS_MAX_AGENTS agents, more than LLE_TRAILS_MAX_SOURCES sources, out of memory -- and lle_trails_last_error says why. */
lle_trails* lle_trails_create(const lle_map* map, const lle_trails_options* opt);
void lle_trails_free(lle_trails* s);

typedef struct lle_trails_args {
    uint32_t struct_bytes; /* sizeof(lle_trails_args) */
    int32_t length_n;      /* N: no trail of N help edges; LLE_TRAILS_MIN_LENGTH .. LLE_TRAILS_MAX_LENGTH */
    int32_t collect_gems;  /* != 0: a plan also collects every gem; the gem mask is then part of a record's identity */
    int32_t t_max;         /* longest plan looked for, >= 0 */
} lle_trails_args;
typedef struct lle_trails_result {
    uint32_t struct_bytes; /* sizeof(lle_trails_result) */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max */
    int64_t n_states;      /* distinct records the search has stored */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    uint32_t trail;        /* the trail value of the plan's last state (0 without a plan) */
    int64_t step_errors;   /* work items whose step refused a joint action the availability mask allowed: must be 0 */
} lle_trails_result;
/* The search from the reset state, whose trail value is that of the reset state's own arcs.  One level = the frontier x every joint
 * action, in pieces of at most `chunk` work items; a piece is four launches (tr_expand, lle_batch_step, tr_insert, tr_commit); the
 * host reads the counters once per level.  A level is always finished before the search stops on a goal, so the per-depth counters
 * do not depend on `chunk`.  Synchronises the stream.  LLE_OK with length >= 0 (solved) or -1 (a reset state that holds a trail of N
 * already, frontier empty, or t_max reached); LLE_TRAILS_CAPACITY when the pool overflowed; LLE_TRAILS_DENSE when the walk over one
 * state's arcs ran out of its budget. */
int lle_trails_run(lle_trails* s, const lle_trails_args* args, lle_trails_result* result);
/* The plan of the last solved run: out[t * A + a] = action of agent a at step t (host memory, length * A bytes, `cap` = its size in
 * bytes).  Returns length (or a negative status; LLE_ERR_ARG when the last run found no plan). */
int lle_trails_plan(const lle_trails* s, uint8_t* out, int64_t cap);
/* Per-depth counters of the last run, as lle_search_stats: frontier[d] = records first reached at depth d (frontier[0] = 1),
 * expanded[d] = available joint actions over the records of depth d.  Writes up to `cap` entries of each; returns the number of
 * frontier entries (depth_reached + 1; expanded has one fewer). */
int lle_trails_stats(const lle_trails* s, int64_t* frontier, int64_t* expanded, int cap);

/* Message of the last failed call of this library on this thread. */
const char* lle_trails_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("tr_expand", "tr_insert<false>":
 * the cell table read from global memory, "tr_insert<true>": staged in LDS, "tr_commit"), NUL-terminated, truncated to `cap`; returns
 * the bytes needed.  lle_trails_debug_compiled lists every kernel the library holds, the same way. */
size_t lle_trails_debug_launched(char* buf, size_t cap);
size_t lle_trails_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_TRAILS_H */
