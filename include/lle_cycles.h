/*
 * lle_cycles.h -- C ABI of liblle_cycles.so: the exact shortest joint plan of a map in which no CLOSED TRAIL of help events over
 * exactly N distinct agents occurs, by breadth-first search over (world state, trail triples) through the step kernel of liblle_hip.so.
 *
 * What yamoling/lle answers with the solve mode no-interdependence-N of its SAT encoding (src/solver/solve_mode.rs;
 * python/lle/characterization/world_characterization.py: is_interdependent; docs/cooperation-characterization.md, "Interdependence"):
 * is there a plan whose trajectory holds no closed trail of order N.  A TRAIL is a sequence of help edges (helper, beneficiary, t),
 * each starting at the agent the one before ends at, with non-decreasing times, in which no temporal edge is used twice; agents and
 * static arcs may repeat.  A CLOSED trail of order N returns to its first agent and visits exactly N distinct agents
 * (TemporalCooperationGraph.has_closed_trail_of_order).  Orders are not monotone: an order-4 ring need not hold an order-3 trail.
 * Neither the flattened relation of include/lle_helpgraph.h nor the trail lengths of include/lle_trails.h decide this.
 *
 * What a trajectory's past means for its future is the set R of triples (anchor a, current c, support S) such that some trail from a
 * to c visits exactly the agents S.  One more state with arcs E gives
 *   R' = R u { (a, y, S u V(P)) : (a, x, S) in R u {(x, x, {x})}, P a non-empty trail inside E from x to y },
 * P using every arc of E at most once, V(P) the agents P touches.  Under no-interdependence-N:
 *   a triple with |S| > N is never stored, because supports only grow;
 *   a trajectory is dropped the moment some (a, a, S) with |S| = N appears;
 *   kept are (a, c, S) with a != c and |S| <= N, and (a, a, S) with |S| < N.
 * (The closed triples of lower order are needed: a -> b -> a -> c -> a closes order 3 through (a, a, {a, b}).)  The kept triples are
 * part of a record's identity, so a breadth-first search with whole-record deduplication is exact.
 *
 * THE VALUE travels as `value_words` 32-bit words: 3 for maps of up to 4 agents (agent class 4), LLE_CYCLES_VALUE_WORDS = 21 for maps
 * of 5 or 6 agents (agent class 6).  With AC the agent class, a pair (a, c) owns a bitset over the subsets of the REMAINING agents of
 * the class; bit p stands for the support whose agent mask is p with a one inserted at bit min(a, c), then at bit max(a, c) (a = c:
 * at bit a):
 *   closed field a             2^(AC - 1) bits at bit  a * 2^(AC - 1)
 *   open field (a, c), a != c  2^(AC - 2) bits at bit  AC * 2^(AC - 1) + (a * (AC - 1) + c - (c > a)) * 2^(AC - 2)
 * bit k of the value being bit k % 32 of word k / 32.  lle_amd.cycles.triples decodes it.
 *
 * An eleventh library over the public ABI of include/lle_hip.h, like liblle_trails.so: it owns an lle_batch of `chunk` environments
 * made with lle_batch_create, writes and reads its five dynamic-state buffers and LLE_BUF_ACTIONS, reads LLE_BUF_ERR, and steps it
 * with lle_batch_step(LLE_STEP_NO_OBS).  Link both (-llle_cycles -llle_hip).
 *
 * HELP EDGES of one state are the coop library's (include/lle_coop.h); the reset state is t = 0 and its edges count.
 * A PLAN is as in include/lle_search.h -- and no closed trail of order N runs over its states, the reset state included.
 * NO CLOSED TRAIL POSSIBLE: order_n above the map's agents can never be closed; lle_cycles_run refuses it with LLE_ERR_ARG (the plain
 * search of include/lle_search.h is the answer).
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on the stream given at creation
 * with the handle's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_CYCLES_H
#define LLE_CYCLES_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_cycles lle_cycles;

/* status codes beyond those of lle_hip.h */
#define LLE_CYCLES_CAPACITY (-20) /* more distinct records than max_states: the search has NO answer (never a partial one);
                                     LLE_SEARCH_CAPACITY of include/lle_search.h, the same value */
#define LLE_CYCLES_DENSE (-21)    /* the arcs of ONE state allowed more trail extensions than the walk's budget
                                     (LLE_CYCLES_WALK_BUDGET): the search has NO answer (never a partial one) */

enum { LLE_CYCLES_MAX_AGENTS = 6, LLE_CYCLES_MAX_SOURCES = 32 }; /* 5^6 joint actions per state; one bit per source in a cell's word */
enum { LLE_CYCLES_MIN_ORDER = 2, LLE_CYCLES_MAX_ORDER = 6 };     /* N of no-interdependence-N */
enum { LLE_CYCLES_WALK_BUDGET = 4096 }; /* arcs tried by the walk over the arcs of one state (LLE_TRAILS_WALK_BUDGET, the same figure) */
enum { LLE_CYCLES_VALUE_WORDS = 21 };   /* words of the value of the larger agent class */

typedef struct lle_cycles_options {
    uint32_t struct_bytes; /* sizeof(lle_cycles_options) */
    int32_t device;        /* HIP device, or -1: the current one */
    int64_t chunk;         /* environments of the handle's batch = work items per piece; 0: 65 536; 1 .. 2^30 */
    int64_t max_states;    /* records of the pool; 0: 4 194 304; 1 .. 2^30 */
    void* stream;          /* hipStream_t of every launch of the handle (NULL: the default stream) */
} lle_cycles_options;

/* A batch of `chunk` environments of `map`, the pool (one array per record word and per value word, parent u32 and action u16 per
 * record), the table (u32 slots, a power of two >= 2 * max_states) and the map's cell table (one u32 per cell: the sources that own a
 * laser tile there).  The map is read now; the handle keeps no pointer to it.  NULL on failure -- no HIP device, more than
 * LLE_CYCLES_MAX_AGENTS agents, more than LLE_CYCLES_MAX_SOURCES sources, out of memory -- and lle_cycles_last_error says why. */
lle_cycles* lle_cycles_create(const lle_map* map, const lle_cycles_options* opt);
void lle_cycles_free(lle_cycles* s);

typedef struct lle_cycles_args {
    uint32_t struct_bytes; /* sizeof(lle_cycles_args) */
    int32_t order_n;       /* N: no closed trail over exactly N agents; LLE_CYCLES_MIN_ORDER .. LLE_CYCLES_MAX_ORDER, at most the map's agents */
    int32_t collect_gems;  /* != 0: a plan also collects every gem; the gem mask is then part of a record's identity */
    int32_t t_max;         /* longest plan looked for, >= 0 */
} lle_cycles_args;
typedef struct lle_cycles_result {
    uint32_t struct_bytes; /* sizeof(lle_cycles_result) */
    int32_t length;        /* joint actions of the shortest plan; -1: there is none within t_max */
    int64_t n_states;      /* distinct records the search has stored */
    int32_t depth_reached; /* levels expanded: == length when solved, the depth at which the frontier ran empty, or t_max */
    int32_t value_words;   /* words of `value` in use: 3 or 21, by the map's agents */
    uint32_t value[21];    /* the value of the plan's last state (zeros without a plan) */
    int64_t step_errors;   /* work items whose step refused a joint action the availability mask allowed: must be 0 */
} lle_cycles_result;
/* The search from the reset state, whose value is that of the reset state's own arcs.  One level = the frontier x every joint
 * action, in pieces of at most `chunk` work items; a piece is four launches (cy_expand, lle_batch_step, cy_insert, cy_commit); the
 * host reads the counters once per level.  A level is always finished before the search stops on a goal, so the per-depth counters
 * do not depend on `chunk`.  Synchronises the stream.  The arguments are judged before the handle.  LLE_OK with length >= 0 (solved)
 * or -1 (a reset state that holds a closed trail of order N already, frontier empty, or t_max reached); LLE_CYCLES_CAPACITY when the
 * pool overflowed; LLE_CYCLES_DENSE when the walk over one state's arcs ran out of its budget. */
int lle_cycles_run(lle_cycles* s, const lle_cycles_args* args, lle_cycles_result* result);
/* The plan of the last solved run: out[t * A + a] = action of agent a at step t (host memory, length * A bytes, `cap` = its size in
 * bytes).  Returns length (or a negative status; LLE_ERR_ARG when the last run found no plan). */
int lle_cycles_plan(const lle_cycles* s, uint8_t* out, int64_t cap);
/* Per-depth counters of the last run, as lle_search_stats: frontier[d] = records first reached at depth d (frontier[0] = 1),
 * expanded[d] = available joint actions over the records of depth d.  Writes up to `cap` entries of each; returns the number of
 * frontier entries (depth_reached + 1; expanded has one fewer). */
int lle_cycles_stats(const lle_cycles* s, int64_t* frontier, int64_t* expanded, int cap);

/* Message of the last failed call of this library on this thread. */
const char* lle_cycles_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process ("cy_expand", "cy_insert<false, 3>":
 * the cell table read from global memory, "cy_insert<true, 3>": staged in LDS, "cy_commit<3>", and the three with 21 for the larger
 * agent class), NUL-terminated, truncated to `cap`; returns the bytes needed.  lle_cycles_debug_compiled lists every kernel the
 * library holds, the same way. */
size_t lle_cycles_debug_launched(char* buf, size_t cap);
size_t lle_cycles_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_CYCLES_H */
