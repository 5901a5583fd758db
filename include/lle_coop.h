/*
 * lle_coop.h -- C ABI of liblle_coop.so: who helps whom, for every environment of an lle_batch, in one launch per step.
 *
 * The cooperation analysis of yamoling/lle (python/lle/characterization/plan/: detect_dependencies, analyser.py:31-60;
 * TemporalCooperationGraph.flattened_edges / max_distinct_helpers / max_distinct_beneficiaries / asymmetric_edges,
 * graph.py:92-151) without its solver: the per-state detection and the per-episode degree profile are pure functions of state the
 * batch already holds on the device.
 *
 * A fourth library over the public ABI of include/lle_hip.h, like liblle_render.so and liblle_shaping.so: it reads a batch only
 * through lle_batch_get_buffer (LLE_BUF_POS, LLE_BUF_BITS, LLE_BUF_EVCOUNT, LLE_BUF_SRC_COLOUR, LLE_BUF_SRC_ENABLED) and the
 * lle_map_* queries, so liblle_hip.so keeps its kernels and its ABI version.  Link both (-llle_coop -llle_hip).
 *
 * The rule, for one environment in one state: for every ENABLED source l of colour c, let S_l be the agents that are the occupant
 * (Laser.agent()) of a laser tile of l in the sense of World.lasers (src/core/world.rs:159-172: the outer layer of a cell and the
 * one directly below it).  If c is in S_l, every other member b of S_l gives the edge c -> b (helper c, beneficiary b); otherwise
 * the source gives nothing.  Whether a tile's beam is on or off plays no part; a colour >= n_agents never blocks; an agent that
 * died entering a beam is no occupant (src/core/tiles/laser.rs:184-197).
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on `stream` with the batch's
 * device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_COOP_H
#define LLE_COOP_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_coop lle_coop;

/* Host only (no device needed): the cell table of `map`, out[i * width + j] = bit l set when source laser_id l owns a laser tile on
 * cell (i, j) in the sense of World.lasers -- what lle_map_laser_tiles enumerates, so on a cell crossed by three or more beams the
 * deeper sources are missing.  Writes up to `cap` words; returns height * width (or a negative status). */
int lle_coop_cell_masks(const lle_map* map, uint32_t* out, int cap);

/* Per map of `batch` (maps[m] = the map of block m, n_maps = lle_batch_n_maps(batch)): the cell table, per agent the mask of the
 * sources of its colour, the enabled mask and the start cells, built on the host and uploaded once; the five arrays below allocated
 * and zeroed (synchronises `stream`).  A map with a start cell on a laser cell also gets its START EDGES -- the edges of the state
 * right after World.reset, whose order effects (an agent can die at reset and re-light the beam, world.rs:411-432) are not restated
 * here: a temporary one-environment batch of the map is made through lle_batch_create, which is freshly reset, and this library's
 * own kernel runs on it.  The maps are read now; the handle keeps no pointer to them.  Free the handle before the batch.  Returns
 * NULL on failure -- no HIP device, more than 16 agents or 32 sources included -- and lle_coop_last_error says why. */
lle_coop* lle_coop_create(lle_batch* batch, const lle_map* const* maps, int n_maps, void* stream);
/* After lle_map_set_exits / lle_map_set_source + lle_batch_update_map / lle_batch_update_sources: colour masks, enabled mask and
 * start edges of map `map_index` are rebuilt and uploaded (synchronises `stream`).  LLE_ERR_ARG when `map` is not a recompilation of
 * the map it replaces (other dimensions, agents, sources, cell table or start cells). */
int lle_coop_update_map(lle_coop* c, int map_index, const lle_map* map, void* stream);
void lle_coop_free(lle_coop* c);

/* Operations, applied in this order to every selected environment. */
enum {
    LLE_COOP_FINISH = 1,      /* last_edges = episode_edges, last_profile = episode_profile with its valid byte set */
    LLE_COOP_CLEAR = 2,       /* episode_edges = 0, episode_profile = 0 */
    LLE_COOP_MARK_STARTS = 4, /* OR in the start edges of the environment's map (the state right after World.reset) */
    LLE_COOP_MARK_POS = 8     /* step_edges = the edges of the state in the batch's buffers now; OR them in */
};
enum {
    LLE_COOP_HONOUR_AUTO_RESET = 1, /* an environment whose LLE_BUF_EVCOUNT has bit 7 set (the step kernel reset it first) gets
                                       LLE_COOP_FINISH | LLE_COOP_CLEAR | LLE_COOP_MARK_STARTS ahead of the operations asked for.
                                       PRECONDITION, that of LLE_SHAPING_HONOUR_AUTO_RESET: only right after a step of the WHOLE
                                       batch with LLE_STEP_AUTO_RESET; after a step of a subset the others carry a stale bit. */
    LLE_COOP_ENV_SOURCES = 2        /* the batch keeps colours and flags per environment (after lle_batch_set_sources /
                                       lle_batch_reset_sources): read LLE_BUF_SRC_COLOUR / LLE_BUF_SRC_ENABLED instead of the
                                       map's own.  On a map with a start cell on a laser cell the start edges then depend on the
                                       environment's colours: LLE_COOP_MARK_STARTS and LLE_COOP_HONOUR_AUTO_RESET return
                                       LLE_ERR_ARG; such a host resets through env_mask and sends FINISH | CLEAR | MARK_POS on the
                                       reset state, which is always exact. */
};

typedef struct lle_coop_update_args {
    uint32_t struct_bytes;   /* sizeof(lle_coop_update_args) */
    uint32_t ops;            /* LLE_COOP_FINISH ... LLE_COOP_MARK_POS */
    uint32_t flags;          /* LLE_COOP_HONOUR_AUTO_RESET, LLE_COOP_ENV_SOURCES */
    uint32_t pad;
    const uint8_t* env_mask; /* device u8 [n]: environments to touch (byte != 0); NULL: all.  The others keep every array. */
} lle_coop_update_args;
/* ONE launch; allocates nothing, does not synchronise with the host and reads no environment variable: safe in a stream capture. */
int lle_coop_update(lle_coop* c, const lle_coop_update_args* args, void* stream);

/* Device pointers of the handle's arrays.
 *   u32 [n_envs][A], row h = bit mask of the beneficiaries of helper h (bits 0-15):
 *     LLE_COOP_STEP_EDGES     the edges of the state seen by the last LLE_COOP_MARK_POS (detect_dependencies)
 *     LLE_COOP_EPISODE_EDGES  their OR over the states of the running episode (flattened_edges)
 *     LLE_COOP_LAST_EDGES     LLE_COOP_EPISODE_EDGES of the most recently finished episode
 *   u8 [n_envs][8], the profile of the edge array beside it (8-byte aligned rows):
 *     LLE_COOP_EPISODE_PROFILE, LLE_COOP_LAST_PROFILE
 *     byte 0 flattened edges - 1 vertices (agents in any edge) - 2 max_distinct_helpers - 3 max_distinct_beneficiaries
 *     4 asymmetric edges (helper never helped, graph.py:147-151) - 5 marked states of the episode with at least one edge,
 *     saturating at 255 - 6 zero - 7 one once the row is valid (written by an update; for LAST: an episode has finished)
 * Every array starts on a 256-byte boundary and lies between two runs of at least LLE_COOP_GUARD_BYTES zero bytes of the same
 * allocation that no call writes (tests read them: a stray store of the kernel shows there). */
#define LLE_COOP_GUARD_BYTES 256
enum { LLE_COOP_STEP_EDGES = 0, LLE_COOP_EPISODE_EDGES, LLE_COOP_LAST_EDGES, LLE_COOP_EPISODE_PROFILE, LLE_COOP_LAST_PROFILE, LLE_COOP_BUF_COUNT };
void* lle_coop_buffer(lle_coop* c, int which);
/* The start edges of map `map_index` as the handle holds them: up to `cap` of its A words copied to `out` (host); returns A. */
int lle_coop_start_edges(const lle_coop* c, int map_index, uint32_t* out, int cap);

/* Message of the last failed call of this library on this thread. */
const char* lle_coop_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process (e.g. "coop_kernel<4,true>":
 * lanes per environment, cell table in LDS), NUL-terminated, truncated to `cap`; returns the bytes needed.
 * lle_coop_debug_compiled lists every instantiation the library holds, the same way. */
size_t lle_coop_debug_launched(char* buf, size_t cap);
size_t lle_coop_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_COOP_H */
