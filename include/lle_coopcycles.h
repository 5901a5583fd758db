/*
 * lle_coopcycles.h -- C ABI of liblle_coopcycles.so: which closed trails of help the episode of every environment holds, in one launch
 * behind the launches of liblle_coop.so and liblle_cooptrails.so.
 *
 * The reference's headline property (python/lle/characterization/plan/profile.py: is_interdependent(n_agents) = "some closed trail of
 * help edges in time order visits exactly n_agents distinct agents") for a whole batch.  Neither the flattened edges of lle_coop.h nor
 * the trail lengths of lle_cooptrails.h decide it for n_agents >= 3.  The set R of (anchor, current, support) triples of the episode
 * does -- some trail leads from `anchor` to `current` and visits exactly the agents of `support` -- and one more state with arcs
 * extends it by the layer_update of lle_amd/cycles/cycles_logic.hpp, the very function the closed-trail SEARCH (lle_cycles.h) runs
 * per record, here with an order that never prunes and never closes (DESIGN.md sections 4.16 and 4.18).
 *
 * A library of its own over the public ABI of lle_hip.h and lle_coop.h: it reads the batch through lle_batch_get_buffer
 * (LLE_BUF_EVCOUNT, LLE_BUF_ERR) and the coop handle through lle_coop_buffer (LLE_COOP_STEP_EDGES) and lle_coop_start_edges, so
 * the other libraries keep their kernels and ABI.  Link all three (-llle_coopcycles -llle_coop -llle_hip).
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on `stream` with the batch's
 * device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_COOPCYCLES_H
#define LLE_COOPCYCLES_H

#include <stddef.h>
#include <stdint.h>

#include "lle_coop.h"
#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_coopcycles lle_coopcycles;

#define LLE_COOPCYCLES_MAX_AGENTS 6     /* a packed set of agent masks is one 64-bit word: maps of more agents are refused */
#define LLE_COOPCYCLES_SMALL_WORDS 3    /* words of a value of a map of up to 4 agents */
#define LLE_COOPCYCLES_LARGE_WORDS 21   /* ... of 5 or 6 agents */
#define LLE_COOPCYCLES_WALK_BUDGET 4096 /* arc extensions the walk of one layer (one state of one environment) may make before it gives up */

/* The four arrays allocated and zeroed, the start edges of every map copied from `coop` (lle_coop_start_edges) and uploaded
 * (synchronises `stream`).  The handle keeps the device pointers of LLE_BUF_EVCOUNT and LLE_BUF_ERR of `batch` and of
 * LLE_COOP_STEP_EDGES of `coop`: free it before either.  NULL on failure -- no HIP device included -- and
 * lle_coopcycles_last_error says why; a map of more than LLE_COOPCYCLES_MAX_AGENTS agents is LLE_ERR_UNSUPPORTED. */
lle_coopcycles* lle_coopcycles_create(lle_batch* batch, lle_coop* coop, void* stream);
/* After lle_coop_update_map(coop, map_index, ...): the start edges of that map are read again from `coop` and uploaded
 * (synchronises `stream`). */
int lle_coopcycles_update_map(lle_coopcycles* t, int map_index, void* stream);
void lle_coopcycles_free(lle_coopcycles* t);

/* Operations: those of lle_coop.h and lle_cooptrails.h, the same values, applied in this order to every selected environment. */
enum {
    LLE_COOPCYCLES_FINISH = 1,      /* last_closed = episode_closed, last_cprofile = episode_cprofile with its valid byte set */
    LLE_COOPCYCLES_CLEAR = 2,       /* episode_closed = 0, episode_cprofile = 0 (the dense mark too) */
    LLE_COOPCYCLES_MARK_STARTS = 4, /* one layer update with the start edges of the environment's map */
    LLE_COOPCYCLES_MARK_POS = 8     /* one layer update with the environment's rows of LLE_COOP_STEP_EDGES */
};
enum {
    LLE_COOPCYCLES_HONOUR_AUTO_RESET = 1, /* LLE_COOP_HONOUR_AUTO_RESET, same meaning and precondition: an environment whose
                                             LLE_BUF_EVCOUNT has bit 7 set gets FINISH | CLEAR | MARK_STARTS ahead of the operations
                                             asked for -- and so more than one layer update in one launch. */
    LLE_COOPCYCLES_SKIP_REFUSED = 2       /* LLE_COOPTRAILS_SKIP_REFUSED: an environment whose LLE_BUF_ERR is non-zero gets no MARK_POS
                                             layer, a refused step made no new state.  Its other operations still apply. */
};

typedef struct lle_coopcycles_update_args {
    uint32_t struct_bytes;   /* sizeof(lle_coopcycles_update_args) */
    uint32_t ops;            /* LLE_COOPCYCLES_FINISH ... LLE_COOPCYCLES_MARK_POS */
    uint32_t flags;          /* LLE_COOPCYCLES_HONOUR_AUTO_RESET, LLE_COOPCYCLES_SKIP_REFUSED */
    uint32_t pad;
    const uint8_t* env_mask; /* device u8 [n]: environments to touch (byte != 0); NULL: all.  The others keep every array. */
} lle_coopcycles_update_args;
/* PRECONDITION: the call follows, on the same stream, the lle_coop_update whose ops, HONOUR_AUTO_RESET flag and env_mask it repeats
 * (LLE_COOP_STEP_EDGES then holds the edges of the state MARK_POS means).
 * ONE launch; allocates nothing, does not synchronise with the host and reads no environment variable: safe in a stream capture.
 * A layer whose walk runs out of LLE_COOPCYCLES_WALK_BUDGET is dropped WHOLE: the value stays as it was and the dense byte is set
 * (sticky until CLEAR, copied by FINISH).  Dropping a layer only loses trails: under dense every order reported is still true and only
 * the absences are uncertain. */
int lle_coopcycles_update(lle_coopcycles* t, const lle_coopcycles_update_args* args, void* stream);

/* Device pointers of the handle's arrays.
 *   u32 [W][n_envs], W = LLE_COOPCYCLES_SMALL_WORDS for maps of up to 4 agents, else LLE_COOPCYCLES_LARGE_WORDS: the packed triples of
 *   lle_cycles.h (THE VALUE), word-major -- word i of environment e at [i * n_envs + e]
 *     LLE_COOPCYCLES_EPISODE_CLOSED  of the running episode
 *     LLE_COOPCYCLES_LAST_CLOSED     of the most recently finished episode
 *   u8 [n_envs][4], the profile of the value beside it:
 *     LLE_COOPCYCLES_EPISODE_CPROFILE, LLE_COOPCYCLES_LAST_CPROFILE
 *     byte 0 the closed orders as a bit set: bit k (2 <= k <= 6) = some closed trail visits exactly k agents - 1 states of the episode
 *     whose layer had an arc and entered the walk, saturating at 255 - 2 one once a layer of the episode was dropped (sticky until
 *     CLEAR) - 3 one once the row is valid (written by an update; for LAST: an episode has finished)
 * Every array starts on a 256-byte boundary and lies between two runs of at least LLE_COOP_GUARD_BYTES zero bytes of the same
 * allocation that no call writes. */
enum { LLE_COOPCYCLES_EPISODE_CLOSED = 0, LLE_COOPCYCLES_LAST_CLOSED, LLE_COOPCYCLES_EPISODE_CPROFILE, LLE_COOPCYCLES_LAST_CPROFILE, LLE_COOPCYCLES_BUF_COUNT };
void* lle_coopcycles_buffer(lle_coopcycles* t, int which);

/* Message of the last failed call of this library on this thread. */
const char* lle_coopcycles_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process (e.g. "coopcycles_kernel<21>": words
 * per value), NUL-terminated, truncated to `cap`; returns the bytes needed.  lle_coopcycles_debug_compiled lists every
 * instantiation the library holds, the same way. */
size_t lle_coopcycles_debug_launched(char* buf, size_t cap);
size_t lle_coopcycles_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_COOPCYCLES_H */
