/*
 * lle_cooptrails.h -- C ABI of liblle_cooptrails.so: how deep the cooperation of every environment's episode is, in one launch
 * behind the launch of liblle_coop.so.
 *
 * The TEMPORAL half of the reference's PlanProfile (python/lle/characterization/plan/profile.py: is_sequential(length) = "a trail of
 * `length` help edges in time order exists") for a whole batch.  The flattened edges of lle_coop.h do not decide it.  One small vector
 * per environment does: L[a] = the length of the longest trail of help edges that ends at agent a (chained, times non-decreasing, no
 * temporal edge twice), updated once per state of the episode by
 *     L'[y] = max(L[y], max over x and over trails P inside this state's edges from x to y of L[x] + |P|)
 * (DESIGN.md sections 4.13 and 4.15).
 *
 * A library of its own over the public ABI of lle_hip.h and lle_coop.h: it reads the batch through lle_batch_get_buffer
 * (LLE_BUF_EVCOUNT, LLE_BUF_ERR) and the coop handle through lle_coop_buffer (LLE_COOP_STEP_EDGES) and lle_coop_start_edges, so
 * liblle_hip.so and liblle_coop.so keep their kernels and ABI.  Link all three (-llle_cooptrails -llle_coop -llle_hip).
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on `stream` with the batch's
 * device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_COOPTRAILS_H
#define LLE_COOPTRAILS_H

#include <stddef.h>
#include <stdint.h>

#include "lle_coop.h"
#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lle_cooptrails lle_cooptrails;

#define LLE_COOPTRAILS_SATURATED 15     /* a length of 15 means 15 or more: no trail is extended past it */
#define LLE_COOPTRAILS_WALK_BUDGET 4096 /* arc extensions one walk (one state, one starting agent) may make before it gives up */

/* The four arrays allocated and zeroed, the start edges of every map copied from `coop` (lle_coop_start_edges) and uploaded
 * (synchronises `stream`).  The handle keeps the device pointers of LLE_BUF_EVCOUNT and LLE_BUF_ERR of `batch` and of
 * LLE_COOP_STEP_EDGES of `coop`: free it before either.  NULL on failure -- no HIP device included -- and
 * lle_cooptrails_last_error says why. */
lle_cooptrails* lle_cooptrails_create(lle_batch* batch, lle_coop* coop, void* stream);
/* After lle_coop_update_map(coop, map_index, ...): the start edges of that map are read again from `coop` and uploaded
 * (synchronises `stream`). */
int lle_cooptrails_update_map(lle_cooptrails* t, int map_index, void* stream);
void lle_cooptrails_free(lle_cooptrails* t);

/* Operations: those of lle_coop.h, the same values, applied in this order to every selected environment. */
enum {
    LLE_COOPTRAILS_FINISH = 1,      /* last_trails = episode_trails, last_tprofile = episode_tprofile with its valid byte set */
    LLE_COOPTRAILS_CLEAR = 2,       /* episode_trails = 0, episode_tprofile = 0 (the dense mark too) */
    LLE_COOPTRAILS_MARK_STARTS = 4, /* one layer update with the start edges of the environment's map */
    LLE_COOPTRAILS_MARK_POS = 8     /* one layer update with the environment's rows of LLE_COOP_STEP_EDGES */
};
enum {
    LLE_COOPTRAILS_HONOUR_AUTO_RESET = 1, /* LLE_COOP_HONOUR_AUTO_RESET, same meaning and precondition: an environment whose
                                             LLE_BUF_EVCOUNT has bit 7 set gets FINISH | CLEAR | MARK_STARTS ahead of the operations
                                             asked for -- and so up to two layer updates in one launch. */
    LLE_COOPTRAILS_SKIP_REFUSED = 2       /* an environment whose LLE_BUF_ERR is non-zero gets no MARK_POS layer: a refused step made
                                             no new state.  Its other operations still apply, and its rows are written as for any
                                             touched environment.  A refusal CAN coincide with bit 7: the step kernel resets a
                                             finished environment first and then applies the actions to the reset state, which may
                                             refuse them; bit 7 is stored all the same.  Such an environment finishes its episode and
                                             starts the next one at the start edges, without a further layer. */
};

typedef struct lle_cooptrails_update_args {
    uint32_t struct_bytes;   /* sizeof(lle_cooptrails_update_args) */
    uint32_t ops;            /* LLE_COOPTRAILS_FINISH ... LLE_COOPTRAILS_MARK_POS */
    uint32_t flags;          /* LLE_COOPTRAILS_HONOUR_AUTO_RESET, LLE_COOPTRAILS_SKIP_REFUSED */
    uint32_t pad;
    const uint8_t* env_mask; /* device u8 [n]: environments to touch (byte != 0); NULL: all.  The others keep every array. */
} lle_cooptrails_update_args;
/* PRECONDITION: the call follows, on the same stream, the lle_coop_update whose ops, HONOUR_AUTO_RESET flag and env_mask it repeats
 * (LLE_COOP_STEP_EDGES then holds the edges of the state MARK_POS means).
 * ONE launch; allocates nothing, does not synchronise with the host and reads no environment variable: safe in a stream capture. */
int lle_cooptrails_update(lle_cooptrails* t, const lle_cooptrails_update_args* args, void* stream);

/* Device pointers of the handle's arrays.
 *   u64 [n_envs]: 4 bits per agent, agent a in bits 4 a .. 4 a + 3 = min(L[a], 15)
 *     LLE_COOPTRAILS_EPISODE_TRAILS  of the running episode
 *     LLE_COOPTRAILS_LAST_TRAILS     of the most recently finished episode
 *   u8 [n_envs][4], the profile of the value beside it:
 *     LLE_COOPTRAILS_EPISODE_TPROFILE, LLE_COOPTRAILS_LAST_TPROFILE
 *     byte 0 the longest trail (the greatest field) - 1 states of the episode whose layer had an edge and entered the walk, saturating
 *     at 255 - 2 one once a walk of the episode ran out of LLE_COOPTRAILS_WALK_BUDGET (the fields are lower bounds then; sticky until
 *     CLEAR) - 3 one once the row is valid (written by an update; for LAST: an episode has finished)
 * Every array starts on a 256-byte boundary and lies between two runs of at least LLE_COOP_GUARD_BYTES zero bytes of the same
 * allocation that no call writes. */
enum { LLE_COOPTRAILS_EPISODE_TRAILS = 0, LLE_COOPTRAILS_LAST_TRAILS, LLE_COOPTRAILS_EPISODE_TPROFILE, LLE_COOPTRAILS_LAST_TPROFILE, LLE_COOPTRAILS_BUF_COUNT };
void* lle_cooptrails_buffer(lle_cooptrails* t, int which);

/* Message of the last failed call of this library on this thread. */
const char* lle_cooptrails_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process (e.g. "cooptrails_kernel<8>": lanes
 * per environment), NUL-terminated, truncated to `cap`; returns the bytes needed.  lle_cooptrails_debug_compiled lists every
 * instantiation the library holds, the same way. */
size_t lle_cooptrails_debug_launched(char* buf, size_t cap);
size_t lle_cooptrails_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_COOPTRAILS_H */
