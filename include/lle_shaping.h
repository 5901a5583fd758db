/*
 * lle_shaping.h -- C ABI of liblle_shaping.so: potential-based reward shaping (PotentialShapedLLE,
 * python/lle/env/reward_strategy.py:112-181) and the LaserSubgoal extras (python/lle/env/extras_generators.py:75-101) of
 * yamoling/lle for every environment of an lle_batch, in one launch per step.
 *
 * A third library over the public ABI of include/lle_hip.h, like liblle_render.so: it reads a batch only through
 * lle_batch_get_buffer (LLE_BUF_POS, LLE_BUF_EVCOUNT) and the lle_map_* queries, so liblle_hip.so keeps its kernels and its
 * ABI version.  Link both (-llle_shaping -llle_hip).
 *
 * Both reference classes keep, per agent and per listed laser source, "has this agent stood on a tile of that source's beam
 * since the last reset" (reward_strategy.py:170-175, extras_generators.py:93-98).  Here that is one 32-bit word per
 * (environment, agent) with bit l = source laser_id l reached, kept twice -- once for the reward strategy, once for the extras
 * generator: the reference holds them in two objects that are cleared and marked at different moments around LLE.set_state
 * (python/lle/env/env.py:208-217).  A beam tile counts whether the beam is on or off and whatever its colour
 * (get_lasers_of, python/lle/env/utils.py:6-11, filters World.lasers by laser_id only), so the cell table is static per map.
 *
 * Threading and streams as in lle_hip.h: a handle is NOT thread-safe; its device work is enqueued on `stream` with the batch's
 * device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_SHAPING_H
#define LLE_SHAPING_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LLE_SHAPING_MAX_COLS 64    /* entries of pbrs_cols, and of extras_cols */
#define LLE_SHAPING_MAX_REPEATS 8  /* times one laser_id may be listed in pbrs_cols */

typedef struct lle_shaping lle_shaping;

/* The selections, fixed at create (host memory, copied):
 *   pbrs_cols    the laser_ids PotentialShapedLLE rewards, in the caller's order (`lasers_to_reward`, reward_strategy.py:132,
 *                163-168).  The reference iterates a LIST: a source listed twice counts twice in the potential, and so it does here.
 *                n_pbrs_cols == 0: nothing to reward (a map without sources, an empty list): the potential of the empty array is 0
 *                and reward_out gets the shaped term 0 -- base[0] + 0 or [base, 0].
 *   extras_cols  the concatenation of the source lists of every LaserSubgoal of the extras generator (MultiGenerator.compute
 *                concatenates along the last axis, extras_generators.py:63-67); column e of the extras is laser_id extras_cols[e].
 *   gamma, reward_value   reward_strategy.py:121-122, as doubles (Python floats). */
typedef struct lle_shaping_config {
    uint32_t struct_bytes;  /* sizeof(lle_shaping_config): lets the struct grow */
    int32_t n_pbrs_cols;
    const int32_t* pbrs_cols;
    int32_t n_extras_cols;
    int32_t pad;
    const int32_t* extras_cols;
    double gamma;
    double reward_value;
} lle_shaping_config;

/* Host only (no device needed): the cell table of `map`, out[i * width + j] = bit l set when source laser_id l OWNS a laser tile
 * on cell (i, j) in the sense of World.lasers (src/core/world.rs:159-172): only the outer laser layer of a cell and the one
 * directly below it are listed, so on a cell crossed by three or more beams the deeper sources do not count -- what
 * lle_map_laser_tiles enumerates.  Writes up to `cap` words; returns height * width (or a negative status). */
int lle_shaping_cell_masks(const lle_map* map, uint32_t* out, int cap);

/* Cell tables and start cells of every map of `batch` (maps[m] = the map of block m, n_maps = lle_batch_n_maps(batch)) built on the
 * host and uploaded once, and the two reached arrays u32 [n_envs][A] allocated and zeroed (synchronises `stream`).  The maps are
 * read now; the handle keeps no pointer to them.  Free the handle before the batch.  The arrays start CLEARED: run
 * lle_shaping_update with LLE_SHAPING_CLEAR | LLE_SHAPING_MARK_STARTS on both before the first step (what LLE.reset does,
 * env.py:191-203).  Returns NULL on failure -- no HIP device included -- and lle_shaping_last_error says why. */
lle_shaping* lle_shaping_create(lle_batch* batch, const lle_map* const* maps, int n_maps, const lle_shaping_config* config, void* stream);
/* After lle_map_set_exits / lle_map_set_source + lle_batch_update_map: the tables depend on neither exits nor colours, so nothing
 * is uploaded; the call only validates that `map` still is a recompilation of map `map_index` (same dimensions, agents, sources,
 * cell table and start cells) and returns LLE_ERR_ARG otherwise. */
int lle_shaping_update_map(lle_shaping* s, int map_index, const lle_map* map, void* stream);
void lle_shaping_free(lle_shaping* s);

/* Operations on one reached array, applied in this order to every selected environment. */
enum {
    LLE_SHAPING_CLEAR = 1,       /* _agents_pos_reached.fill(False)        (reward_strategy.py:180, extras_generators.py:100-101) */
    LLE_SHAPING_MARK_STARTS = 2, /* mark agent a at start cell a of the env's map: compute_potential / compute right after World.reset */
    LLE_SHAPING_MARK_POS = 4     /* mark agent a at its current LLE_BUF_POS, dead or alive (reward_strategy.py:170-174; an agent that
                                    just died on a beam has reached it, python/tests/test_observations.py:463-469) */
};
enum {
    LLE_SHAPING_HONOUR_AUTO_RESET = 1 /* an environment whose LLE_BUF_EVCOUNT has bit 7 set (the step kernel reset it first,
                                         LLE_STEP_AUTO_RESET) gets LLE_SHAPING_CLEAR | LLE_SHAPING_MARK_STARTS on BOTH arrays ahead of the
                                         operations asked for: LLE.reset between two episodes (env.py:191-203).
                                         PRECONDITION: the bit is the one the LAST step launch left, and a step rewrites it only for the
                                         environments it served.  Pass the flag only right after a step of the WHOLE batch with
                                         LLE_STEP_AUTO_RESET (lle_batch_step / _step_outputs); after a step of a sub-range or of a masked
                                         subset the other environments carry a stale bit and would be reset here a second time -- such a
                                         host resets through env_mask instead. */
};

/* One update.  Every pointer is device memory or NULL (= not wanted).
 *   env_mask     u8  [n]        environments to touch (byte != 0); NULL: all.  An unselected environment keeps its arrays and
 *                               gets none of the outputs written.
 *   base_reward  f32 [n][1|4]   the wrapped strategy's reward (lle_env_outputs.reward with the same reward_kind); required with reward_out
 *   reward_out   f32 [n][1|5]   PotentialShapedLLE.compute_reward (reward_strategy.py:148-160).  With `prev` the potential of the strategy
 *                               array after LLE_SHAPING_CLEAR / _MARK_STARTS (and the auto-reset) and before LLE_SHAPING_MARK_POS, `cur` the
 *                               one after it, potential = double(entries not reached) * reward_value (reward_strategy.py:175):
 *                                   p = gamma * prev - cur                 in double, the product rounded before the subtraction
 *                               reward_kind 0: out[0] = base[0] + float(p), added in float32 (numpy's `reward[0] += p`)
 *                               reward_kind 1: out[0..3] = base[0..3], out[4] = float(p)  (the reference's np.concat gives float64 there)
 *                               No previous potential is stored: it is a function of the bits.
 *   extras_out   f32 [n][A][E]  LaserSubgoal.compute (extras_generators.py:93-98): 1.0 / 0.0 from the extras array after its operations */
typedef struct lle_shaping_update_args {
    uint32_t struct_bytes;  /* sizeof(lle_shaping_update_args) */
    uint32_t strategy_ops;  /* LLE_SHAPING_* on the reward strategy's array */
    uint32_t extras_ops;    /* LLE_SHAPING_* on the extras generator's array */
    uint32_t flags;         /* LLE_SHAPING_HONOUR_AUTO_RESET */
    int32_t reward_kind;    /* 0: SingleObjective underneath, 1: MultiObjective */
    int32_t pad;
    const uint8_t* env_mask;
    const float* base_reward;
    float* reward_out;
    float* extras_out;
} lle_shaping_update_args;
/* ONE launch; allocates nothing and does not synchronise with the host: safe inside a stream capture. */
int lle_shaping_update(lle_shaping* s, const lle_shaping_update_args* args, void* stream);

/* Device pointers of the two arrays, u32 [n_envs][A] (element strides A, 1): which 0 = reward strategy, 1 = extras generator. */
void* lle_shaping_reached(lle_shaping* s, int which);

/* Message of the last failed call of this library on this thread. */
const char* lle_shaping_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process (the spelling of
 * lle_debug_launched, e.g. "shaping_kernel<4,true>": lanes per environment, cell table in LDS), NUL-terminated, truncated to
 * `cap`; returns the bytes needed.  lle_shaping_debug_compiled lists every instantiation the library holds, the same way. */
size_t lle_shaping_debug_launched(char* buf, size_t cap);
size_t lle_shaping_debug_compiled(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_SHAPING_H */
