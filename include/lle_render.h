/*
 * lle_render.h -- C ABI of liblle_render.so: batched RGB frames of an lle_batch, the renderer of yamoling/lle
 * (src/rendering/renderer.rs, sprites.rs; World.get_image, src/bindings/world/pyworld.rs:518-524) for many environments of a
 * batch in one launch.
 *
 * A second library over the public ABI of include/lle_hip.h: it reads a batch only through lle_batch_get_buffer and the
 * lle_map_* queries, so liblle_hip.so keeps its kernels.  Link both (-llle_render -llle_hip).
 *
 * Frame: (32 H + 1, 32 W + 1, 3) values in HWC order per environment, the reference's layout and draw order -- static frame
 * (floor, walls, exits, voids), then every entry of World::lasers() with its recursion into the wrapped tiles, every
 * uncollected gem, every agent in id order, every laser source (opaque), the grid.  Alpha blending in float32, rounded op by op
 * (no FMA), truncated to u8 (renderer.rs:132-149).
 *
 * Threading and streams as in lle_hip.h: a renderer is NOT thread-safe; its device work is enqueued on `stream` with the
 * batch's device current, and the caller's current device is put back before a call returns.
 */
#ifndef LLE_RENDER_H
#define LLE_RENDER_H

#include <stddef.h>
#include <stdint.h>

#include "lle_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LLE_RENDER_TILE 32

typedef struct lle_renderer lle_renderer;

/* The sprites, host memory, 32 x 32 RGBA pixels each, rows first.  Each family is `n_*` numbered sprites followed by its
 * fallback (the reference's `k.png` ... and `n.png`; sprites.rs:94-148: ids beyond the numbered ones take the fallback).
 *   agents   [n_agents + 1][32][32][4]
 *   lasers   [n_lasers + 1][32][32][4]   horizontal; vertical = rotated 90 degrees clockwise (build.rs:106-126)
 *   sources  [n_sources + 1][32][32][4]  facing east; south / west / north = 1 / 2 / 3 clockwise rotations (build.rs:128-151);
 *                                        drawn opaque: their alpha is ignored (sprites.rs:70-88 load them as RGB)
 *   gem, void_  [32][32][4]
 * The library has no sprites of its own: the caller always passes them (the Python package draws a default set,
 * lle_amd/rendering.py SpriteAtlas.builtin(), or reads the reference's PNG files).  lle_render_create copies them. */
typedef struct lle_render_atlas {
    int32_t n_agents, n_lasers, n_sources;
    int32_t pad;
    const uint8_t* agents;
    const uint8_t* lasers;
    const uint8_t* sources;
    const uint8_t* gem;
    const uint8_t* void_;
} lle_render_atlas;

/* Static tiles and draw tables of every map of `batch` (maps[m] = the map of block m, n_maps = the batch's lle_batch_n_maps), built on
 * the host and uploaded once (synchronises `stream`).  The maps are read now; the renderer keeps no pointer to them.  Free the
 * renderer before the batch.  `atlas` must not be NULL.  Returns NULL on failure (lle_render_last_error says why). */
lle_renderer* lle_render_create(lle_batch* batch, const lle_map* const* maps, int n_maps, const lle_render_atlas* atlas, void* stream);
/* Rebuild the tables of map `map_index` after lle_map_set_exits or lle_map_set_source: the exits and the map's source colours are
 * drawn from them.  Synchronises `stream`.  LLE_ERR_ARG when `map` is not a recompilation of that map. */
int lle_render_update_map(lle_renderer* r, int map_index, const lle_map* map, void* stream);
void lle_render_free(lle_renderer* r);

enum { LLE_RENDER_U8 = 0, LLE_RENDER_F16 = 1, LLE_RENDER_BF16 = 2, LLE_RENDER_F32 = 3 };  /* element type of the frames */
enum {
    LLE_RENDER_ENV_SOURCES = 1  /* source colours from LLE_BUF_SRC_COLOUR (a batch after lle_batch_set_sources), not from the maps */
};

/* Shape and strides (in elements) of the output of lle_render_frame for n_sel environments: (n_sel, 32H+1, 32W+1, 3); each
 * environment's frame starts at a multiple of stride[0] elements (the frame's byte count rounded up to 128, for every dtype). */
typedef struct lle_render_desc {
    int32_t elem_bytes, ndim;
    int64_t shape[4];
    int64_t stride[4];
    int64_t bytes;  /* size of the output buffer */
} lle_render_desc;
int lle_render_desc_of(const lle_renderer* r, int64_t n_sel, int dtype, lle_render_desc* out);

/* Render the CURRENT state of n_sel environments into out_dev (device memory, 16-byte aligned, >= desc.bytes): environment
 * env_ids_dev[s] (device int64 [n_sel]; NULL = environments 0 .. n_sel-1) to slot s.  An id outside [0, n_envs) gives a frame
 * of zeros.  One launch, no allocation, no host synchronisation, no environment lookup: safe inside a stream capture. */
int lle_render_frame(lle_renderer* r, const int64_t* env_ids_dev, int64_t n_sel, uint32_t flags, int dtype, void* out_dev,
                     int64_t out_bytes, void* stream);

/* Message of the last failed call of this library on this thread. */
const char* lle_render_last_error(void);
/* Debug registry: newline-separated names of the kernels of this library launched by this process (the spelling of
 * lle_debug_launched, e.g. "render_kernel<0>"), NUL-terminated, truncated to `cap`; returns the bytes needed. */
size_t lle_render_debug_launched(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LLE_RENDER_H */
