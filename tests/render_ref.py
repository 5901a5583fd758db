"""A numpy restatement of the reference renderer, for the tests: src/rendering/renderer.rs, mod.rs, sprites.rs and build.rs:8-150
of yamoling/lle, written down rule by rule (each cites its line) and evaluated the way the reference does -- a static frame, then
the draw calls in order on a full-size image -- NOT the way the kernel does (per pixel from resolved per-cell lists).  The GPU
frames of liblle_render.so must equal this byte for byte.

`render(scene, state, atlas)`:
  scene  a `Scene` of a Map: the static description the reference's World holds (walls, exits, voids, gems, sources, the laser
         stack of every cell -- Laser::wrapped, through lle_map_cell_layers)
  state  a `State`: agents' positions, the gem bits (LLE_BUF_GEMS), the beam words (LLE_BUF_BEAMS) and the colour of every beam
         word (LLE_BUF_SRC_COLOUR, or the map's colours)
  atlas  a lle_amd.rendering.SpriteAtlas
"""
from dataclasses import dataclass

import numpy as np

TILE_SIZE = 32                      # mod.rs:8
BACKGROUND_GREY = (218, 218, 218)   # mod.rs:9
GRID_GREY = (127, 127, 127)         # mod.rs:10
BLACK = (0, 0, 0)                   # mod.rs:11
NORTH, EAST, SOUTH, WEST = 0, 1, 2, 3


def rotate90(img):
    """image::imageops::rotate90 (build.rs:84-93): clockwise, dst[x][h - 1 - y] = src[y][x]."""
    h, w = img.shape[:2]
    out = np.empty((w, h) + img.shape[2:], dtype=img.dtype)
    for y in range(h):
        out[:, h - 1 - y] = img[y]
    return out


def blend(bg, fg):
    """add_transparent_image's arithmetic (renderer.rs:139-148): alpha = a as f32 / 255.0; ((1.0 - alpha) * bg as f32 + alpha *
    fg as f32) as u8 -- every operation rounded to f32 on its own (Rust does not contract into an FMA), `as u8` truncates
    (saturating).  bg: uint8 [..., 3]; fg: uint8 [..., 4]."""
    alpha = fg[..., 3:4].astype(np.float32) / np.float32(255.0)
    one_minus = np.float32(1.0) - alpha
    v = one_minus * bg.astype(np.float32) + alpha * fg[..., :3].astype(np.float32)
    return np.clip(np.floor(v), 0, 255).astype(np.uint8)


def add_transparent_image(frame, sprite, x, y):
    """renderer.rs:132-149."""
    frame[y:y + TILE_SIZE, x:x + TILE_SIZE] = blend(frame[y:y + TILE_SIZE, x:x + TILE_SIZE], sprite)


def draw_rectangle(img, x, y, width, height, colour, thickness):
    """renderer.rs:151-168: four opaque bars."""
    img[y:y + thickness, x:x + width] = colour
    img[y + height - thickness:y + height, x:x + width] = colour
    img[y:y + height, x:x + thickness] = colour
    img[y:y + height, x + width - thickness:x + width] = colour


# ---- sprite selection (sprites.rs:93-148; build.rs:63-150)
def agent_sprite(atlas, agent_id):
    """agent_id <= MAX_NUMBERED_AGENT_SPRITE_ID ? AGENTS[agent_id] : AGENT_FALLBACK (sprites.rs:111-118)."""
    return atlas.agents[agent_id] if agent_id <= atlas.n_agents - 1 else atlas.agents[-1]


def laser_sprite(atlas, colour, direction):
    """draw_laser (renderer.rs:190-193): North / South -> vertical_laser, East / West -> horizontal_laser; `.get(id)` or the
    fallback (sprites.rs:93-128); vertical = the horizontal sprite rotated once (build.rs:106-126)."""
    sprite = atlas.lasers[colour] if colour < atlas.n_lasers else atlas.lasers[-1]
    return rotate90(sprite) if direction in (NORTH, SOUTH) else sprite


def source_sprite(atlas, colour, direction):
    """draw_laser_source (renderer.rs:200-209): east as stored, south / west / north 1 / 2 / 3 rotations (build.rs:128-151), loaded
    as RGB (sprites.rs:70-88: the alpha channel is dropped)."""
    sprite = atlas.sources[colour] if colour < atlas.n_sources else atlas.sources[-1]
    for _ in range({EAST: 0, SOUTH: 1, WEST: 2, NORTH: 3}[direction]):
        sprite = rotate90(sprite)
    return sprite[..., :3]


@dataclass
class Scene:
    height: int
    width: int
    walls: list
    exits: list
    voids: list
    gems: list          # positions in gem-index order
    sources: list       # (i, j, direction, map colour, first beam word) in laser_id order
    stacks: dict        # (i, j) -> [(laser_id, direction, word, bit), ...] outermost first (Laser::wrapped)

    @staticmethod
    def of(m):
        """From an lle_amd._capi.Map."""
        from lle_amd._capi import LLE_POS_EXIT, LLE_POS_GEM, LLE_POS_VOID, LLE_POS_WALL
        stacks = {}
        for c in m.cell_layers():
            stacks.setdefault((c.i, c.j), []).append((c.depth, (int(c.laser_id), int(c.direction), int(c.word), int(c.bit))))
        stacks = {k: [e for _, e in sorted(v)] for k, v in stacks.items()}
        words = m.source_first_words()
        sources = [(int(s.i), int(s.j), int(s.direction), int(s.agent_id), words[k]) for k, s in enumerate(m.sources())]
        return Scene(m.height, m.width, m.positions(LLE_POS_WALL), m.positions(LLE_POS_EXIT), m.positions(LLE_POS_VOID),
                     m.positions(LLE_POS_GEM), sources, stacks)


@dataclass
class State:
    positions: list     # (i, j) per agent
    gem_bits: int       # bit g = gem g collected
    beam_words: list    # LLE_BUF_BEAMS of the env
    colours: list       # colour of every beam word (None: the map's)


def static_frame(scene, atlas):
    """Renderer::static_rendering (renderer.rs:39-73)."""
    frame = np.empty((TILE_SIZE * scene.height + 1, TILE_SIZE * scene.width + 1, 3), dtype=np.uint8)
    frame[:] = BACKGROUND_GREY                                   # :41
    for i, j in scene.walls:                                     # :43-49, sprites.rs:90-91 (an opaque black tile)
        frame[TILE_SIZE * i:TILE_SIZE * (i + 1), TILE_SIZE * j:TILE_SIZE * (j + 1)] = BLACK
    for i, j in scene.exits:                                     # :52-64
        draw_rectangle(frame, TILE_SIZE * j + 1, TILE_SIZE * i + 1, TILE_SIZE - 1, TILE_SIZE - 1, BLACK, 2)
    for i, j in scene.voids:                                     # :67-72
        add_transparent_image(frame, atlas.void, TILE_SIZE * j, TILE_SIZE * i)
    return frame


def render(scene, state, atlas):
    """Renderer::update (renderer.rs:75-108)."""
    frame = static_frame(scene, atlas)
    gem_at = {p: g for g, p in enumerate(scene.gems)}

    def colour_of(word, laser_id):
        return scene.sources[laser_id][3] if state.colours is None else int(state.colours[word])

    def draw_gem(g, x, y):                                       # renderer.rs:181-185
        if not (state.gem_bits >> g) & 1:
            add_transparent_image(frame, atlas.gem, x, y)

    def draw_laser(stack, depth, pos, x, y):                     # renderer.rs:187-198
        laser_id, direction, word, bit = stack[depth]
        if (int(state.beam_words[word]) >> bit) & 1:             # laser.is_on()
            add_transparent_image(frame, laser_sprite(atlas, colour_of(word, laser_id), direction), x, y)
        if depth + 1 < len(stack):                               # draw_tile(laser.wrapped()) (renderer.rs:172-179)
            draw_laser(stack, depth + 1, pos, x, y)
        elif pos in gem_at:
            draw_gem(gem_at[pos], x, y)

    for pos, stack in sorted(scene.stacks.items()):              # World::lasers() (world.rs:159-172): the outer layer and,
        x, y = TILE_SIZE * pos[1], TILE_SIZE * pos[0]             # when nested, the second one as an entry of its own
        for entry in range(min(2, len(stack))):
            draw_laser(stack, entry, pos, x, y)
    for g, (i, j) in enumerate(scene.gems):                      # renderer.rs:85-92
        draw_gem(g, TILE_SIZE * j, TILE_SIZE * i)
    for a, (i, j) in enumerate(state.positions):                 # renderer.rs:93-97: every agent, dead or arrived
        add_transparent_image(frame, agent_sprite(atlas, a), TILE_SIZE * j, TILE_SIZE * i)
    for laser_id, (i, j, direction, _colour, first_word) in enumerate(scene.sources):  # renderer.rs:98-105, copy_from: opaque
        sprite = source_sprite(atlas, colour_of(first_word, laser_id), direction)
        frame[TILE_SIZE * i:TILE_SIZE * (i + 1), TILE_SIZE * j:TILE_SIZE * (j + 1)] = sprite
    frame[::TILE_SIZE, :] = GRID_GREY                            # draw_grid (renderer.rs:119-130)
    frame[:, ::TILE_SIZE] = GRID_GREY
    return frame


def states_of(bw, env_sources=False):
    """The State of every env of a BatchedWorld, from its device buffers (synchronises)."""
    import torch
    torch.cuda.synchronize(bw.device)
    pos = bw.pos.cpu().numpy()
    gems = bw.gems.cpu().numpy().view(np.uint32)
    beams = bw.beams.cpu().numpy().view(np.uint32)
    colours = bw.src_colour.cpu().numpy() if env_sources else None
    return [State([(int(p[0]), int(p[1])) for p in pos[e]], int(gems[e]), list(beams[e]), None if colours is None else list(colours[e]))
            for e in range(bw.n_envs)]


# ---- synthetic states: the domain of the render kernel beyond what rollouts reach (tests/test_gpu_render_states.py)
def cell_tags(scene):
    """(i, j) -> the set of classes a cell belongs to, for the coverage assertions: its static tile ("floor", "wall", "exit",
    "void"; a source's cell is "source"), "gem", and "beamK" for a stack of K laser layers.  "floor" means a bare floor cell."""
    tags = {(i, j): {"floor"} for i in range(scene.height) for j in range(scene.width)}
    for name, cells in (("wall", scene.walls), ("exit", scene.exits), ("void", scene.voids)):
        for c in cells:
            tags[tuple(c)] = {name}
    for s in scene.sources:
        tags[(s[0], s[1])] = {"source"}
    for c in scene.gems:
        tags[tuple(c)].add("gem")
    for c, stack in scene.stacks.items():
        tags[tuple(c)].add(f"beam{len(stack)}")
    for c, t in tags.items():
        if "floor" in t and len(t) > 1:
            t.discard("floor")
    return tags


def random_states(scenes, n_envs, n_agents, n_words, seed, planted=()):
    """Seeded states over the whole domain the kernel reads, as numpy arrays for `write_states`: pos u8 [n, A, 2], gems u32 [n],
    beams u32 [n, Lw], colours u8 [n, Lw].  scenes: the Scene of every block of envs (len(scenes) divides n_envs).
      gems    any subset (random 32-bit words masked to the map's gems); env 0 none, env 1 all, env 2 the highest index alone
      beams   arbitrary words, not only prefixes; env 0 all off, env 1 all on, envs 2 .. 33 bit (e - 2) of EVERY word alone,
              then single bits of single words and random words
      pos     any cell that is not a laser source: the class of the cell (cell_tags) is drawn first so that rare classes are hit,
              then a cell of it; an agent joins an earlier agent's cell with probability 1/4; env 3: all agents on one cell
      colours any byte; 0, the values around 12 and 255 are frequent
    `planted`: (env, agent, (i, j)) positions put in afterwards.  `classes_hit` says which classes of cells the agents stand on."""
    rng = np.random.default_rng(seed)
    per = n_envs // len(scenes)
    pos = np.zeros((n_envs, n_agents, 2), np.uint8)
    gems = rng.integers(0, 1 << 32, n_envs, dtype=np.uint64).astype(np.uint32)
    beams = rng.integers(0, 1 << 32, (n_envs, max(n_words, 1)), dtype=np.uint64).astype(np.uint32)
    palette = np.array([0, 1, 2, 3, 4, 5, 11, 12, 13, 14, 200, 254, 255], np.uint8)
    colours = np.where(rng.random((n_envs, max(n_words, 1))) < 0.5, palette[rng.integers(0, len(palette), (n_envs, max(n_words, 1)))],
                       rng.integers(0, 256, (n_envs, max(n_words, 1)), dtype=np.uint8)).astype(np.uint8)
    for e in range(n_envs):
        scene = scenes[e // per]
        G = len(scene.gems)
        full = np.uint32((1 << G) - 1)
        gems[e] &= full
        if e % per == 0:
            gems[e], beams[e] = 0, 0
        elif e % per == 1:
            gems[e], beams[e] = full, 0xFFFFFFFF
        elif e % per == 2 and G:
            gems[e] = np.uint32(1 << (G - 1))
        if 2 <= e % per < 34:
            beams[e] = np.uint32(1 << (e % per - 2))
        elif 34 <= e % per < 40 and n_words:
            beams[e] = 0
            beams[e, rng.integers(0, n_words)] = np.uint32(1 << int(rng.integers(0, 32)))
    tags = [cell_tags(s) for s in scenes]
    by_tag = []
    for t in tags:
        d = {}
        for c, ts in sorted(t.items()):
            for name in ts - {"source"}:
                d.setdefault(name, []).append(c)
        by_tag.append(d)
    for e in range(n_envs):
        d = by_tag[e // per]
        names = sorted(d)
        for a in range(n_agents):
            if a > 0 and (e % per == 3 or rng.random() < 0.25):
                c = tuple(pos[e, rng.integers(0, a)])
            else:
                cells = d[names[rng.integers(0, len(names))]]
                c = cells[rng.integers(0, len(cells))]
            pos[e, a] = c
    for e, a, c in planted:
        pos[e, a] = c
    return dict(pos=pos, gems=gems, beams=beams[:, :n_words], colours=colours[:, :n_words])


def classes_hit(scenes, pos):
    """The set of cell tags (cell_tags) that hold an agent somewhere in pos [n, A, 2]; no agent may stand on a laser source (the kernel
    documents that a source's cell holds no agent, and the reference would hide one there)."""
    tags = [cell_tags(s) for s in scenes]
    per = len(pos) // len(scenes)
    hit = set()
    for e in range(len(pos)):
        for p in pos[e]:
            ts = tags[e // per][(int(p[0]), int(p[1]))]
            assert "source" not in ts, "a source's cell holds no agent"
            hit |= ts
    return hit


def write_states(bw, pos=None, gems=None, beams=None, colours=None):
    """Write synthetic states straight into the device buffers the renderer reads (BatchedWorld.pos / .gems / .beams / .src_colour
    are views of them).  No step may follow: the engine's invariants are not kept."""
    import torch

    def put(view, arr, as_type):
        if arr is not None and view.numel():
            view.copy_(torch.from_numpy(np.ascontiguousarray(arr).view(as_type).reshape(tuple(view.shape))).to(view.device))
    put(bw.pos, pos, np.uint8)
    put(bw.gems, gems, np.int32)
    put(bw.beams, beams, np.int32)
    put(bw.src_colour, colours, np.uint8)
    torch.cuda.synchronize(bw.device)


def check_frames(bw, atlas, env_ids=None, env_sources=False, where="", dtype=None, cells=None, frames=None):
    """bw.render(env_ids, atlas, dtype) == the restatement of every selected env's current state, byte for byte.  atlas: a
    SpriteAtlas (None: the built-in one).  cells: compare only the tiles of these (i, j) -- with their grid lines --, cropped on the
    device before the copy.  frames: a tensor rendered by the caller (instead of bw.render).  An id outside the batch: zeros."""
    import torch

    from lle_amd.rendering import SpriteAtlas
    dtype = torch.uint8 if dtype is None else dtype
    got = bw.render(env_ids=env_ids, atlas=atlas, dtype=dtype) if frames is None else frames
    assert got.dtype == dtype
    T = TILE_SIZE
    boxes = None if cells is None else [(T * i, T * (i + 1) + 1, T * j, T * (j + 1) + 1) for i, j in cells]

    def to_host(t):  # (0 .. 255 are exact in every dtype; numpy has no bfloat16)
        t = t.contiguous().cpu()
        return (t if t.dtype == torch.uint8 else t.float()).numpy()
    host = [to_host(got)] if boxes is None else [to_host(got[:, y0:y1, x0:x1]) for y0, y1, x0, x1 in boxes]
    states = states_of(bw, env_sources)
    scenes = [Scene.of(m) for m in bw.maps]
    atlas = SpriteAtlas.builtin() if atlas is None else atlas
    ids = list(range(bw.n_envs)) if env_ids is None else [int(e) for e in env_ids]
    assert got.shape[0] == len(ids)
    for s, e in enumerate(ids):
        if 0 <= e < bw.n_envs:
            want = render(scenes[e // bw.envs_per_map], states[e], atlas)
        else:
            want = np.zeros((T * bw.map.height + 1, T * bw.map.width + 1, 3), np.uint8)
        parts = [want] if boxes is None else [want[y0:y1, x0:x1] for y0, y1, x0, x1 in boxes]
        for k, (g, w) in enumerate(zip(host, parts)):
            if not np.array_equal(g[s], w):
                bad = np.argwhere((g[s] != w).any(axis=2))
                oy, ox = (0, 0) if boxes is None else (boxes[k][0], boxes[k][2])
                raise AssertionError(f"{where} env {e} ({dtype}): {len(bad)} pixels differ, first (y, x) {[int(bad[0][0]) + oy, int(bad[0][1]) + ox]}: "
                                     f"got {g[s][tuple(bad[0])].tolist()}, want {w[tuple(bad[0])].tolist()}")
