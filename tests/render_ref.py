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
