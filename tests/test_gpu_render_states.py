"""The render kernel (liblle_render.so) over the parts of its domain that rollouts do not reach, against the numpy restatement of the
reference renderer (tests/render_ref.py), byte for byte.

The frame of an environment depends only on `pos`, `gems`, `beams`, `src_colour` and the map tables, and BatchedWorld exposes
those device buffers as torch views: the tests write SYNTHETIC states into them (render_ref.write_states; no step follows, so the
engine's invariants do not matter), read them back (render_ref.states_of) and compare every frame.  Each generator's coverage is
asserted (assert_coverage), not assumed: the cell classes that hold an agent, every gem index, every bit of every beam word, the fallback colours,
and all 2^24 (alpha, foreground, background) triples of one blend in each of the three channel positions.

Also here: the refusals and bounds of the C ABI (include/lle_render.h), rendering into an `out=` slice between canaries, on another
stream and after autotune(), and World's LaserSource mutators followed by get_image()."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from lle_amd import mapgen
from lle_amd._capi import Map
from oracle.levels import LEVELS
from tests import render_ref
from tests.parity_util import EXTRA_MAPS, LONG_MAPS, _grid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPRITES = os.path.join(ROOT, "tests", "golden", "sprites")
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
LLE_ERR_NULL, LLE_ERR_ARG = -1, -2

# 16 agents (ids 12 .. 15 take the fallback sprite of both 12-sprite atlases) and one laser whose beam crosses (0, 1), (0, 2) and the exits
MAP16 = "L0E . . X X X X X X X X X\n" + " ".join(f"S{k}" for k in range(12)) + "\nS12 S13 S14 S15 X X X X X X X X"
# (2, 2): a gem under THREE beams; (2, 1) and (2, 3) under two
THREE_LAYERS = ". . L0S . .\nX . . . X\nL1E . G . L2W\n. . . . .\nS0 S1 . S2 X"
# 16 agents next to one cell of every static tile: floor (1, 0), wall (1, 1), exit (1, 2), void (1, 3)
CHAIN_MAP = _grid(3, 16, {**{(0, k): f"S{k}" for k in range(16)}, (1, 1): "@", (1, 2): "X", (1, 3): "V", **{(2, k): "X" for k in range(16)}})
# the widest and the tallest map the engine takes (LLE_MAX_DIM = 255): two beams of 254 cells (8 words each), a gem and an exit next to
# the closing grid lines, gems under the first and the last cell of a beam
WIDE = _grid(3, 255, {(0, 0): "L0E", (1, 254): "L1W", (2, 0): "S0", (2, 1): "S1", (2, 2): "X", (2, 3): "X", (2, 254): "G", (0, 254): "G",
                      (1, 0): "G", (0, 100): "G", (2, 128): "V", (2, 253): "X", (1, 130): "V"})
TALL = _grid(255, 3, {(0, 0): "L0S", (254, 1): "L1N", (0, 2): "S0", (1, 2): "S1", (2, 2): "X", (3, 2): "X", (254, 2): "G", (254, 0): "G",
                      (0, 1): "G", (100, 0): "G", (128, 2): "V", (253, 2): "X", (130, 1): "V"})
GEMS20 = mapgen.generate(12, 13, 4, 5, 20, seed=9, n_voids=3)  # more than 16 gems, two layers, walls
# 64 x 64 with 2 agents and 4 lasers: the engine refuses a batch of the 64 x 64 map with 6 agents and 8 lasers for a reason of its own (the step
# kernel's tables and row, 194 112 B, exceed the 160 KiB of LDS; lle_batch_create says so), not the renderer
BIG64 = mapgen.generate(64, 64, 2, 4, 24, seed=5, n_voids=6, max_beam=63)
# the frame's byte count 3 (32 H + 1)(32 W + 1) is 3 + 96 (H + W) modulo 128 -- one map per value of (H + W) % 4 -- and 3 modulo 16
# for EVERY map (32 H + 1 = 1 mod 16): no size gives another remainder there
ODD_SIZES = [(2, 3), (3, 3), (3, 4), (4, 4), (5, 7), (1, 6)]
ODD_MAPS = {f"{h}x{w}": mapgen.generate(h, w, 1, 1, 1, n_exits=1, wall_fraction=0.0, n_voids=0, seed=16 * h + w) for h, w in ODD_SIZES}

STATE_MAPS = {k: EXTRA_MAPS[k] for k in ("four_layers", "nested", "voids_gems", "exit_under_beam", "three_beams", "many_agents", "gen_20_lasers")}
STATE_MAPS.update(LONG_MAPS)
STATE_MAPS.update(level6=LEVELS[6], three_layers=THREE_LAYERS, gems20=GEMS20, map16=MAP16)
REQUIRED_CLASSES = {"floor", "exit", "void", "gem", "beam1", "beam2", "beam3", "beam4"}


def _atlas(name):
    from lle_amd.rendering import SpriteAtlas
    if name == "builtin":
        return None
    if name == "reference":
        return SpriteAtlas.from_directory(SPRITES)
    assert name == "custom"  # another count per family: 3 agents, 5 lasers, 2 sources (and their fallbacks), random pixels, random alpha
    return random_atlas(77, 3, 5, 2)


def random_atlas(seed, n_agents, n_lasers, n_sources):
    from lle_amd.rendering import SpriteAtlas
    rng = np.random.default_rng(seed)

    def pixels(*lead):
        return rng.integers(0, 256, lead + (32, 32, 4), dtype=np.uint8)
    return SpriteAtlas(pixels(n_agents + 1), pixels(n_lasers + 1), pixels(n_sources + 1), pixels(), pixels())


def make_batch(maps, n, env_sources):
    """A fresh batch; env_sources: one set_sources with the maps' own (legal) colours, so that render() draws from src_colour."""
    from lle_amd import BatchedWorld
    bw = BatchedWorld(maps, n)
    if env_sources:
        own = np.array([[int(s.agent_id) for s in m.sources()] for m in bw.maps], np.uint8).reshape(len(bw.maps), bw.map.n_sources)
        bw.set_sources(colours=torch.from_numpy(np.repeat(own, bw.envs_per_map, axis=0)))
    return bw


def assert_coverage(maps, arrays):
    """What the states of a batch of 40 envs per map and more cover, asserted on the arrays that are written to the device: every class
    of cell the maps have holds an agent somewhere (never a laser source); every bit of every beam word is on alone in its word, on
    and off across the batch, all on and all off; every gem index is collected and not, all, none and the highest alone."""
    scenes = [render_ref.Scene.of(m) for m in maps]
    present = set().union(*[set().union(*render_ref.cell_tags(s).values()) for s in scenes]) - {"source"}
    hit = render_ref.classes_hit(scenes, arrays["pos"])
    per = len(arrays["pos"]) // len(maps)
    assert per >= 40 and hit == present, f"classes of cells without an agent: {sorted(present - hit)}"
    for k, m in enumerate(maps):
        assert_beam_coverage(arrays["beams"][k * per:(k + 1) * per])
        assert_gem_coverage(arrays["gems"][k * per:(k + 1) * per], m.n_gems)


def assert_beam_coverage(beams):
    if beams.shape[1] == 0:
        return
    assert (np.bitwise_or.reduce(beams, axis=0) == 0xFFFFFFFF).all() and (np.bitwise_and.reduce(beams, axis=0) == 0).all()
    assert (beams == 0xFFFFFFFF).all(axis=1).any() and (beams == 0).all(axis=1).any()
    for w in range(beams.shape[1]):
        alone = {int(v) for v in beams[:, w] if int(v) and int(v) & (int(v) - 1) == 0}
        assert alone == {1 << b for b in range(32)}, f"word {w}: bits never on alone {sorted(set(range(32)) - {v.bit_length() - 1 for v in alone})}"
    assert any(int(v) & (int(v) + 1) for v in beams.reshape(-1)), "only prefixes of beams"


def assert_gem_coverage(gems, G):
    if G == 0:
        return
    full = (1 << G) - 1
    assert (gems == 0).any() and (gems == full).any() and (gems == 1 << (G - 1)).any()
    for g in range(G):
        bit = (gems >> np.uint32(g)) & 1
        assert bit.any() and not bit.all(), f"gem {g}"


def run_states(maps, n, seed, atlases, env_sources, planted=(), edit=None, cover=True, **check):
    """Seeded synthetic states of n envs (render_ref.random_states), changed in place by `edit`, checked for coverage, written and
    compared.  cover=False: batches too small for assert_coverage, or states that `edit` gives over to assertions of the caller's own."""
    maps = [m if isinstance(m, Map) else Map(m) for m in (maps if isinstance(maps, (list, tuple)) else [maps])]
    scenes = [render_ref.Scene.of(m) for m in maps]
    arrays = render_ref.random_states(scenes, n, maps[0].n_agents, maps[0].n_beam_words, seed, planted)
    if edit is not None:
        edit(arrays)
    if cover:
        assert_coverage(maps, arrays)
    render_ref.classes_hit(scenes, arrays["pos"])  # (no agent on a source)
    bw = make_batch(maps if len(maps) > 1 else maps[0], n, env_sources)
    if not env_sources:
        arrays = {k: v for k, v in arrays.items() if k != "colours"}
    render_ref.write_states(bw, **arrays)
    for name in atlases:
        render_ref.check_frames(bw, _atlas(name), env_sources=env_sources, where=f"atlas {name}", **check)
    return bw, arrays


# ------------------------------------------------------------------------------------------------ 1. synthetic states
@pytest.mark.parametrize("atlas", ["builtin", "reference"])
@pytest.mark.parametrize("name", sorted(STATE_MAPS))
def test_synthetic_states(name, atlas):
    """Any subset of gems, arbitrary beam words, agents on every class of cell the map has (several on one cell), and -- with the
    reference's sprites -- any byte as the colour of every beam word; with the built-in ones the maps' own colours."""
    run_states(STATE_MAPS[name], 48, 1000 + len(name), [atlas], env_sources=atlas == "reference")


def test_state_maps_hold_every_class_of_cell():
    """test_synthetic_states asserts that an agent stands on every class of cell its map has; together the maps have every class
    there is: floor, exit, void, gem, and beam cells with 1, 2, 3 and 4 layers.  More than 16 gems and three beam words too."""
    tags = set()
    for text in STATE_MAPS.values():
        tags |= set().union(*render_ref.cell_tags(render_ref.Scene.of(Map(text))).values())
    assert REQUIRED_CLASSES | {"wall"} <= tags
    assert Map(GEMS20).n_gems == 20
    m = Map(LONG_MAPS["long_three_words"])
    assert max(-(-int(s.length) // 32) for s in m.sources()) == 3


@pytest.mark.parametrize("atlas", ["builtin", "reference"])
def test_four_layers_deepest_cell(atlas):
    """All agents on the gem under four beams at (2, 2) -- the longest draw list there is -- with the gem present and collected and
    every subset of the four layers on."""
    m = Map(EXTRA_MAPS["four_layers"])
    layers = [(int(c.word), int(c.bit)) for c in m.cell_layers() if (c.i, c.j) == (2, 2)]
    assert len(layers) == 4 and (2, 2) in render_ref.Scene.of(m).gems

    def edit(arrays):
        for e in range(32):
            arrays["pos"][e, :] = (2, 2)
            arrays["gems"][e] = (e & 1) * ((1 << m.n_gems) - 1)
            arrays["beams"][e] = 0
            for k, (word, bit) in enumerate(layers):
                if (e >> (k + 1)) & 1:
                    arrays["beams"][e, word] |= np.uint32(1 << bit)
    run_states(m, 40, 5, [atlas], env_sources=True, edit=edit, cover=False)


@pytest.mark.parametrize("atlas", ["builtin", "reference", "custom"])
def test_sixteen_agents_on_one_cell(atlas):
    """1 .. 16 agents on the beam cell, then all sixteen on a beam-and-exit cell, a start and the last cell of the last row: the
    agents are blended in id order, ids beyond the atlas's numbered sprites with its fallback."""
    m = Map(MAP16)
    a = _atlas(atlas)
    assert m.n_agents == 16 and (12 if a is None else a.n_agents) < 16
    rng = np.random.default_rng(16)

    def edit(arrays):
        pos = arrays["pos"]
        for e in range(16):                      # agents 0 .. e (a random set of e + 1 in the second half) on (0, 1), the others spread
            on = np.arange(e + 1)
            pos[e] = [(1 + k // 12, k % 12) for k in range(16)]
            pos[e, on] = (0, 1)
            pos[16 + e] = pos[e]
            pos[16 + e, rng.permutation(16)[:e + 1]] = (0, 2)
            arrays["beams"][e] = arrays["beams"][16 + e] = 0xFFFFFFFF
        for e, cell in zip(range(32, 36), [(0, 3), (1, 0), (2, 11), (0, 1)]):
            pos[e] = cell
        arrays["beams"][35] = 0
    bw, arrays = run_states(m, 48, 6, [atlas], env_sources=True, edit=edit, cover=False)
    assert (arrays["pos"][15] == (0, 1)).all() and (arrays["pos"][34] == (2, 11)).all()


@pytest.mark.parametrize("atlas", ["builtin", "reference", "custom"])
@pytest.mark.parametrize("name", ["four_layers", "three_layers", "long_three_words", "nested"])
def test_source_colours_any_byte(name, atlas):
    """src_colour overwritten with any byte after one legal set_sources: numbered colours, the first one beyond the atlas (its
    count), 12, 13 and 255; laser sprites take theirs per beam word, source sprites from the first word of the source, in all
    four directions.  The custom atlas has another count per family (3 / 5 / 2): exchanging one clamp or the source stride for
    another draws another sprite."""
    text = THREE_LAYERS if name == "three_layers" else {**EXTRA_MAPS, **LONG_MAPS}[name]
    m = Map(text)
    a = _atlas(atlas)
    counts = (12, 12) if a is None else (a.n_lasers, a.n_sources)

    def edit(arrays):
        c = arrays["colours"]
        for e in range(20):
            c[e] = e                                   # every word the same colour 0 .. 19
        c[20], c[21] = 255, 254
        if c.shape[1] > 1:
            c[22] = np.arange(c.shape[1]) + 11            # 11, 12, 13, ...: neighbours differ
        arrays["beams"][:24] = 0xFFFFFFFF
    bw, arrays = run_states(m, 48, 7, [atlas], env_sources=True, edit=edit, cover=False)
    seen = set(arrays["colours"].reshape(-1).tolist())
    assert {0, 1, 2, 3, 4, 5, 11, 12, 13, 255} <= seen and all(n - 1 in seen and n in seen and n + 1 in seen for n in counts)
    if name == "four_layers":
        assert {int(s.direction) for s in m.sources()} == {0, 1, 2, 3}
    if name == "long_three_words":  # the words of one source carry different colours: a laser sprite takes its own word's
        first = m.source_first_words()
        c = arrays["colours"]
        assert any(len(set(c[e, first[0]:first[0] + 3].tolist())) == 3 for e in range(48))


# ------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_maximum_width_and_height(name):
    """3 x 255 and 255 x 3, the renderer's and the engine's limit: whole frames of every env as uint8 (beams of 8 words each, every bit
    on alone), then every dtype on a subset with ids outside the batch; an agent on the gem in the last row and column."""
    m = Map(WIDE if name == "wide" else TALL)
    assert (m.height, m.width) == ((3, 255) if name == "wide" else (255, 3)) and m.n_beam_words == 16
    last = (m.height - 1, m.width - 1)
    assert last in render_ref.Scene.of(m).gems
    planted = [(4, 0, last), (4, 1, last), (5, 0, last), (5, 1, (last[0] - (name == "tall"), last[1] - (name == "wide")))]
    g = render_ref.Scene.of(m).gems.index(last)

    def edit(arrays):  # the gem under the agents present in env 4, collected in env 5
        arrays["gems"][4] &= ~np.uint32(1 << g)
        arrays["gems"][5] |= np.uint32(1 << g)
    bw, arrays = run_states(m, 40, 8, ["builtin"], env_sources=True, planted=planted, edit=edit)
    assert (arrays["pos"][4] == last).all() and tuple(arrays["pos"][5, 0]) == last
    for dt in DTYPES:
        render_ref.check_frames(bw, None, env_ids=[4, 40, 1, -1, 39, 5, 5], env_sources=True, where=name, dtype=dt)
    render_ref.check_frames(bw, _atlas("reference"), env_ids=[0, 1, 4, 5, 17], env_sources=True, where=name + " reference")


def test_64_by_64():
    m = Map(BIG64)
    assert (m.height, m.width) == (64, 64) and m.n_gems == 24
    last = (63, 63)
    planted = [(1, 0, last)] if "source" not in render_ref.cell_tags(render_ref.Scene.of(m))[last] else []
    bw, _ = run_states(m, 6, 9, ["builtin"], env_sources=True, planted=planted, cover=False)
    some = [last, (0, 0), (31, 32), (63, 0)] + [tuple(c) for c in render_ref.Scene.of(m).gems[16:]]  # (cropped on the device)
    render_ref.check_frames(bw, _atlas("reference"), env_ids=[5, 6, 1], env_sources=True, dtype=torch.float16, cells=some, where="64x64 f16")


@pytest.mark.parametrize("size", sorted(ODD_MAPS))
def test_frame_sizes(size):
    """One map per remainder of the frame's byte count modulo 128 (the module's comment on ODD_SIZES has the arithmetic), every dtype,
    env subsets with an id out of range, an agent in the last row and column."""
    m = Map(ODD_MAPS[size])
    last = (m.height - 1, m.width - 1)
    planted = [(1, 0, last)] if "source" not in render_ref.cell_tags(render_ref.Scene.of(m))[last] else []
    bw, _ = run_states(m, 8, 10, ["builtin", "reference"], env_sources=True, planted=planted, cover=False)
    for dt in DTYPES:
        render_ref.check_frames(bw, None, env_ids=[7, 8, 1, 0, -3], env_sources=True, where=size, dtype=dt)


def test_frame_sizes_cover_every_remainder():
    nbytes = [3 * (32 * h + 1) * (32 * w + 1) for h, w in ODD_SIZES]
    assert {b % 128 for b in nbytes} == {3, 35, 67, 99} and {b % 16 for b in nbytes} == {3}
    assert all(3 * (32 * h + 1) * (32 * w + 1) % 16 == 3 for h in range(1, 256) for w in (1, 2, 3, 100, 255))


@pytest.mark.parametrize("per", [1, 2, 3, 5, 8, 16])
def test_blocks_of_maps_synthetic(per):
    """The generated trio of test_gpu_render.test_blocks_of_maps: env / envs_per_map picks the tables while the states differ per env."""
    maps = [mapgen.generate(height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2, seed=200 + s) for s in range(3)]
    run_states(maps, 3 * per, 11 + per, ["builtin"], env_sources=per % 2 == 1, cover=False)


# ------------------------------------------------------------------------------------------------ 2. the blend
N_BLEND_ATLASES = 5  # 65 536 (alpha, fg) pairs per channel / (16 sprites x 961 visible pixels) = 4.3


def blend_atlas(k):
    """Atlas k of the blend test.  Laser sprite c (256 numbered) is opaque with value c in every channel: the background under an
    agent on a lit beam cell is exactly c.  The 961 pixels of a tile that the grid does not cover, of the 16 agent sprites of the 5
    atlases, enumerate the pairs: pixel p holds alpha = p >> 8 and fg = p & 255 in the first channel, fg ^ 0x55 and fg ^ 0xAA in
    the other two (each channel sees every pair; no two channels the same value)."""
    from lle_amd.rendering import SpriteAtlas
    p = ((np.arange(16 * 961) + k * 16 * 961) % 65536).reshape(16, 31, 31)
    agents = np.full((17, 32, 32, 4), 77, np.uint8)
    agents[:16, 1:, 1:, 0] = p & 255
    agents[:16, 1:, 1:, 1] = (p & 255) ^ 0x55
    agents[:16, 1:, 1:, 2] = (p & 255) ^ 0xAA
    agents[:16, 1:, 1:, 3] = p >> 8
    lasers = np.zeros((257, 32, 32, 4), np.uint8)
    lasers[:256, :, :, :3] = np.arange(256, dtype=np.uint8)[:, None, None, None]
    lasers[..., 3] = 255
    zeros = np.zeros((32, 32, 4), np.uint8)
    return SpriteAtlas(agents, lasers, np.zeros((2, 32, 32, 4), np.uint8), zeros, zeros)


def blend_plan(start_pos):
    """Env 16 c + a: agent a on the beam cell (0, 1), the others on their starts, the beam's colour c."""
    n = 4096
    pos = np.repeat(np.asarray(start_pos, np.uint8)[None], n, axis=0)
    for e in range(n):
        pos[e, e % 16] = (0, 1)
    colours = (np.arange(n) // 16).astype(np.uint8).reshape(n, 1)
    return pos, colours


def test_every_blend_triple():
    """Every (alpha, fg, bg) in 0 .. 255 cubed, in each of the three channel positions of the packed word, against render_ref.blend: the
    shortcuts at alpha 0 and 255 and every rounding of (1 - a) * bg + a * fg, which an FMA would change."""
    from lle_amd._capi import LLE_POS_START
    m = Map(MAP16)
    tile = [t for t in m.laser_tiles() if (t.i, t.j) == (0, 1)]
    assert len(tile) == 1 and m.n_beam_words == 1
    bw = make_batch(m, 4096, True)
    start = bw.pos.cpu().numpy()[0]
    assert sorted(map(tuple, start.tolist())) == sorted(m.positions(LLE_POS_START))
    pos, colours = blend_plan(start)
    beams = np.full((4096, 1), 1 << int(tile[0].bit), np.uint32)
    render_ref.write_states(bw, pos=pos, beams=beams, colours=colours)
    assert np.array_equal(bw.src_colour.cpu().numpy(), colours) and np.array_equal(bw.pos.cpu().numpy(), pos)
    out = torch.empty(int(bw.render_desc(atlas=blend_atlas(0)).bytes), dtype=torch.uint8, device=bw.device)
    seen = np.zeros((3, 256, 256, 256), dtype=bool)
    bg = colours.reshape(256, 16)[:, 0]
    assert np.array_equal(bg, np.arange(256))
    for k in range(N_BLEND_ATLASES):
        atlas = blend_atlas(k)
        got = bw.render(out=out, atlas=atlas)[:, 1:32, 33:64].contiguous().cpu().numpy().reshape(256, 16, 31, 31, 3)
        fg = atlas.agents[:16, 1:, 1:]                                             # [16, 31, 31, 4]: env 16 c + a shows sprite a
        want = render_ref.blend(np.broadcast_to(bg[:, None, None, None, None], got.shape), fg[None])
        if not np.array_equal(got, want):
            c, a, y, x, ch = (int(v) for v in np.argwhere(got != want)[0])
            raise AssertionError(f"atlas {k}: {int((got != want).sum())} values differ; alpha {fg[a, y, x, 3]}, fg {fg[a, y, x, ch]}, bg {c}, "
                                 f"channel {ch}: got {got[c, a, y, x, ch]}, want {want[c, a, y, x, ch]}")
        for ch in range(3):  # the bookkeeping, from the sprites and colours that were uploaded
            seen[ch, fg[None, ..., 3], fg[None, ..., ch], bg[:, None, None, None]] = True
    assert seen.all() and int(seen.sum()) == 3 * 2 ** 24


def test_blend_chains():
    """Up to 16 random RGBA sprites on one cell over each of the four static tiles (floor, wall, exit, void): the truncated result of
    one blend is the background of the next."""
    m = Map(CHAIN_MAP)
    targets = [(1, 0), (1, 1), (1, 2), (1, 3)]
    tags = render_ref.cell_tags(render_ref.Scene.of(m))
    assert [sorted(tags[t]) for t in targets] == [["floor"], ["wall"], ["exit"], ["void"]] and m.n_agents == 16
    n = 64
    rng = np.random.default_rng(2)
    pos = np.zeros((n, 16, 2), np.uint8)
    for e in range(n):
        pos[e] = [(0, k) for k in range(16)]
        pos[e, rng.permutation(16)[:e // 4 + 1]] = targets[e % 4]
    assert all((pos[60 + t] == targets[t]).all() for t in range(4))  # sixteen on each tile
    bw = make_batch(m, n, False)
    render_ref.write_states(bw, pos=pos)
    for seed in (3, 4):
        render_ref.check_frames(bw, random_atlas(seed, 16, 1, 1), where=f"chains, atlas {seed}")


# ------------------------------------------------------------------------------------------------ 4. the C ABI
def _c_atlas(a, counts=None):
    from lle_amd import rendering
    na, nl, ns = counts or (a.n_agents, a.n_lasers, a.n_sources)
    return rendering.RenderAtlas(na, nl, ns, 0, a.agents.ctypes.data, a.lasers.ctypes.data, a.sources.ctypes.data, a.gem.ctypes.data, a.void.ctypes.data)


def test_refusals_leave_the_output_alone():
    """Every refusal of include/lle_render.h: its error code, a message in lle_render_last_error, and not one byte written."""
    from lle_amd import BatchedWorld, rendering
    L = rendering.lib()
    bw = BatchedWorld(LEVELS[6], 8)
    atlas = rendering.SpriteAtlas.builtin()
    handles = (C.c_void_p * 2)(bw.map.h, bw.map.h)
    for n_maps, counts, word in [(2, None, b"n_maps"), (0, None, b"n_maps"), (1, (-1, 12, 12), b"negative"), (1, (12, -1, 12), b"negative"),
                                 (1, (12, 12, -5), b"negative")]:
        st = _c_atlas(atlas, counts)
        assert not L.lle_render_create(bw.h, handles, n_maps, C.byref(st), bw._stream())
        assert word in L.lle_render_last_error(), (n_maps, counts, L.lle_render_last_error())
    r = bw._renderer(None)
    good = bw.render().clone()
    d = rendering.RenderDesc()
    for n_sel, dtype in [(-1, 0), (1, -1), (1, 4), (-5, 7)]:
        assert L.lle_render_desc_of(r.h, n_sel, dtype, C.byref(d)) == LLE_ERR_ARG and b"n_sel or dtype" in L.lle_render_last_error()
    assert L.lle_render_desc_of(r.h, 1, 0, None) == LLE_ERR_NULL and L.lle_render_desc_of(None, 1, 0, C.byref(d)) == LLE_ERR_NULL
    need = int(r.desc(8, 0).bytes)
    canary = torch.full((2 * need + 64,), 0xA5, dtype=torch.uint8, device=bw.device)
    ptr = canary.data_ptr()
    assert ptr % 16 == 0
    ids = torch.arange(16, device=bw.device, dtype=torch.int64)
    cases = [  # (env ids, n_sel, flags, dtype, out, out_bytes, code, word of the message)
        (None, 8, 0, 0, ptr, need - 1, LLE_ERR_ARG, b"smaller"),
        (None, 8, 0, 3, ptr, need, LLE_ERR_ARG, b"smaller"),          # float32 needs four times the bytes
        (None, 8, 0, 0, ptr, 0, LLE_ERR_ARG, b"smaller"),
        (None, 8, 0, 0, ptr + 8, need, LLE_ERR_ARG, b"aligned"),
        (None, 8, 0, 0, ptr + 1, need, LLE_ERR_ARG, b"aligned"),
        (None, 8, 2, 0, ptr, need, LLE_ERR_ARG, b"flags"),
        (None, 8, 0x80000001, 0, ptr, need, LLE_ERR_ARG, b"flags"),
        (None, 9, 0, 0, ptr, 2 * need, LLE_ERR_ARG, b"n_envs"),
        (None, 8, 0, 0, None, need, LLE_ERR_NULL, b"NULL"),
        (None, -1, 0, 0, ptr, need, LLE_ERR_ARG, b"n_sel or dtype"),
        (None, 8, 0, 4, ptr, need, LLE_ERR_ARG, b"n_sel or dtype"),
        (None, 0, 0, 0, ptr, need, 0, None),                          # n_sel == 0 succeeds and writes nothing
        (ids.data_ptr(), 0, 1, 2, ptr, 0, 0, None),
    ]
    for ids_ptr, n_sel, flags, dtype, out, out_bytes, code, word in cases:
        rc = L.lle_render_frame(r.h, ids_ptr, n_sel, flags, dtype, out, out_bytes, bw._stream())
        assert rc == code, (n_sel, flags, dtype, out_bytes, rc, L.lle_render_last_error())
        assert word is None or word in L.lle_render_last_error(), L.lle_render_last_error()
        torch.cuda.synchronize(bw.device)
        assert bool((canary == 0xA5).all()), (n_sel, flags, dtype, out_bytes)
    assert L.lle_render_frame(None, None, 8, 0, 0, ptr, need, bw._stream()) == LLE_ERR_NULL
    # lle_render_update_map: an index out of range, a map of another shape, a map of the same shape with another number of draw operations
    other, fewer = Map("S0 . X"), Map(LEVELS[6].replace("G", ".", 1))
    assert (fewer.height, fewer.width, fewer.n_agents, fewer.n_sources) == (bw.map.height, bw.map.width, bw.map.n_agents, bw.map.n_sources)
    for index, map_, code, word in [(-1, bw.map, LLE_ERR_ARG, b"out of range"), (1, bw.map, LLE_ERR_ARG, b"out of range"),
                                    (0, other, LLE_ERR_ARG, b"recompilation"), (0, fewer, LLE_ERR_ARG, b"recompilation")]:
        assert L.lle_render_update_map(r.h, index, map_.h, bw._stream()) == code and word in L.lle_render_last_error(), (index, word)
    assert L.lle_render_update_map(r.h, 0, None, bw._stream()) == LLE_ERR_NULL
    # more ids than envs is fine WITH ids; and after all the refusals the renderer draws what it drew before
    assert L.lle_render_frame(r.h, ids.data_ptr(), 16, 0, 0, ptr, 2 * need, bw._stream()) == 0
    assert torch.equal(bw.render(), good)
    torch.cuda.synchronize(bw.device)
    assert bool((canary[2 * need:] == 0xA5).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("size", ["level6", "3x4", "5x7"])
def test_out_slice_between_canaries(size, dtype):
    """An odd n_sel into a slice of exactly desc.bytes inside a larger buffer: not a byte before or after it changes."""
    bw = make_batch(Map(LEVELS[6] if size == "level6" else ODD_MAPS[size]), 8, False)
    ids = [6, 0, 3]
    need = int(bw.render_desc(len(ids), dtype).bytes)
    guard = 4096
    big = torch.full((need + 2 * guard,), 0x5A, dtype=torch.uint8, device=bw.device)
    frames = bw.render(env_ids=ids, out=big[guard:guard + need], dtype=dtype)
    torch.cuda.synchronize(bw.device)
    assert frames.data_ptr() == big.data_ptr() + guard
    assert bool((big[:guard] == 0x5A).all()) and bool((big[guard + need:] == 0x5A).all())
    render_ref.check_frames(bw, None, env_ids=ids, frames=frames, dtype=dtype, where="out=")
    with pytest.raises(AssertionError):
        bw.render(env_ids=ids, out=big[guard:guard + need - 1], dtype=dtype)


@pytest.mark.parametrize("size", ["level6"] + sorted(ODD_MAPS))
def test_render_desc_is_the_headers(size):
    """include/lle_render.h: shape (n_sel, 32H+1, 32W+1, 3); strides in elements; stride[0] is the frame's element count rounded up to
    128, for every dtype; bytes = n_sel * stride[0] * elem_bytes."""
    bw = make_batch(Map(LEVELS[6] if size == "level6" else ODD_MAPS[size]), 4, False)
    Hp, Wp = 32 * bw.map.height + 1, 32 * bw.map.width + 1
    pitch = -(-3 * Hp * Wp // 128) * 128
    for dtype, eb in zip(DTYPES, (1, 2, 2, 4)):
        for n_sel in (0, 1, 3, 4, 7):
            d = bw.render_desc(n_sel, dtype)
            assert (d.elem_bytes, d.ndim, list(d.shape), list(d.stride), d.bytes) == (eb, 4, [n_sel, Hp, Wp, 3], [pitch, 3 * Wp, 3, 1], n_sel * pitch * eb)
        frames = bw.render(env_ids=[1, 2, 3], dtype=dtype)
        assert frames.dtype == dtype and tuple(frames.shape) == (3, Hp, Wp, 3) and frames.stride() == (pitch, 3 * Wp, 3, 1)


def test_other_stream_and_after_autotune():
    """The renderer caches the batch's buffer pointers at creation: frames on a non-default torch stream, and after
    BatchedWorld.autotune() and a step, are still the current state's."""
    from lle_amd import BatchedWorld
    bw = BatchedWorld(LEVELS[6], 64)
    render_ref.check_frames(bw, None, env_ids=[0, 63], where="fresh")
    side = torch.cuda.Stream(device=bw.device)
    side.wait_stream(torch.cuda.current_stream(bw.device))
    with torch.cuda.stream(side):
        for t in range(3):
            bw.step(sample=True, auto_reset=True, seed=4, t=t)
        frames = bw.render()
        side.synchronize()
        render_ref.check_frames(bw, None, frames=frames, where="side stream")
    bw.autotune(5.0)
    render_ref.check_frames(bw, None, env_ids=[0, 1, 62, 63], where="after autotune")
    bw.step(sample=True, auto_reset=True, seed=4, t=0)
    bw.step(sample=True, auto_reset=True, seed=4, t=1)
    render_ref.check_frames(bw, None, where="autotune, then steps")
    render_ref.check_frames(bw, _atlas("reference"), env_ids=[5, 6], where="a renderer made after autotune")


# ------------------------------------------------------------------------------------------------ 5. World sources
def _world_frame(w):
    from lle_amd.rendering import SpriteAtlas
    img = w.get_image()
    want = render_ref.render(render_ref.Scene.of(w._map), render_ref.states_of(w._batch)[0], SpriteAtlas.builtin())
    assert np.array_equal(img, want)
    return img


def test_world_source_mutators_are_rendered():
    """LaserSource.set_colour / disable / enable go through update_sources and a rebuild of the renderer's op words (they carry the
    map's colours): get_image() afterwards is the restatement of the changed world, and differs from the frame before."""
    from lle_amd import World
    from lle_amd.rendering import SpriteAtlas
    w = World("S0 . . X\n. . . .\nS1 . G X\n. L0N . .")
    first = _world_frame(w)
    src = w.laser_sources[0]
    src.set_colour(1)
    recoloured = _world_frame(w)
    assert not np.array_equal(recoloured, first) and w.laser_sources[0].agent_id == 1
    src.disable()
    off = _world_frame(w)
    assert not np.array_equal(off, recoloured) and not render_ref.states_of(w._batch)[0].beam_words[0]
    assert np.array_equal(off[97:129, 33:65], recoloured[97:129, 33:65])  # the source itself is drawn all the same
    src.enable()
    on = _world_frame(w)
    assert np.array_equal(on, recoloured) and not np.array_equal(on, off)
    src.set_colour(0)
    assert np.array_equal(_world_frame(w), first)
    # the refused change (pylaser_source.rs:107-141 recolours the world before it checks the starts): the frame shows the new colour
    w = World("L0E X X . S0\n@ @ @ S1 .")
    before = _world_frame(w)
    with pytest.raises(ValueError, match="cross the start position"):
        w.laser_sources[0].set_colour(1)
    after = _world_frame(w)
    assert not np.array_equal(after, before) and int(w._map.sources()[0].agent_id) == 1
    assert np.array_equal(after[1:32, 1:32], SpriteAtlas.builtin().sources[1][1:, 1:, :3])
    assert np.array_equal(before[1:32, 1:32], SpriteAtlas.builtin().sources[0][1:, 1:, :3])
