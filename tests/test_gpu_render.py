"""Frames of the render kernel (liblle_render.so) against the numpy restatement of the reference renderer (tests/render_ref.py),
byte for byte, with the package's own sprites and with the reference's (tests/golden/sprites): every level, the extra and long
maps, a 13-agent map that needs the fallback sprites, rollouts with deaths and auto-resets (the engine's states checked against the
oracle), per-environment colours with disabled sources, blocks of maps, env subsets, moved exits, every dtype, and the public
entry points (World.get_image, the "rgb-image" generator, BatchedLLE)."""
import os

import numpy as np
import pytest
import torch

from oracle.levels import LEVELS
from tests import render_ref
from tests.parity_util import EXTRA_MAPS, LONG_MAPS, legal_colours

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPRITES = os.path.join(ROOT, "tests", "golden", "sprites")
L12E = ("L12E .  .  .  .  .  .  .  .  .  .   .   .   X\n"  # ref:src/unit_tests/test_renderer.rs:28-37
        "S0  S1 S2 S3 S4 S5 S6 S7 S8 S9 S10 S11 S12 .\n"
        "X    X  X  X  X  X  X  X  X  X  X   X   X   .")


def _atlas(name):
    from lle_amd.rendering import SpriteAtlas
    return SpriteAtlas.builtin() if name == "builtin" else SpriteAtlas.from_directory(SPRITES)


def check_frames(bw, atlas_name, env_ids=None, env_sources=False, where=""):
    """bw.render(env_ids) == the restatement of every selected env's current state."""
    atlas = _atlas(atlas_name)
    got = bw.render(env_ids=env_ids, atlas=None if atlas_name == "builtin" else atlas)
    torch.cuda.synchronize(bw.device)
    got = got.cpu().numpy()
    states = render_ref.states_of(bw, env_sources)
    scenes = [render_ref.Scene.of(m) for m in bw.maps]
    ids = range(bw.n_envs) if env_ids is None else env_ids
    for s, e in enumerate(ids):
        want = render_ref.render(scenes[e // bw.envs_per_map], states[e], atlas)
        if not np.array_equal(got[s], want):
            bad = np.argwhere((got[s] != want).any(axis=2))
            raise AssertionError(f"{where} env {e}: {len(bad)} pixels differ, first (y, x) {bad[0].tolist()}: "
                                 f"got {got[s][tuple(bad[0])].tolist()}, want {want[tuple(bad[0])].tolist()}")


MAPS = {f"level{k}": LEVELS[k] for k in range(1, 7)}
MAPS.update(EXTRA_MAPS)
MAPS.update(LONG_MAPS)
MAPS["l12e"] = L12E


@pytest.mark.parametrize("atlas", ["builtin", "reference"])
@pytest.mark.parametrize("name", sorted(MAPS))
def test_rollout_frames(name, atlas):
    """Reset, then sampled steps with auto-reset: deaths, exits, gems, beams cut and restored."""
    from lle_amd import BatchedWorld
    n = 4
    bw = BatchedWorld(MAPS[name], n)
    check_frames(bw, atlas, where=f"{name} reset")
    for t in range(6):
        bw.step(sample=True, auto_reset=True, seed=7, t=t)
        if t % 2 == 1:
            check_frames(bw, atlas, where=f"{name} t={t}")


def test_rollout_states_are_the_oracles():
    """Level 6: the states rendered along a rollout are the oracle's (deaths and auto-resets included), frame by frame."""
    from lle_amd import BatchedWorld
    from oracle import oracle
    from tests.parity_util import assert_state_equal, unpack_engine
    n = 16
    bw = BatchedWorld(LEVELS[6], n)
    ob = oracle.OracleBatch(LEVELS[6], n)
    dims = (ob.A, ob.G, ob.Ls, ob.beam_stride, ob.C, ob.H, ob.W)
    deaths = 0
    for t in range(24):
        bw.step(sample=True, auto_reset=True, seed=99, t=t)
        ob.step(None, auto_reset=True, seed=99, t=t)
        assert_state_equal(unpack_engine(bw.host_buffers(), *dims), ob.dump(), f"t={t}")
        deaths += bw.stats()["deaths"]
        if t % 6 == 5:
            check_frames(bw, "builtin", where=f"t={t}")
    assert deaths > 0


@pytest.mark.parametrize("atlas", ["builtin", "reference"])
@pytest.mark.parametrize("name", ["level6", "nested", "four_layers", "colour_alias"])
def test_per_env_colours_and_disabled_sources(name, atlas):
    from lle_amd import BatchedWorld
    n = 8
    bw = BatchedWorld(MAPS[name], n)
    L, A = bw.map.n_sources, bw.map.n_agents
    g = torch.Generator().manual_seed(3)
    colours = legal_colours(bw.map, torch.randint(0, A, (n, L), generator=g, dtype=torch.uint8))
    enabled = torch.randint(0, 1 << L, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    bw.set_sources(colours=colours, enabled=enabled)
    check_frames(bw, atlas, env_sources=True, where=f"{name} set_sources")
    for t in range(4):
        bw.step(sample=True, auto_reset=True, seed=5, t=t)
    check_frames(bw, atlas, env_sources=True, where=f"{name} stepped")


@pytest.mark.parametrize("per", [1, 2, 3, 5, 8, 16])
def test_blocks_of_maps(per):
    from lle_amd import BatchedWorld, mapgen
    maps = [mapgen.generate(height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2, seed=200 + s) for s in range(3)]
    bw = BatchedWorld(maps, 3 * per)
    for t in range(3):
        bw.step(sample=True, auto_reset=True, seed=11, t=t)
    check_frames(bw, "builtin", where=f"per={per}")


def test_env_subsets():
    from lle_amd import BatchedWorld
    bw = BatchedWorld(LEVELS[6], 32)
    for t in range(5):
        bw.step(sample=True, auto_reset=True, seed=1, t=t)
    ids = [31, 0, 7, 7, 18]
    check_frames(bw, "builtin", env_ids=ids, where="subset")
    full = bw.render().cpu()
    sub = bw.render(env_ids=torch.tensor(ids, device=bw.device)).cpu()
    assert torch.equal(sub, full[ids])
    out = bw.render(env_ids=[2, -1, 32]).cpu()  # ids outside the batch: frames of zeros
    assert torch.equal(out[0], full[2]) and not out[1].any() and not out[2].any()


def test_exit_changes():
    from lle_amd import BatchedWorld, World
    text = "S0 . . X\n. . . .\nS1 . G X\n. L0N . ."  # (1, 1) lies under the beam
    bw = BatchedWorld(text, 4)
    check_frames(bw, "builtin", where="before")
    bw.set_exits([(1, 1), (1, 3)])
    check_frames(bw, "builtin", where="after set_exits")
    w = World(text)
    before = w.get_image()
    w.exit_pos = [(1, 2), (1, 0)]
    after = w.get_image()
    assert not np.array_equal(before, after)
    want = render_ref.render(render_ref.Scene.of(w._map), render_ref.states_of(w._batch)[0], _atlas("builtin"))
    assert np.array_equal(after, want)


def test_every_dtype_is_the_uint8_frame():
    from lle_amd import BatchedWorld
    from lle_amd import rendering
    bw = BatchedWorld(LEVELS[6], 8)
    for t in range(3):
        bw.step(sample=True, auto_reset=True, seed=2, t=t)
    ref = bw.render().clone()
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        got = bw.render(dtype=dt)
        assert got.dtype == dt and got.shape == ref.shape
        assert torch.equal(got.float(), ref.float()), dt
    # every kernel compiled into liblle_render.so has been launched by this process
    import importlib.util
    spec = importlib.util.spec_from_file_location("compiled_kernels", os.path.join(ROOT, "tools", "compiled_kernels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    compiled = set(mod.compiled_kernels(lib=rendering.LIB_PATH))
    assert compiled == {f"render_kernel<{k}>" for k in range(4)}
    assert compiled <= set(rendering.launched_kernels())


def test_world_get_image_and_generator():
    from lle_amd import World
    from lle_amd.observations import ObservationType
    w = World("S0 . X")
    img = w.get_image()
    assert img.dtype == np.uint8 and img.shape == (33, 97, 3) and img.max() > img.min()
    w6 = World.level(6)
    img6 = w6.get_image()
    assert img6.shape == (385, 417, 3)
    want = render_ref.render(render_ref.Scene.of(w6._map), render_ref.states_of(w6._batch)[0], _atlas("builtin"))
    assert np.array_equal(img6, want)
    gen = ObservationType.RGB_IMAGE.get_observation_generator(w6)
    assert gen.shape == (385, 417, 3) and gen.obs_type == ObservationType.RGB_IMAGE
    obs = gen.observe()
    assert obs.dtype == np.float32 and obs.shape == (w6.n_agents, 385, 417, 3)
    assert np.array_equal(obs[w6.n_agents - 1], img6.astype(np.float32))
    assert np.array_equal(gen.get_state(), img6.astype(np.float32))


def test_batched_lle_rgb_image():
    from lle_amd.env import BatchedLLE
    env = BatchedLLE.level(6).obs_type("rgb-image").state_type("rgb-image").build(4096)
    obs, state = env.reset()
    assert env.observation_shape == (4, 385, 417, 3) and env.state_shape == (385, 417, 3)
    assert obs.shape == (4096, 4, 385, 417, 3) and obs.dtype == torch.uint8 and state.shape == (4096, 385, 417, 3)
    actions = torch.zeros((4096, 4), dtype=torch.uint8, device=env.world.device) + 4  # STAY
    for persistent in (False, True):
        out = env.step(actions, auto_reset=True, persistent=persistent)
        sel = [0, 1, 4095]
        frames = env.world.render(env_ids=sel).cpu()
        assert torch.equal(out["obs"][sel, 3].cpu(), frames) and torch.equal(out["state"][sel].cpu(), frames)
    check_frames(env.world, "builtin", env_ids=[0, 2048, 4095], where="BatchedLLE")
    assert np.array_equal(env.get_image(5), env.world.render(env_ids=[5])[0].cpu().numpy())
    f32 = BatchedLLE.level(3).obs_type("rgb-image").build(4, obs_dtype=torch.float32)
    o, _ = f32.reset()
    assert o.dtype == torch.float32 and torch.equal(o[:, 0].cpu(), f32.world.render().cpu().float())


def test_renderers_are_kept_per_atlas_content():
    """Atlases with the same sprites share one renderer (BatchedWorld keys them by SpriteAtlas.digest): rendering with a fresh
    SpriteAtlas.from_directory(...) object every call creates no further renderer."""
    from lle_amd import BatchedWorld
    bw = BatchedWorld(LEVELS[3], 2)
    bw.render()
    for _ in range(3):
        bw.render(atlas=_atlas("reference"))
    assert len(bw._renderers) == 2


def test_rgb_observation_and_state_share_one_frame():
    """obs_type == state_type == "rgb-image": one render launch per step serves both (the state IS the frame the observation
    broadcasts), on the default, the two-launch and the persistent step."""
    from lle_amd import rendering
    from lle_amd.env import BatchedLLE
    env = BatchedLLE.level(6).obs_type("rgb-image").state_type("rgb-image").build(8)
    obs, state = env.reset()
    assert obs.data_ptr() == state.data_ptr()
    actions = torch.full((8, 4), 4, dtype=torch.uint8, device=env.world.device)
    for kw in (dict(), dict(fused=False), dict(persistent=True)):
        out = env.step(actions, auto_reset=True, **kw)
        assert out["obs"].data_ptr() == out["state"].data_ptr(), kw
        assert torch.equal(out["obs"][:, 2].cpu(), out["state"].cpu())
    import ctypes as C
    L = rendering.lib()
    maps = (C.c_void_p * 1)(env.world.map.h)
    assert not L.lle_render_create(env.world.h, maps, 1, None, None)  # the C library has no default sprites: an atlas is required
    assert b"atlas" in L.lle_render_last_error()
