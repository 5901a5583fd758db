"""Rendering without a GPU: frame shapes, the PNG reader, rotations, the blend arithmetic of the restatement (tests/render_ref.py),
the restatement against two frames the reference's own renderer drew (tests/golden/reference_frames), the built-in sprites,
lle_map_cell_layers, the exports of liblle_render.so, the refusal without a device and the ISA tripwire on the render kernel's
translation unit.  The kernel's frames are compared on the MI355X (tests/test_gpu_render.py, tests/test_gpu_render_states.py)."""
import glob
import importlib.util
import os

import numpy as np
import pytest

from lle_amd import World, rendering
from lle_amd._capi import LLE_POS_START, Map
from tests import render_ref
from tests.parity_util import EXTRA_MAPS, LONG_MAPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPRITES = os.path.join(ROOT, "tests", "golden", "sprites")


def test_frame_shapes():
    """ref:python/tests/test_world.py:291-297 and ref:src/unit_tests/test_renderer.rs:15-24."""
    w = World("S0 . X")
    assert w.image_dimensions == (97, 33)
    assert render_ref.static_frame(render_ref.Scene.of(w._map), rendering.SpriteAtlas.builtin()).shape == (33, 97, 3)
    w6 = World.level(6)
    assert w6.image_dimensions == (417, 385)
    assert render_ref.static_frame(render_ref.Scene.of(w6._map), rendering.SpriteAtlas.builtin()).shape == (385, 417, 3)
    from lle_amd.world.rendering import TILE_SIZE  # the reference's import path (ref:python/tests/test_imports.py:27)
    assert TILE_SIZE == 32


def test_png_reader_against_pil():
    pil = pytest.importorskip("PIL.Image")
    files = sorted(glob.glob(os.path.join(SPRITES, "**", "*.png"), recursive=True))
    assert len(files) == 41
    for f in files:
        want = np.asarray(pil.open(f).convert("RGBA"))
        assert np.array_equal(rendering.read_png(f), want), f


def _png(img, filt):
    """An 8-bit RGBA PNG of `img` whose rows all use filter type `filt` (encoder for the reader's own test)."""
    import struct
    import zlib
    h, w, _ = img.shape
    bpp, raw, prev = 4, bytearray(), np.zeros(w * 4, dtype=np.int32)
    for y in range(h):
        line = img[y].reshape(-1).astype(np.int32)
        left = np.concatenate([np.zeros(bpp, np.int32), line[:-bpp]])
        upleft = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
        if filt == 0:
            f = line
        elif filt == 1:
            f = line - left
        elif filt == 2:
            f = line - prev
        elif filt == 3:
            f = line - (left + prev) // 2
        else:
            p = left + prev - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - prev), np.abs(p - upleft)
            f = line - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, upleft))
        raw += bytes([filt]) + bytes((f & 255).astype(np.uint8))
        prev = line

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(bytes(raw)))
            + chunk(b"IEND", b""))


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
def test_png_reader_every_filter(filt):
    rng = np.random.default_rng(filt)
    img = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)
    assert np.array_equal(rendering.read_png(_png(img, filt)), img)


def test_png_reader_refuses_other_formats():
    data = bytearray(_png(np.zeros((2, 2, 4), np.uint8), 0))
    data[24] = 16  # bit depth 16
    with pytest.raises(ValueError):
        rendering.read_png(bytes(data))
    with pytest.raises(ValueError):
        rendering.read_png(b"GIF89a")


def test_rotation_is_clockwise():
    """image::imageops::rotate90 turns clockwise: the top-left pixel goes to the top-right corner."""
    img = np.zeros((32, 32, 4), np.uint8)
    img[0, 0] = (1, 2, 3, 4)
    img[0, 1] = (5, 6, 7, 8)
    r = render_ref.rotate90(img)
    assert tuple(r[0, 31]) == (1, 2, 3, 4) and tuple(r[1, 31]) == (5, 6, 7, 8)
    assert np.array_equal(render_ref.rotate90(render_ref.rotate90(render_ref.rotate90(render_ref.rotate90(img)))), img)
    assert np.array_equal(render_ref.rotate90(img), np.rot90(img, k=-1))


def test_blend_hand_computed():
    """((1 - a/255) * bg + a/255 * fg) in f32, truncated: values worked out by hand in single precision."""
    cases = [  # (bg, fg, alpha, expected)
        (218, 0, 255, 0),      # opaque: the sprite
        (218, 0, 0, 218),      # transparent: the background
        (218, 0, 128, 108),    # a = 0.5019608: 0.4980392 * 218 = 108.57255 -> 108
        (100, 200, 51, 120),   # a = 0.2: 0.8 * 100 + 0.2 * 200 = 80.0 + 40.000004 = 120.000004 -> 120
        (255, 255, 200, 255),  # both 255: 254.99998 or 255.0 -> never above 255
        (10, 250, 1, 10),      # 0.99607843 * 10 + 0.003921569 * 250 = 9.960784 + 0.98039216 = 10.941176 -> 10
    ]
    for bg, fg, a, want in cases:
        got = render_ref.blend(np.array([[bg, bg, bg]], np.uint8), np.array([[fg, fg, fg, a]], np.uint8))
        assert got.tolist() == [[want] * 3], (bg, fg, a)


# Frames the reference's own renderer drew (tests/golden/README.md): its docs/3x1.png and docs/example_custom.png, the map text of
# the second from the module docstring of python/lle/__init__.py:126-132.  EXCLUDED: the cells whose sprites (agents, lasers, laser
# sources) were redrawn after the pictures were made -- a constant, never computed from where mismatches fall.
REFERENCE_FRAMES = {
    "3x1": ("S0 G X", [(0, 0)]),
    "example_custom": ("S0 . G . X\nS1 @ . . .\nL0E . . V V\n@  @ . V V\nG  . . . X", [(0, 0), (1, 0), (2, 0), (2, 1), (2, 2), (2, 3), (2, 4)]),
}


@pytest.mark.parametrize("name", sorted(REFERENCE_FRAMES))
def test_restatement_against_reference_frames(name):
    """render_ref.render of the reset state with the reference's sprites == the frame the reference shipped, red and blue swapped
    back: every grid pixel and every cell outside EXCLUDED byte for byte (floors, walls, exits, gems and voids blended over the
    floor -- real blends, truncation included).  A failure is a finding about tests/render_ref.py.  The excluded cells must differ:
    when they stop doing so the fixtures have been refreshed and the list can shrink."""
    text, excluded = REFERENCE_FRAMES[name]
    png = rendering.read_png(os.path.join(ROOT, "tests", "golden", "reference_frames", name + ".png"))
    assert (png[..., 3] == 255).all()
    ref = png[..., [2, 1, 0]]  # the files were written by a tool that expects BGR
    m = Map(text)
    scene = render_ref.Scene.of(m)
    beams = [m.reset_beam(s.laser_id, s.agent_id) & 0xFFFFFFFF for s in m.sources()]  # (beams of at most 32 cells: one word each)
    state = render_ref.State(m.positions(LLE_POS_START), 0, beams, None)
    want = render_ref.render(scene, state, rendering.SpriteAtlas.from_directory(SPRITES))
    assert ref.shape == want.shape == (32 * m.height + 1, 32 * m.width + 1, 3)
    T = render_ref.TILE_SIZE
    assert np.array_equal(ref[::T], want[::T]) and np.array_equal(ref[:, ::T], want[:, ::T]), "grid lines"
    assert (want[::T] == render_ref.GRID_GREY).all() and (want[:, ::T] == render_ref.GRID_GREY).all()
    assert set(excluded) <= {(i, j) for i in range(m.height) for j in range(m.width)}
    for i in range(m.height):
        for j in range(m.width):
            a, b = ref[T * i + 1:T * (i + 1), T * j + 1:T * (j + 1)], want[T * i + 1:T * (i + 1), T * j + 1:T * (j + 1)]
            if (i, j) in excluded:
                assert not np.array_equal(a, b), f"cell {(i, j)} equals the reference's frame now: take it off the list"
            else:
                assert np.array_equal(a, b), f"cell {(i, j)}: {int((a != b).any(axis=2).sum())} pixels differ from the reference's frame"
    assert len(excluded) == {"3x1": 1, "example_custom": 7}[name]


def test_builtin_atlas_well_formed():
    a = rendering.SpriteAtlas.builtin()
    assert a.agents.shape == (13, 32, 32, 4) and a.lasers.shape == (13, 32, 32, 4) and a.sources.shape == (13, 32, 32, 4)
    assert a.gem.shape == a.void.shape == (32, 32, 4)
    sprites = list(a.agents) + list(a.lasers) + list(a.sources) + [a.gem, a.void]
    keys = {s.tobytes() for s in sprites}
    assert len(keys) == len(sprites), "built-in sprites must be pairwise distinct"
    for s in list(a.agents) + list(a.lasers) + [a.gem, a.void]:  # partial alpha: the blend path is exercised
        alpha = s[..., 3]
        assert ((alpha > 0) & (alpha < 255)).any()
    assert rendering.SpriteAtlas.builtin() is a  # drawn once
    ref = rendering.SpriteAtlas.from_directory(SPRITES)
    assert (ref.n_agents, ref.n_lasers, ref.n_sources) == (12, 12, 12)
    assert not any(np.array_equal(x, y) for x, y in zip(a.agents, ref.agents))  # the package's own drawing


def test_from_directory_requires_contiguous_numbers(tmp_path):
    import shutil
    for fam in ("agents", "lasers", "sources"):
        shutil.copytree(os.path.join(SPRITES, fam), tmp_path / fam)
    for f in ("gem.png", "void.png"):
        shutil.copy(os.path.join(SPRITES, f), tmp_path / f)
    os.remove(tmp_path / "lasers" / "3.png")
    with pytest.raises(ValueError, match="contiguous"):
        rendering.SpriteAtlas.from_directory(str(tmp_path))


def _all_maps():
    maps = {f"level{k}": Map(level=k) for k in range(1, 7)}
    maps.update({k: Map(v) for k, v in EXTRA_MAPS.items()})
    maps.update({k: Map(v) for k, v in LONG_MAPS.items()})
    return maps


def test_cell_layers_extend_laser_tiles():
    for name, m in _all_maps().items():
        layers = m.cell_layers()
        first_two = [(c.i, c.j, c.laser_id, c.offset, c.depth, c.word, c.bit) for c in layers if c.depth < 2]
        tiles = [(t.i, t.j, t.laser_id, t.offset, t.layer, t.word, t.bit) for t in m.laser_tiles()]
        assert first_two == tiles, name
        srcs = m.sources()
        assert all(c.direction == srcs[c.laser_id].direction for c in layers), name
        assert max([c.depth for c in layers], default=-1) + 1 == (m.max_cell_layers if layers else 0), name
    four = Map(EXTRA_MAPS["four_layers"])
    at = [c for c in four.cell_layers() if (c.i, c.j) == (2, 2)]
    assert [c.depth for c in at] == [0, 1, 2, 3] and len({c.laser_id for c in at}) == 4
    assert (2, 2) in four.positions(4)  # the gem under the four beams


def test_library_exports():
    """liblle_render.so exports every function include/lle_render.h declares, and the binding knows exactly those; the header
    is plain C (a C host can include it) and is the one the library is compiled against."""
    import re
    import subprocess
    L = rendering.lib()
    header = open(os.path.join(ROOT, "include", "lle_render.h")).read()
    declared = set(re.findall(r"\b(lle_[a-z_0-9]+)\s*\(", header))
    assert declared == set(rendering.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "include", "lle_render.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert '#include "../../include/lle_render.h"' in open(os.path.join(ROOT, "lle_amd", "render", "render.hip")).read()


def test_atlas_digest_is_content():
    a, b = rendering.SpriteAtlas.from_directory(SPRITES), rendering.SpriteAtlas.from_directory(SPRITES)
    assert a is not b and a.digest == b.digest
    assert a.digest != rendering.SpriteAtlas.builtin().digest


def test_get_image_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        World("S0 . X").get_image()


def test_render_translation_unit_isa_scan():
    spec = importlib.util.spec_from_file_location("isa_exec_copy_scan", os.path.join(ROOT, "tools", "isa_exec_copy_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text = mod.asm_of(os.path.join(ROOT, "lle_amd", "render", "render.hip"))
    assert "render_kernel" in text
    assert mod.scan(text) == []
