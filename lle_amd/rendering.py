"""Rendering: the reference's `World.get_image` (src/rendering/renderer.rs, sprites.rs; pyworld.rs:518-524) for whole batches.

The frames come from the HIP kernel of liblle_render.so (lle_amd/render/render.hip, C ABI include/lle_render.h):
one launch writes the (32 H + 1, 32 W + 1, 3) frame of every selected environment in the reference's layout, draw order and
float32 blend arithmetic.  This module holds the sprites (`SpriteAtlas`) and the ctypes binding (`Renderer`); the public entry
points are `BatchedWorld.render`, `World.get_image`, the "rgb-image" observation and `BatchedLLE.get_image`.

Two differences from the reference's frames.  The reference ships its sprites as PNG files compiled into the binary
(build.rs:8-150); this package draws its own set with numpy (`SpriteAtlas.builtin()`, the default) -- same tile size, grid, layer
order and arithmetic, other pixels.  `SpriteAtlas.from_directory(path)` reads the reference's own directory layout, and with it the
frames are the reference's pixels.  And the reference's PyWorld draws its exits once, at construction (pyworld.rs:86, 203-209);
here the frame follows `exit_pos` changes.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np

from . import _capi

TILE_SIZE = 32  # src/rendering/mod.rs:8
BACKGROUND_GREY = (218, 218, 218)  # mod.rs:9
GRID_GREY = (127, 127, 127)  # mod.rs:10

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_render.so")

# enum of render.hip
LLE_RENDER_U8, LLE_RENDER_F16, LLE_RENDER_BF16, LLE_RENDER_F32 = 0, 1, 2, 3
LLE_RENDER_ENV_SOURCES = 1

EXPORTS = ["lle_render_create", "lle_render_update_map", "lle_render_free", "lle_render_desc_of", "lle_render_frame",
           "lle_render_last_error", "lle_render_debug_launched"]


# ------------------------------------------------------------------------------------------------ PNG
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def read_png(source):
    """Decode an 8-bit RGB or RGBA, non-interlaced PNG (a path or the file's bytes) into uint8 (H, W, 4); RGB gets alpha 255 (what
    `to_rgba8` gives, sprites.rs:10-19).  All five row filters.  Anything else raises ValueError."""
    data = source if isinstance(source, (bytes, bytearray)) else open(source, "rb").read()
    if data[:8] != _PNG_SIGNATURE:
        raise ValueError("not a PNG file")
    pos, header, idat = 8, None, []
    while pos + 8 <= len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        pos += 12 + length
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if header is None:
        raise ValueError("PNG without IHDR")
    width, height, depth, colour, compression, filt, interlace = header
    if depth != 8 or colour not in (2, 6) or compression != 0 or filt != 0 or interlace != 0:
        raise ValueError(f"unsupported PNG: bit depth {depth}, colour type {colour}, interlace {interlace} (8-bit RGB / RGBA, non-interlaced only)")
    bpp = 3 if colour == 2 else 4
    stride = width * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != height * (stride + 1):
        raise ValueError("truncated PNG image data")
    out = np.zeros((height, stride), dtype=np.uint8)
    prev = bytearray(stride)
    for y in range(height):
        ftype = raw[y * (stride + 1)]
        line = bytearray(raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        if ftype == 1:
            for i in range(bpp, stride):
                line[i] = (line[i] + line[i - bpp]) & 255
        elif ftype == 2:
            for i in range(stride):
                line[i] = (line[i] + prev[i]) & 255
        elif ftype == 3:
            for i in range(stride):
                left = line[i - bpp] if i >= bpp else 0
                line[i] = (line[i] + ((left + prev[i]) >> 1)) & 255
        elif ftype == 4:
            for i in range(stride):
                a = line[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                line[i] = (line[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
        elif ftype != 0:
            raise ValueError(f"bad PNG filter type {ftype}")
        out[y] = np.frombuffer(bytes(line), dtype=np.uint8)
        prev = line
    img = out.reshape(height, width, bpp)
    if bpp == 3:
        img = np.concatenate([img, np.full((height, width, 1), 255, dtype=np.uint8)], axis=2)
    return img


# ------------------------------------------------------------------------------------------------ sprites
# 12 numbered colours (agents, lasers, sources 0..11) and the fallback's, this package's own palette
_PALETTE = np.array([(214, 39, 40), (31, 119, 180), (44, 160, 44), (255, 187, 34), (148, 103, 189), (23, 190, 207),
                     (255, 127, 14), (227, 119, 194), (140, 86, 75), (188, 189, 34), (0, 0, 128), (0, 128, 128)], dtype=np.int32)
_FALLBACK = np.array((96, 96, 96), dtype=np.int32)


def _canvas():
    return np.zeros((TILE_SIZE, TILE_SIZE, 4), dtype=np.uint8)


def _yx():
    y, x = np.mgrid[0:TILE_SIZE, 0:TILE_SIZE]
    return y.astype(np.float64) + 0.5, x.astype(np.float64) + 0.5


def _agent_sprite(rgb, marks):
    """A disc with a soft rim (partial alpha) and `marks` white pips along its top: agent k carries k % 4 + 1 of them."""
    y, x = _yx()
    r = np.hypot(y - 17.0, x - 16.0)
    alpha = np.clip((12.5 - r) * 96.0, 0, 230)
    img = _canvas()
    img[..., :3] = np.asarray(rgb, dtype=np.uint8)
    img[..., 3] = alpha.astype(np.uint8)
    for m in range(marks):
        cy, cx = 12, 10 + 4 * m
        img[cy - 1:cy + 1, cx - 1:cx + 1, :3] = 255
    img[20:22, 14:18, :3] = 0  # a mouth: no symmetry, so a rotation would show
    return img


def _laser_sprite(rgb):
    """A horizontal beam: a band across the tile whose alpha falls off from its core."""
    img = _canvas()
    img[..., :3] = np.asarray(rgb, dtype=np.uint8)
    profile = {12: 40, 13: 100, 14: 190, 15: 235, 16: 235, 17: 190, 18: 100, 19: 40}
    for row, a in profile.items():
        img[row, :, 3] = a
    img[15:17, :, :3] = np.minimum(255, np.asarray(rgb, dtype=np.int32) + 80).astype(np.uint8)
    return img


def _source_sprite(rgb):
    """An east-facing emitter: a dark housing with an arrow of the beam's colour pointing east (opaque: sources are RGB)."""
    img = _canvas()
    img[..., :3] = 64
    img[2:30, 2:30, :3] = 40
    y, x = _yx()
    arrow = (x > 8) & (x < 27) & (np.abs(y - 16.0) < (27 - x) * 0.6)
    img[arrow, :3] = np.asarray(rgb, dtype=np.uint8)
    img[..., 3] = 255
    return img


def _gem_sprite():
    y, x = _yx()
    d = np.abs(y - 16.0) / 11.0 + np.abs(x - 16.0) / 9.0
    img = _canvas()
    img[..., 0], img[..., 1], img[..., 2] = 20, 200, 130
    img[..., 3] = np.clip((1.0 - d) * 600.0, 0, 210).astype(np.uint8)
    img[9:13, 13:16, :3] = 240  # a highlight, upper left
    return img


def _void_sprite():
    y, x = _yx()
    r = np.hypot(y - 16.0, x - 16.0)
    img = _canvas()
    img[..., :3] = 16
    img[..., 3] = np.clip(250.0 - r * 9.0, 60, 250).astype(np.uint8)
    return img


class SpriteAtlas:
    """The sprites of a renderer, in the families of the reference (sprites.rs:56-91; build.rs:63-150): each of `agents`, `lasers`
    (horizontal) and `sources` (facing east, drawn opaque) is uint8 [n + 1, 32, 32, 4] -- n numbered sprites and the fallback
    (`n.png`) last --; `gem` and `void` are [32, 32, 4].  Vertical lasers and the other source directions are clockwise rotations
    of these, made by the renderer (build.rs:84-93, 106-151)."""

    def __init__(self, agents, lasers, sources, gem, void):
        fams = [np.ascontiguousarray(a, dtype=np.uint8) for a in (agents, lasers, sources)]
        for name, a in zip(("agents", "lasers", "sources"), fams):
            if a.ndim != 4 or a.shape[1:] != (TILE_SIZE, TILE_SIZE, 4) or a.shape[0] < 2:
                raise ValueError(f"{name}: [n + 1, 32, 32, 4] with at least one numbered sprite and the fallback, got {a.shape}")
        self.agents, self.lasers, self.sources = fams
        self.gem, self.void = (np.ascontiguousarray(a, dtype=np.uint8) for a in (gem, void))
        for name, a in (("gem", self.gem), ("void", self.void)):
            if a.shape != (TILE_SIZE, TILE_SIZE, 4):
                raise ValueError(f"{name}: [32, 32, 4], got {a.shape}")
        self._digest = None

    @property
    def digest(self):
        """A hash of the sprites (families, counts and pixels): BatchedWorld keeps one renderer per distinct atlas CONTENT."""
        if self._digest is None:
            import hashlib
            h = hashlib.sha256()
            for a in (self.agents, self.lasers, self.sources, self.gem, self.void):
                h.update(repr(a.shape).encode())
                h.update(a.tobytes())
            self._digest = h.hexdigest()
        return self._digest

    @property
    def n_agents(self):
        return self.agents.shape[0] - 1

    @property
    def n_lasers(self):
        return self.lasers.shape[0] - 1

    @property
    def n_sources(self):
        return self.sources.shape[0] - 1

    @classmethod
    def builtin(cls):
        """This package's own sprites (drawn here, deterministic): agents, lasers and sources 0..11 plus fallbacks, a gem, a void."""
        global _BUILTIN
        if _BUILTIN is None:
            cols = list(_PALETTE) + [_FALLBACK]
            agents = np.stack([_agent_sprite(c, k % 4 + 1) for k, c in enumerate(cols[:-1])] + [_agent_sprite(_FALLBACK, 0)])
            lasers = np.stack([_laser_sprite(c) for c in cols])
            sources = np.stack([_source_sprite(c) for c in cols])
            _BUILTIN = cls(agents, lasers, sources, _gem_sprite(), _void_sprite())
        return _BUILTIN

    @classmethod
    def from_directory(cls, path):
        """The reference's layout (resources/sprites): agents/k.png, lasers/k.png, sources/k.png -- numbered from 0 without a gap
        (build.rs:8-31) -- each with n.png as the fallback, plus gem.png and void.png."""
        def family(name):
            d = os.path.join(path, name)
            numbered = {}
            for f in os.listdir(d):
                stem, ext = os.path.splitext(f)
                if ext == ".png" and stem.isdigit():
                    numbered[int(stem)] = os.path.join(d, f)
            if not numbered:
                raise ValueError(f"{d}: at least one numbered sprite is required")
            for k in range(len(numbered)):
                if k not in numbered:
                    raise ValueError(f"numbered sprites in {d} must be contiguous from 0; missing {k}")
            files = [numbered[k] for k in range(len(numbered))] + [os.path.join(d, "n.png")]
            return np.stack([read_png(f) for f in files])
        return cls(family("agents"), family("lasers"), family("sources"), read_png(os.path.join(path, "gem.png")),
                   read_png(os.path.join(path, "void.png")))


_BUILTIN = None


# ------------------------------------------------------------------------------------------------ C ABI
class RenderAtlas(C.Structure):
    """lle_render_atlas (render.hip)."""
    _fields_ = [("n_agents", C.c_int32), ("n_lasers", C.c_int32), ("n_sources", C.c_int32), ("pad", C.c_int32),
                ("agents", C.c_void_p), ("lasers", C.c_void_p), ("sources", C.c_void_p), ("gem", C.c_void_p), ("void_", C.c_void_p)]


class RenderDesc(C.Structure):
    """lle_render_desc (render.hip)."""
    _fields_ = [("elem_bytes", C.c_int32), ("ndim", C.c_int32), ("shape", C.c_int64 * 4), ("stride", C.c_int64 * 4), ("bytes", C.c_int64)]


_lib = None


def lib():
    """Load liblle_render.so (after liblle_hip.so, which it links against).  No fallback: a missing library raises."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback renderer.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.lle_render_create.restype = vp
    L.lle_render_create.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(RenderAtlas), vp]
    L.lle_render_update_map.restype = i32
    L.lle_render_update_map.argtypes = [vp, i32, vp, vp]
    L.lle_render_free.restype = None
    L.lle_render_free.argtypes = [vp]
    L.lle_render_desc_of.restype = i32
    L.lle_render_desc_of.argtypes = [vp, i64, i32, C.POINTER(RenderDesc)]
    L.lle_render_frame.restype = i32
    L.lle_render_frame.argtypes = [vp, vp, i64, C.c_uint32, i32, vp, i64, vp]
    L.lle_render_last_error.restype = C.c_char_p
    L.lle_render_last_error.argtypes = []
    L.lle_render_debug_launched.restype = C.c_size_t
    L.lle_render_debug_launched.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_render.so this process has launched (lle_render_debug_launched)."""
    fn = lib().lle_render_debug_launched
    need = fn(None, 0)
    buf = C.create_string_buffer(need)
    fn(buf, need)
    return [n for n in buf.value.decode().split("\n") if n]


class Renderer:
    """One lle_renderer over a BatchedWorld: the static tiles and draw tables of its maps, uploaded once (lle_render_create)."""

    def __init__(self, batch, atlas=None):
        self.atlas = atlas if atlas is not None else SpriteAtlas.builtin()
        a = self.atlas
        st = RenderAtlas(a.n_agents, a.n_lasers, a.n_sources, 0, a.agents.ctypes.data, a.lasers.ctypes.data, a.sources.ctypes.data,
                         a.gem.ctypes.data, a.void.ctypes.data)
        handles = (C.c_void_p * len(batch.maps))(*[m.h for m in batch.maps])
        self.h = lib().lle_render_create(batch.h, handles, len(batch.maps), C.byref(st), batch._stream())
        if not self.h:
            raise RuntimeError(f"lle_render_create failed: {lib().lle_render_last_error().decode()}")

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"liblle_render call failed ({rc}): {lib().lle_render_last_error().decode()}")

    def update_map(self, map_index, map_, stream):
        self._check(lib().lle_render_update_map(self.h, int(map_index), map_.h, stream))

    def desc(self, n_sel, dtype):
        d = RenderDesc()
        self._check(lib().lle_render_desc_of(self.h, int(n_sel), int(dtype), C.byref(d)))
        return d

    def frame(self, env_ids_ptr, n_sel, flags, dtype, out_ptr, out_bytes, stream):
        self._check(lib().lle_render_frame(self.h, env_ids_ptr, int(n_sel), int(flags), int(dtype), out_ptr, int(out_bytes), stream))

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_render_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()
