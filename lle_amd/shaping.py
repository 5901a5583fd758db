"""ctypes binding of liblle_shaping.so (lle_amd/shaping/shaping.hip, C ABI include/lle_shaping.h):
potential-based reward shaping (PotentialShapedLLE, python/lle/env/reward_strategy.py:112-181) and the LaserSubgoal extras
(python/lle/env/extras_generators.py:75-101) for whole batches, one launch per step.

The public entry points are the descriptors of lle_amd/env.py (`PotentialShapedLLE`, `LaserSubgoal`, ...) handed to `BatchedLLE`;
this module is loaded only when one of them is.  No fallback: a missing library raises.

The sources of the library are in the DIRECTORY lle_amd/shaping/ (shaping.hip, Makefile), next to this module of the same name.  That
directory must never get an `__init__.py`: `import lle_amd.shaping` resolves to this file because a regular module wins over a
namespace package, and a package of that name would shadow the binding (the renderer pairs rendering.py with render/ instead).
"""
import ctypes as C
import os

from . import _binding, _capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_shaping.so")

# enums of include/lle_shaping.h
LLE_SHAPING_CLEAR, LLE_SHAPING_MARK_STARTS, LLE_SHAPING_MARK_POS = 1, 2, 4
LLE_SHAPING_HONOUR_AUTO_RESET = 1
LLE_SHAPING_MAX_COLS, LLE_SHAPING_MAX_REPEATS = 64, 8

EXPORTS = ["lle_shaping_cell_masks", "lle_shaping_create", "lle_shaping_update_map", "lle_shaping_free", "lle_shaping_update",
           "lle_shaping_reached", "lle_shaping_last_error", "lle_shaping_debug_launched", "lle_shaping_debug_compiled"]


class ShapingConfig(C.Structure):
    """lle_shaping_config."""
    _fields_ = [("struct_bytes", C.c_uint32), ("n_pbrs_cols", C.c_int32), ("pbrs_cols", C.POINTER(C.c_int32)), ("n_extras_cols", C.c_int32),
                ("pad", C.c_int32), ("extras_cols", C.POINTER(C.c_int32)), ("gamma", C.c_double), ("reward_value", C.c_double)]


class UpdateArgs(C.Structure):
    """lle_shaping_update_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("strategy_ops", C.c_uint32), ("extras_ops", C.c_uint32), ("flags", C.c_uint32),
                ("reward_kind", C.c_int32), ("pad", C.c_int32), ("env_mask", C.c_void_p), ("base_reward", C.c_void_p),
                ("reward_out", C.c_void_p), ("extras_out", C.c_void_p)]


_lib = None


def lib():
    """Load liblle_shaping.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for reward shaping.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_shaping_cell_masks.restype = i32
    L.lle_shaping_cell_masks.argtypes = [vp, C.POINTER(C.c_uint32), i32]
    L.lle_shaping_create.restype = vp
    L.lle_shaping_create.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(ShapingConfig), vp]
    L.lle_shaping_update_map.restype = i32
    L.lle_shaping_update_map.argtypes = [vp, i32, vp, vp]
    L.lle_shaping_free.restype = None
    L.lle_shaping_free.argtypes = [vp]
    L.lle_shaping_update.restype = i32
    L.lle_shaping_update.argtypes = [vp, C.POINTER(UpdateArgs), vp]
    L.lle_shaping_reached.restype = vp
    L.lle_shaping_reached.argtypes = [vp, i32]
    L.lle_shaping_last_error.restype = C.c_char_p
    L.lle_shaping_last_error.argtypes = []
    for fn in (L.lle_shaping_debug_launched, L.lle_shaping_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_shaping.so this process has launched (lle_shaping_debug_launched)."""
    return _binding.names(lib().lle_shaping_debug_launched)


def compiled_kernels():
    """Every instantiation the library holds (lle_shaping_debug_compiled)."""
    return _binding.names(lib().lle_shaping_debug_compiled)


def cell_masks(map_):
    """The cell table of a Map (lle_shaping_cell_masks; host only): a list of height * width integers, bit l of entry i * width + j
    set when source laser_id l owns a laser tile on (i, j) in the sense of World.lasers (the outer two layers of a cell)."""
    L = lib()
    n = L.lle_shaping_cell_masks(map_.h, None, 0)
    if n < 0:
        raise RuntimeError(f"lle_shaping_cell_masks failed: {L.lle_shaping_last_error().decode()}")
    buf = (C.c_uint32 * max(n, 1))()
    L.lle_shaping_cell_masks(map_.h, buf, n)
    return [int(buf[k]) for k in range(n)]


class Shaping:
    """One lle_shaping over a BatchedWorld: the cell tables of its maps and the two reached arrays (lle_shaping_create)."""

    def __init__(self, batch, pbrs_cols, extras_cols, gamma, reward_value):
        L = lib()
        self.pbrs_cols, self.extras_cols = [int(c) for c in pbrs_cols], [int(c) for c in extras_cols]
        pc = (C.c_int32 * max(len(self.pbrs_cols), 1))(*self.pbrs_cols)
        ec = (C.c_int32 * max(len(self.extras_cols), 1))(*self.extras_cols)
        cfg = ShapingConfig(C.sizeof(ShapingConfig), len(self.pbrs_cols), pc, len(self.extras_cols), 0, ec, float(gamma), float(reward_value))
        handles = (C.c_void_p * len(batch.maps))(*[m.h for m in batch.maps])
        self.h = L.lle_shaping_create(batch.h, handles, len(batch.maps), C.byref(cfg), batch._stream())
        if not self.h:
            raise RuntimeError(f"lle_shaping_create failed: {L.lle_shaping_last_error().decode()}")
        self._update = L.lle_shaping_update
        self._device, self._shape = batch.device, (int(batch.n_envs), int(batch.map.n_agents))

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"liblle_shaping call failed ({rc}): {lib().lle_shaping_last_error().decode()}")

    @staticmethod
    def make_args(strategy_ops=0, extras_ops=0, flags=0, reward_kind=0, env_mask=None, base_reward=None, reward_out=None, extras_out=None):
        """An lle_shaping_update_args over device tensors (None = not wanted); the caller keeps the tensors alive."""
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return UpdateArgs(C.sizeof(UpdateArgs), int(strategy_ops), int(extras_ops), int(flags), int(reward_kind), 0, ptr(env_mask),
                          ptr(base_reward), ptr(reward_out), ptr(extras_out))

    def update(self, args, stream):
        rc = self._update(self.h, C.byref(args), stream)
        if rc != 0:
            self._check(rc)

    def update_map(self, map_index, map_, stream):
        self._check(lib().lle_shaping_update_map(self.h, int(map_index), map_.h, stream))

    def reached_ptr(self, which):
        return lib().lle_shaping_reached(self.h, int(which))

    def reached(self, which):
        """The device array behind lle_shaping_reached as a torch tensor, int32 [n_envs, A] (the bits of the u32 words): a VIEW of the
        handle's memory, not a copy -- writes land in the state the next update reads.  which: 0 reward strategy, 1 extras generator.
        Valid until free()."""
        import torch
        ptr = self.reached_ptr(which)
        if not ptr:
            raise RuntimeError(f"lle_shaping_reached failed: {lib().lle_shaping_last_error().decode()}")

        class _Words:  # (the array interface keeps no owner: the handle owns the memory)
            __cuda_array_interface__ = {"shape": self._shape, "typestr": "<i4", "data": (int(ptr), False), "version": 2, "strides": None}
        return torch.as_tensor(_Words(), device=self._device)

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_shaping_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()
