"""What the ctypes bindings of the package share: loading a library that has no fallback, the text of a debug name function, a torch
view of device memory a handle owns, and the signatures and the argument struct every cooperation tracker library has
(include/lle_coop.h, lle_cooptrails.h, lle_coopcycles.h).  It imports no other module of the package."""
import ctypes as C
import os


def names(fn):
    """The lines a lle_*_debug_launched / lle_*_debug_compiled function writes."""
    need = fn(None, 0)
    buf = C.create_string_buffer(need)
    fn(buf, need)
    return [n for n in buf.value.decode().split("\n") if n]


def load(path, what):
    """CDLL of `path`; a missing file is an ImportError that says so: lle_amd has no fallback for `what`."""
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          f"lle_amd has no fallback for {what}.")
    return C.CDLL(path)


def device_view(ptr, shape, typestr, device):
    """A torch tensor over `ptr`, device memory that a handle owns: the array interface keeps no owner."""
    import torch

    class _Array:
        __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(_Array(), device=device)


class UpdateArgs(C.Structure):
    """lle_coop_update_args, lle_cooptrails_update_args, lle_coopcycles_update_args: one layout."""
    _fields_ = [("struct_bytes", C.c_uint32), ("ops", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32), ("env_mask", C.c_void_p)]


def tracker_signatures(L, prefix, create_argtypes, update_map_argtypes):
    """The eight functions every tracker library exports under `prefix` ("lle_coop", ...): create and update_map take what the library
    says, the other six are the same everywhere."""
    vp, i32 = C.c_void_p, C.c_int
    for name, restype, argtypes in (("create", vp, create_argtypes), ("update_map", i32, update_map_argtypes), ("free", None, [vp]),
                                    ("update", i32, [vp, C.POINTER(UpdateArgs), vp]), ("buffer", vp, [vp, i32]), ("last_error", C.c_char_p, []),
                                    ("debug_launched", C.c_size_t, [C.c_char_p, C.c_size_t]), ("debug_compiled", C.c_size_t, [C.c_char_p, C.c_size_t])):
        fn = getattr(L, f"{prefix}_{name}")
        fn.restype, fn.argtypes = restype, argtypes


def tracker_view(L, prefix, handle, which, shape, typestr, device):
    """Array `which` of a tracker handle (lle_*_buffer) as a torch view."""
    ptr = getattr(L, f"{prefix}_buffer")(handle, which)
    if not ptr:
        raise RuntimeError(f"{prefix}_buffer failed: {getattr(L, prefix + '_last_error')().decode()}")
    return device_view(ptr, shape, typestr, device)


def tracker_check(L, prefix, rc):
    if rc != 0:
        raise RuntimeError(f"lib{prefix} call failed ({rc}): {getattr(L, prefix + '_last_error')().decode()}")
