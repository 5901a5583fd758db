"""ctypes binding of liblle_policyforest.so (lle_amd/policyforest/policyforest.hip, C ABI include/lle_policyforest.h; INTEGRATION.md
section 24) and `PolicyForest`: how far from solved every environment of a batch of MANY maps is now, and what an optimal joint
action would be there.

`lle_amd.OptimalPolicy` answers for one map per handle.  A curriculum steps one batch of many generated maps
(`BatchedWorld([m0, m1, ...], n)`, map m owning the environments [m * E, (m + 1) * E)); the forest builds one steps-to-go table per
map in the same launches -- per map exactly the table OptimalPolicy builds -- and answers the whole batch in ONE launch:

    pf = PolicyForest(worlds, 12)                     # frozen at construction; equally shaped worlds, Maps or map texts
    env = BatchedWorld(worlds, len(worlds) * 256)     # the same maps in the same order, any number of environments per map
    steps = pf.steps_to_go(env)                       # int32 [n]: steps >= 0, pf.UNKNOWN (-1) or pf.DEAD_END (-2)
    actions, steps = pf.actions(env)                  # uint8 [n, A] + the same steps
    pf.act(env); env.step(env.actions)                # the experts' actions straight into the batch's action buffer: no copy
    pf.steps_to_go(World(worlds[3]), map_index=3)     # a single-map env of map 3

A map with more than `max_states_per_map` distinct states within the horizon has no table (`over_capacity[m]`, every environment of it
reads UNKNOWN); the other maps are untouched.  No fallback: a missing library raises.
"""
import ctypes as C
import os

import numpy as np

from . import _binding, _capi
from .policy import (LLE_POLICY_CAPACITY, LLE_POLICY_DEAD_END, LLE_POLICY_MAX_AGENTS, LLE_POLICY_MAX_HORIZON, LLE_POLICY_UNKNOWN, PolicyArgs, _as_map, _batched,
                     _device_index, map_fingerprint)
from .policy import lib as _policy_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_policyforest.so")

EXPORTS = ["lle_policyforest_create", "lle_policyforest_free", "lle_policyforest_build", "lle_policyforest_stats", "lle_policyforest_lookup",
           "lle_policyforest_fingerprints", "lle_policyforest_last_error", "lle_policyforest_debug_launched", "lle_policyforest_debug_compiled"]
KERNELS = ["pf_commit", "pf_expand", "pf_insert", "pf_lookup", "pf_relax", "pf_roots", "pf_seed"]


class PolicyForestOptions(C.Structure):
    """lle_policyforest_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("envs_per_map", C.c_int64), ("max_states_per_map", C.c_int64), ("stream", C.c_void_p)]


class PolicyForestMapResult(C.Structure):
    """lle_policyforest_result."""
    _fields_ = [("status", C.c_int32), ("depth_reached", C.c_int32), ("n_states", C.c_int64), ("complete", C.c_int32), ("root_steps", C.c_int32),
                ("passes", C.c_int32), ("pad", C.c_int32)]


class PolicyForestSummary(C.Structure):
    """lle_policyforest_summary."""
    _fields_ = [("struct_bytes", C.c_uint32), ("pad", C.c_int32), ("step_errors", C.c_int64), ("explore_ms", C.c_double), ("relax_ms", C.c_double),
                ("explore_items", C.c_int64), ("explore_lanes", C.c_int64), ("relax_items", C.c_int64), ("relax_lanes", C.c_int64)]


_lib = None


def lib():
    """Load liblle_policyforest.so (after liblle_hip.so and liblle_policy.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _policy_lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the forest of steps-to-go tables.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_policyforest_create.restype = vp
    L.lle_policyforest_create.argtypes = [C.POINTER(vp), i32, C.POINTER(PolicyForestOptions)]
    L.lle_policyforest_free.restype = None
    L.lle_policyforest_free.argtypes = [vp]
    L.lle_policyforest_build.restype = i32
    L.lle_policyforest_build.argtypes = [vp, C.POINTER(PolicyArgs), C.POINTER(PolicyForestMapResult), C.POINTER(PolicyForestSummary)]
    L.lle_policyforest_stats.restype = i32
    L.lle_policyforest_stats.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_policyforest_lookup.restype = i32
    L.lle_policyforest_lookup.argtypes = [vp, vp, i32, vp, vp, C.c_int64, vp]
    L.lle_policyforest_fingerprints.restype = i32
    L.lle_policyforest_fingerprints.argtypes = [vp, C.POINTER(C.c_uint64), i32]
    L.lle_policyforest_last_error.restype = C.c_char_p
    L.lle_policyforest_last_error.argtypes = []
    for fn in (L.lle_policyforest_debug_launched, L.lle_policyforest_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_policyforest.so this process has launched (lle_policyforest_debug_launched)."""
    return _binding.names(lib().lle_policyforest_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_policyforest_debug_compiled)."""
    return _binding.names(lib().lle_policyforest_debug_compiled)


class PolicyForest:
    """One steps-to-go table per world up to `horizon` levels ("auto": (width * height) // 2, as OptimalPolicy), built together.

    `worlds`: lle_amd.Worlds, Maps or map texts of one shape (what lle_batch_create_multi wants the maps of a batch to agree on;
    ValueError with the library's message otherwise).  FROZEN at construction, like OptimalPolicy: the forest keeps its own copies of the
    maps as they are now and their fingerprints, and the tables are built right here.  `collect_gems`: a goal also has every gem
    collected.  `envs_per_map`: environments per map of the build's own batch = work items of a map per piece;
    `max_states_per_map`: records of every map's pool segment.

    Arrays over the maps: n_states, complete (the map's frontier ran empty: every answer of it is exact), depth_reached, root_steps
    (int32: steps from the reset state, UNKNOWN or DEAD_END), status, over_capacity (the map met more states than max_states_per_map:
    no table, UNKNOWN everywhere), passes (relaxation passes the map took part in; depends on scheduling).  `stats(m)`: frontier /
    expanded per depth of map m; `occupancy`: lanes that served a work item over lanes launched, per phase; `explore_ms`, `relax_ms`.

    Every lookup takes `env`: a BatchedWorld or BatchedLLE that holds the forest's maps in the forest's order, with any number of
    environments per map, on the forest's device -- or, with `map_index=m`, a single-map BatchedWorld, BatchedLLE or World of map m.
    It compares the env's map fingerprints with the forest's, all of them or the one (`check_map=False` skips that: the caller
    vouches for the maps), and refuses an env with per-environment sources or another number of maps with ValueError."""

    UNKNOWN = LLE_POLICY_UNKNOWN
    DEAD_END = LLE_POLICY_DEAD_END

    def __init__(self, worlds, horizon="auto", *, collect_gems=False, envs_per_map=256, max_states_per_map=1 << 16, device=None):
        from .world import World
        worlds = list(worlds)
        if not worlds:
            raise ValueError("a forest needs at least one world")
        sources = [_as_map(w) for w in worlds]
        first = sources[0]
        self.horizon = self._horizon(horizon, first)
        if int(envs_per_map) < 1 or int(max_states_per_map) < 1:
            raise ValueError("envs_per_map and max_states_per_map must be at least 1")
        if first.n_agents > LLE_POLICY_MAX_AGENTS:
            raise ValueError(f"the tables serve maps of at most {LLE_POLICY_MAX_AGENTS} agents (5^A joint actions per state); map 0 has {first.n_agents}")
        for k, w in enumerate(worlds):
            batch = getattr(w, "_batch_obj", None) if isinstance(w, World) else None
            if batch is not None and getattr(batch, "_env_sources", False):
                raise ValueError(f"map {k} keeps per-environment sources: the tables are built on the map's own source colours and flags")
        self.collect_gems, self.envs_per_map, self.max_states_per_map = bool(collect_gems), int(envs_per_map), int(max_states_per_map)
        self.maps = [m.clone() for m in sources]  # frozen: later changes of the worlds do not reach this forest
        self.n_maps, self.n_agents = len(self.maps), first.n_agents
        L = lib()
        opt = PolicyForestOptions(C.sizeof(PolicyForestOptions), _device_index(device if device is not None else getattr(worlds[0], "_device", None)),
                                  self.envs_per_map, self.max_states_per_map, None)
        handles = (C.c_void_p * self.n_maps)(*[m.h for m in self.maps])
        self.h = L.lle_policyforest_create(handles, self.n_maps, C.byref(opt))
        if not self.h:
            message = L.lle_policyforest_last_error().decode()
            raise (ValueError if "lle_batch_create_multi" in message or "must be" in message else RuntimeError)(f"lle_policyforest_create failed: {message}")
        kept = (C.c_uint64 * self.n_maps)()
        L.lle_policyforest_fingerprints(self.h, kept, self.n_maps)
        self.fingerprints = [int(v) for v in kept]  # lle_policy_map_fingerprint of every map, as the handle keeps them
        self._lookup = L.lle_policyforest_lookup
        self._build()

    @staticmethod
    def _horizon(horizon, first):
        value = (first.width * first.height) // 2 if isinstance(horizon, str) and horizon == "auto" else int(horizon)
        if not 0 <= value <= LLE_POLICY_MAX_HORIZON:
            raise ValueError(f"horizon must be 0 .. {LLE_POLICY_MAX_HORIZON}, got {value}.")
        return value

    def _build(self):
        L, M = lib(), self.n_maps
        args = PolicyArgs(C.sizeof(PolicyArgs), int(self.collect_gems), self.horizon, 0)
        res = (PolicyForestMapResult * M)()
        summary = PolicyForestSummary(C.sizeof(PolicyForestSummary))
        rc = L.lle_policyforest_build(self.h, C.byref(args), res, C.byref(summary))
        if rc != 0:
            raise RuntimeError(f"lle_policyforest_build failed ({rc}): {L.lle_policyforest_last_error().decode()}")
        self.status = np.array([r.status for r in res], dtype=np.int32)
        self.over_capacity = self.status == LLE_POLICY_CAPACITY
        self.n_states = np.array([r.n_states for r in res], dtype=np.int64)
        self.complete = np.array([bool(r.complete) for r in res], dtype=bool)
        self.depth_reached = np.array([r.depth_reached for r in res], dtype=np.int32)
        self.root_steps = np.array([r.root_steps for r in res], dtype=np.int32)
        self.passes = np.array([r.passes for r in res], dtype=np.int32)
        self.explore_ms, self.relax_ms = float(summary.explore_ms), float(summary.relax_ms)
        self.occupancy = dict(explore_items=int(summary.explore_items), explore_lanes=int(summary.explore_lanes), relax_items=int(summary.relax_items),
                              relax_lanes=int(summary.relax_lanes),
                              explore=summary.explore_items / summary.explore_lanes if summary.explore_lanes else 0.0,
                              relax=summary.relax_items / summary.relax_lanes if summary.relax_lanes else 0.0)

    def rebuild(self, horizon=None, collect_gems=None):
        """Builds every table again under another horizon and / or collect_gems; the new tables replace the old ones."""
        self._alive()
        if horizon is not None:
            self.horizon = self._horizon(horizon, self.maps[0])
        if collect_gems is not None:
            self.collect_gems = bool(collect_gems)
        self._build()
        return self

    def stats(self, m):
        """dict(frontier=[...], expanded=[...]) of map m: states first reached at depth d, available joint actions over the states of depth d."""
        self._alive()
        if not 0 <= int(m) < self.n_maps:
            raise IndexError(f"no map {m}: the forest holds {self.n_maps}")
        cap = int(self.depth_reached[m]) + 2
        frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
        n = lib().lle_policyforest_stats(self.h, int(m), frontier, expanded, cap)
        return dict(frontier=[int(frontier[d]) for d in range(n)], expanded=[int(expanded[d]) for d in range(n - 1)])

    def _alive(self):
        if not getattr(self, "h", None):
            raise RuntimeError("the forest has been freed")

    # ---- the env a lookup reads
    def _world_of(self, env, check_map, map_index):
        self._alive()
        w = _batched(env)
        if not hasattr(w, "h") or not hasattr(w, "maps"):
            raise TypeError(f"expected a BatchedWorld, a BatchedLLE or a World, got {type(env).__name__}")
        if map_index is None:
            index, own = -1, self.fingerprints
            if len(w.maps) != self.n_maps:
                raise ValueError(f"the env holds {len(w.maps)} maps, the forest {self.n_maps}: pass the forest's maps in its order, or map_index for a single-map env")
        else:
            index = int(map_index)
            if not 0 <= index < self.n_maps:
                raise ValueError(f"map_index must be 0 .. {self.n_maps - 1}, got {index}")
            own = [self.fingerprints[index]]
            if len(w.maps) != 1:
                raise ValueError(f"the env holds {len(w.maps)} maps: map_index asks for an env of that map alone")
        if getattr(w, "_env_sources", False):
            raise ValueError("the env keeps per-environment sources: the tables are built on the maps' own source colours and flags")
        if w.map.n_agents != self.n_agents:
            raise ValueError(f"the env's maps have {w.map.n_agents} agents, the forest's {self.n_agents}")
        if check_map:
            for k, (m, want) in enumerate(zip(w.maps, own)):
                if map_fingerprint(m) != want:
                    raise ValueError(f"map {k} of the env is not map {k if index < 0 else index} of the forest (lle_policy_map_fingerprint differs): build a "
                                     "PolicyForest for the env's maps, or pass check_map=False to vouch for them")
        return w, index

    def _call(self, w, index, steps, actions_ptr, action_stride):
        rc = self._lookup(self.h, w.h, index, steps.data_ptr(), actions_ptr, action_stride, w._stream())
        if rc != 0:
            message = lib().lle_policyforest_last_error().decode()
            raise (ValueError if rc == -2 else RuntimeError)(f"lle_policyforest_lookup failed ({rc}): {message}")

    @staticmethod
    def _steps(w, out):
        import torch
        if out is None:
            return torch.empty(w.n_envs, dtype=torch.int32, device=w.device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != w.device or tuple(out.shape) != (w.n_envs,) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int32 tensor of shape ({w.n_envs},) on {w.device}")
        return out

    def steps_to_go(self, env, check_map=True, out=None, map_index=None):
        """int32 [n] on the env's device: the length of the shortest plan from every environment's current state in its own map,
        UNKNOWN or DEAD_END.  `out`: the tensor to write into (a hot loop allocates nothing)."""
        w, index = self._world_of(env, check_map, map_index)
        steps = self._steps(w, out)
        self._call(w, index, steps, None, 0)
        return steps

    def actions(self, env, check_map=True, out=None, map_index=None):
        """(uint8 [n, A], int32 [n]): an optimal joint action of every environment -- among the shortest, the one with the smallest
        base-5 code, agent 0 the lowest digit -- and steps_to_go; all STAY where steps is negative."""
        import torch
        w, index = self._world_of(env, check_map, map_index)
        steps = self._steps(w, out)
        actions = torch.empty((w.n_envs, self.n_agents), dtype=torch.uint8, device=w.device)
        self._call(w, index, steps, actions.data_ptr(), self.n_agents)
        return actions, steps

    def act(self, env, check_map=True, out=None, map_index=None):
        """Writes the actions into the env's own action buffer (`BatchedWorld.actions`) and returns steps_to_go (in `out` when given):
        `env.step(env.actions)` then takes them without a copy.  Nothing else of the env is written."""
        w, index = self._world_of(env, check_map, map_index)
        steps = self._steps(w, out)
        self._call(w, index, steps, w.actions.data_ptr(), int(w.actions.stride(0)))
        return steps

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_policyforest_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()


__all__ = ["PolicyForest"]
