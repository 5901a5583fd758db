"""ctypes binding of liblle_policy.so (lle_amd/policy/policy.hip, C ABI include/lle_policy.h) and
`OptimalPolicy`: how far from solved every environment of a batch is now, and what an optimal joint action would be there.

The table is built once per map by exhaustive search through the step kernel itself (explore every reachable state up to the horizon,
then relax the distances backwards from the goal states), so the answers are exact with respect to `World.step`.  A lookup is one
kernel launch over the batch, a lane per environment:

    pol = OptimalPolicy(Map(level=3))                 # frozen at construction, like Solver
    env = BatchedWorld(Map(level=3), 65536)
    steps = pol.steps_to_go(env)                      # int32 [n]: steps >= 0, pol.UNKNOWN (-1) or pol.DEAD_END (-2)
    actions, steps = pol.actions(env)                 # uint8 [n, A] + the same steps
    pol.act(env); env.step(env.actions)               # the expert's actions straight into the batch's action buffer: no copy

UNKNOWN: the state is not in the table, or the table stopped at the horizon before its value could be proved shortest.  DEAD_END: an
agent is dead, or the table is complete and no goal can be reached from the state.  For both every agent's action is STAY.

The module is loaded only when a policy is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _binding, _capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_policy.so")

# include/lle_policy.h
LLE_POLICY_CAPACITY = -20
LLE_POLICY_UNKNOWN, LLE_POLICY_DEAD_END = -1, -2
LLE_POLICY_MAX_AGENTS = 6
LLE_POLICY_MAX_HORIZON = 32767

EXPORTS = ["lle_policy_create", "lle_policy_free", "lle_policy_build", "lle_policy_stats", "lle_policy_lookup", "lle_policy_map_fingerprint",
           "lle_policy_last_error", "lle_policy_debug_launched", "lle_policy_debug_compiled"]


class PolicyOptions(C.Structure):
    """lle_policy_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("chunk", C.c_int64), ("max_states", C.c_int64), ("stream", C.c_void_p)]


class PolicyArgs(C.Structure):
    """lle_policy_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("collect_gems", C.c_int32), ("horizon", C.c_int32), ("pad", C.c_int32)]


class PolicyResult(C.Structure):
    """lle_policy_result."""
    _fields_ = [("struct_bytes", C.c_uint32), ("depth_reached", C.c_int32), ("n_states", C.c_int64), ("complete", C.c_int32), ("passes", C.c_int32),
                ("root_steps", C.c_int32), ("pad", C.c_int32), ("step_errors", C.c_int64), ("explore_ms", C.c_double), ("relax_ms", C.c_double)]


_lib = None


def lib():
    """Load liblle_policy.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the steps-to-go table.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_policy_create.restype = vp
    L.lle_policy_create.argtypes = [vp, C.POINTER(PolicyOptions)]
    L.lle_policy_free.restype = None
    L.lle_policy_free.argtypes = [vp]
    L.lle_policy_build.restype = i32
    L.lle_policy_build.argtypes = [vp, C.POINTER(PolicyArgs), C.POINTER(PolicyResult)]
    L.lle_policy_stats.restype = i32
    L.lle_policy_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_policy_lookup.restype = i32
    L.lle_policy_lookup.argtypes = [vp, vp, vp, vp, C.c_int64, vp]
    L.lle_policy_map_fingerprint.restype = C.c_uint64
    L.lle_policy_map_fingerprint.argtypes = [vp]
    L.lle_policy_last_error.restype = C.c_char_p
    L.lle_policy_last_error.argtypes = []
    for fn in (L.lle_policy_debug_launched, L.lle_policy_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_policy.so this process has launched (lle_policy_debug_launched)."""
    return _binding.names(lib().lle_policy_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_policy_debug_compiled)."""
    return _binding.names(lib().lle_policy_debug_compiled)


def map_fingerprint(map_):
    """lle_policy_map_fingerprint of a Map (host only): a 64-bit hash of what decides a step -- dimensions, positions of every kind,
    sources, laser tiles.  Equal for a clone."""
    v = lib().lle_policy_map_fingerprint(map_.h)
    if not v:
        raise RuntimeError(f"lle_policy_map_fingerprint failed: {lib().lle_policy_last_error().decode()}")
    return int(v)


class PolicyCapacityError(RuntimeError):
    """The build met more distinct states than `max_states`: there is no table.  Build the OptimalPolicy with a larger max_states."""


def _as_map(world):
    from .world import World
    if isinstance(world, World):
        return world._map
    if isinstance(world, _capi.Map):
        return world
    return _capi.Map(str(world))


def _device_index(device):
    if device is None:
        return -1
    if isinstance(device, int):
        return device
    text = str(device)
    return int(text.split(":")[1]) if ":" in text else -1


def _batched(env):
    """The BatchedWorld behind a BatchedWorld, a BatchedLLE or a World."""
    from .world import World
    if isinstance(env, World):
        return env._batch
    inner = getattr(env, "world", None)
    return inner if inner is not None and hasattr(inner, "h") and hasattr(inner, "maps") else env


class OptimalPolicy:
    """The steps-to-go table of one map up to `horizon` levels ("auto": (width * height) // 2, as Solver).

    `world`: an lle_amd.World, a Map or map text.  The policy is FROZEN at construction, like Solver: it keeps its own copy of the map
    as it is now and that copy's fingerprint; the table is built right here (PolicyCapacityError when the map has more than
    `max_states` distinct states within the horizon -- then there is no policy).  `collect_gems`: a goal also has every gem collected.
    `chunk`: environments of the build's own batch = work items per piece.

    Attributes: n_states, complete (the frontier ran empty: every reachable state is stored and every answer is exact),
    depth_reached, passes (relaxation passes; depends on scheduling), root_steps (steps from the reset state, None when unknown or
    unsolvable), stats (frontier / expanded per depth, explore_ms, relax_ms).

    Every lookup takes `env`: a BatchedWorld, a BatchedLLE or a World of the same map, of any size, on the policy's device; it
    compares the env's map fingerprint with the policy's (`check_map=False` skips that: the caller vouches for the map) and refuses
    an env with per-environment sources or more than one map with ValueError."""

    UNKNOWN = LLE_POLICY_UNKNOWN
    DEAD_END = LLE_POLICY_DEAD_END

    def __init__(self, world, horizon="auto", *, collect_gems=False, chunk=65536, max_states=1 << 22, device=None):
        from .world import World
        source = _as_map(world)
        self.horizon = (source.width * source.height) // 2 if isinstance(horizon, str) and horizon == "auto" else int(horizon)
        if not 0 <= self.horizon <= LLE_POLICY_MAX_HORIZON:
            raise ValueError(f"horizon must be 0 .. {LLE_POLICY_MAX_HORIZON}, got {self.horizon}.")
        if int(chunk) < 1 or int(max_states) < 1:
            raise ValueError("chunk and max_states must be at least 1")
        if source.n_agents > LLE_POLICY_MAX_AGENTS:
            raise ValueError(f"the table serves maps of at most {LLE_POLICY_MAX_AGENTS} agents (5^A joint actions per state); this one has "
                             f"{source.n_agents}")
        batch = getattr(world, "_batch_obj", None) if isinstance(world, World) else None
        if batch is not None and getattr(batch, "_env_sources", False):
            raise ValueError("the world keeps per-environment sources: the table is built on the map's own source colours and flags")
        self.collect_gems, self.chunk, self.max_states = bool(collect_gems), int(chunk), int(max_states)
        self.map = source.clone()  # frozen: later changes of the world's map do not reach this policy
        self.fingerprint = map_fingerprint(self.map)
        self.n_agents = self.map.n_agents
        L = lib()
        opt = PolicyOptions(C.sizeof(PolicyOptions), _device_index(device if device is not None else getattr(world, "_device", None)),
                            self.chunk, self.max_states, None)
        self.h = L.lle_policy_create(self.map.h, C.byref(opt))
        if not self.h:
            raise RuntimeError(f"lle_policy_create failed: {L.lle_policy_last_error().decode()}")
        self._lookup = L.lle_policy_lookup
        args = PolicyArgs(C.sizeof(PolicyArgs), int(self.collect_gems), self.horizon, 0)
        res = PolicyResult(C.sizeof(PolicyResult))
        rc = L.lle_policy_build(self.h, C.byref(args), C.byref(res))
        if rc != 0:
            message = L.lle_policy_last_error().decode()
            self.free()
            if rc == LLE_POLICY_CAPACITY:
                raise PolicyCapacityError(message)
            raise RuntimeError(f"lle_policy_build failed ({rc}): {message}")
        self.n_states, self.complete, self.depth_reached, self.passes = int(res.n_states), bool(res.complete), int(res.depth_reached), int(res.passes)
        self.root_steps = int(res.root_steps) if res.root_steps >= 0 else None
        cap = res.depth_reached + 2
        frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
        n = L.lle_policy_stats(self.h, frontier, expanded, cap)
        self.stats = dict(frontier=[int(frontier[d]) for d in range(n)], expanded=[int(expanded[d]) for d in range(res.depth_reached)],
                          explore_ms=float(res.explore_ms), relax_ms=float(res.relax_ms))

    # ---- the env a lookup reads
    def _world_of(self, env, check_map):
        w = _batched(env)
        if not hasattr(w, "h") or not hasattr(w, "maps"):
            raise TypeError(f"expected a BatchedWorld, a BatchedLLE or a World, got {type(env).__name__}")
        if len(w.maps) != 1:
            raise ValueError(f"the env holds {len(w.maps)} maps: the table is one map's")
        if getattr(w, "_env_sources", False):
            raise ValueError("the env keeps per-environment sources: the table is built on the map's own source colours and flags")
        if w.map.n_agents != self.n_agents:
            raise ValueError(f"the env's map has {w.map.n_agents} agents, the policy's {self.n_agents}")
        if check_map and map_fingerprint(w.map) != self.fingerprint:
            raise ValueError("the env's map is not the policy's (lle_policy_map_fingerprint differs): build an OptimalPolicy for it, or pass "
                             "check_map=False to vouch for it")
        return w

    def _call(self, w, steps, actions_ptr, action_stride):
        if not self.h:
            raise RuntimeError("the policy has been freed")
        rc = self._lookup(self.h, w.h, steps.data_ptr(), actions_ptr, action_stride, w._stream())
        if rc != 0:
            message = lib().lle_policy_last_error().decode()
            raise (ValueError if rc == -2 else RuntimeError)(f"lle_policy_lookup failed ({rc}): {message}")

    def _steps(self, w, out):
        import torch
        if out is None:
            return torch.empty(w.n_envs, dtype=torch.int32, device=w.device)
        if out.dtype != torch.int32 or out.device != w.device or tuple(out.shape) != (w.n_envs,) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int32 tensor of shape ({w.n_envs},) on {w.device}")
        return out

    def steps_to_go(self, env, check_map=True, out=None):
        """int32 [n] on the env's device: the length of the shortest plan from every environment's current state, UNKNOWN or DEAD_END.
        `out`: the tensor to write into (a hot loop allocates nothing)."""
        w = self._world_of(env, check_map)
        steps = self._steps(w, out)
        self._call(w, steps, None, 0)
        return steps

    def actions(self, env, check_map=True):
        """(uint8 [n, A], int32 [n]): an optimal joint action of every environment -- among the shortest, the one with the smallest
        base-5 code, agent 0 the lowest digit -- and steps_to_go; all STAY where steps is negative."""
        import torch
        w = self._world_of(env, check_map)
        steps = torch.empty(w.n_envs, dtype=torch.int32, device=w.device)
        actions = torch.empty((w.n_envs, self.n_agents), dtype=torch.uint8, device=w.device)
        self._call(w, steps, actions.data_ptr(), self.n_agents)
        return actions, steps

    def act(self, env, check_map=True, out=None):
        """Writes the actions into the env's own action buffer (`BatchedWorld.actions`) and returns steps_to_go (in `out` when given):
        `env.step(env.actions)` then takes them without a copy.  Nothing else of the env is written."""
        w = self._world_of(env, check_map)
        steps = self._steps(w, out)
        self._call(w, steps, w.actions.data_ptr(), int(w.actions.stride(0)))
        return steps

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_policy_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()


__all__ = ["OptimalPolicy", "PolicyCapacityError"]
