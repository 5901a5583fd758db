"""ctypes binding of liblle_search.so (lle_amd/search/search.hip, C ABI include/lle_search.h) and the
reference's solver names over it: `Solver`, `solve`, `SolveMode` (python/lle/solver/solver.py).

The reference encodes a map as SAT clauses and asks MiniSat for a plan of each length in turn.  Here the shortest plan comes from a
breadth-first search over joint states in which every successor is computed by the step kernel itself, so the answer is exact with
respect to `World.step`:

    plan = Solver(World.level(4), 10).find_shortest()            # [(Action.SOUTH, Action.SOUTH), ...] or None
    Solver(world, 10).find_shortest("no-cooperation") is None    # every plan needs somebody in somebody else's beam

A plan is a list of joint actions from the reset state that `World.step` accepts, in which nobody dies and after which everybody has
arrived (with collect_gems: and every gem is collected).  A state in which all agents have arrived is absorbing (only STAY is
available), so a shortest plan padded with all-STAY rows is a plan of any greater length: that is what `t_min` and `solve(path_length)`
return.  Modes: "standard" and "no-cooperation"; the other mode names of the reference parse and raise NotImplementedError.

Which of several shortest plans comes back may differ between runs; its length and the per-depth counters (`last_stats`) do not.
The module is loaded only when a solver is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os
import re

from . import _binding, _capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_search.so")

# include/lle_search.h
LLE_SEARCH_CAPACITY = -20
LLE_SEARCH_STANDARD, LLE_SEARCH_NO_COOPERATION = 0, 1
LLE_SEARCH_MAX_AGENTS = 6

EXPORTS = ["lle_search_create", "lle_search_free", "lle_search_run", "lle_search_plan", "lle_search_stats", "lle_search_lower_bound",
           "lle_search_last_error", "lle_search_debug_launched", "lle_search_debug_compiled"]


class SearchOptions(C.Structure):
    """lle_search_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("chunk", C.c_int64), ("max_states", C.c_int64), ("stream", C.c_void_p)]


class SearchArgs(C.Structure):
    """lle_search_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("mode", C.c_int32), ("collect_gems", C.c_int32), ("t_max", C.c_int32)]


class SearchResult(C.Structure):
    """lle_search_result."""
    _fields_ = [("struct_bytes", C.c_uint32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("pad", C.c_int32),
                ("step_errors", C.c_int64)]


_lib = None


def lib():
    """Load liblle_search.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the solver.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_search_create.restype = vp
    L.lle_search_create.argtypes = [vp, C.POINTER(SearchOptions)]
    L.lle_search_free.restype = None
    L.lle_search_free.argtypes = [vp]
    L.lle_search_run.restype = i32
    L.lle_search_run.argtypes = [vp, C.POINTER(SearchArgs), C.POINTER(SearchResult)]
    L.lle_search_plan.restype = i32
    L.lle_search_plan.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_search_stats.restype = i32
    L.lle_search_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_search_lower_bound.restype = i32
    L.lle_search_lower_bound.argtypes = [vp]
    L.lle_search_last_error.restype = C.c_char_p
    L.lle_search_last_error.argtypes = []
    for fn in (L.lle_search_debug_launched, L.lle_search_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


_names = _binding.names


def launched_kernels():
    """Names of the kernels of liblle_search.so this process has launched (lle_search_debug_launched)."""
    return _names(lib().lle_search_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_search_debug_compiled)."""
    return _names(lib().lle_search_debug_compiled)


def lower_bound(map_):
    """lle_search_lower_bound of a Map (host only): the reference's solution_lower_bound."""
    v = lib().lle_search_lower_bound(map_.h)
    if v < 0:
        raise RuntimeError(f"lle_search_lower_bound failed: {lib().lle_search_last_error().decode()}")
    return int(v)


class SolverCapacityError(RuntimeError):
    """The search met more distinct states than `max_states`: it has no answer.  Build the Solver with a larger max_states."""


# ------------------------------------------------------------------------------------------------ solve modes
_PARAMETRIZED = ("no-sequence", "no-interdependence", "no-convergence", "no-divergence")
_PLAIN = ("standard", "no-cooperation", "no-asymmetric", "no-fully-coupled")
_NATIVE = {"standard": LLE_SEARCH_STANDARD, "no-cooperation": LLE_SEARCH_NO_COOPERATION}
_UNKNOWN = ("Unknown solve mode: '{}'. Expected one of: 'standard', 'no-cooperation', 'no-asymmetric', 'no-mutual', 'no-fully-coupled', "
            "'no-sequence[-N]', 'no-interdependence[-N]', 'no-convergence[-N]', 'no-divergence[-N]'")


class SolveMode:
    """A solve mode of the reference (src/solver/solve_mode.rs): `kind` is the name without its parameter, `n` the parameter (None for
    the plain modes), `str(mode)` the canonical string ("no-sequence" for n = 2, "no-sequence-3")."""

    def __init__(self, kind, n=None):
        if kind not in _PLAIN + _PARAMETRIZED:
            raise ValueError(_UNKNOWN.format(kind))
        if (kind in _PARAMETRIZED) != (n is not None):
            raise ValueError(f"solve mode '{kind}' {'needs' if kind in _PARAMETRIZED else 'takes no'} parameter")
        if n is not None and int(n) < 2:
            raise ValueError(f"solve mode '{kind}' needs a parameter of at least 2, got {n}")
        self.kind, self.n = kind, None if n is None else int(n)

    @staticmethod
    def standard():
        return SolveMode("standard")

    @staticmethod
    def no_cooperation():
        return SolveMode("no-cooperation")

    @staticmethod
    def no_asymmetric():
        return SolveMode("no-asymmetric")

    @staticmethod
    def no_fully_coupled():
        return SolveMode("no-fully-coupled")

    @staticmethod
    def no_mutual():
        return SolveMode("no-interdependence", 2)

    @staticmethod
    def no_sequence(length=2):
        return SolveMode("no-sequence", length)

    @staticmethod
    def no_interdependence(order=2):
        return SolveMode("no-interdependence", order)

    @staticmethod
    def no_convergence(k=2):
        return SolveMode("no-convergence", k)

    @staticmethod
    def no_divergence(k=2):
        return SolveMode("no-divergence", k)

    @staticmethod
    def from_str(text):
        s = str(text).strip().lower()
        if s in _PLAIN:
            return SolveMode(s)
        if s == "no-mutual":
            return SolveMode.no_mutual()
        for kind in _PARAMETRIZED:
            if s == kind:
                return SolveMode(kind, 2)
            m = re.fullmatch(re.escape(kind) + r"-(\d+)", s)
            if m:
                return SolveMode(kind, int(m.group(1)))
        raise ValueError(_UNKNOWN.format(text))

    @property
    def is_built(self):
        """Whether the search serves this mode."""
        return self.kind in _NATIVE

    def __str__(self):
        return self.kind if self.n in (None, 2) else f"{self.kind}-{self.n}"

    def __repr__(self):
        return f"SolveMode({str(self)!r})"

    def __eq__(self, other):
        return isinstance(other, SolveMode) and (self.kind, self.n) == (other.kind, other.n)

    def __hash__(self):
        return hash((self.kind, self.n))


def _parse_mode(mode):
    return mode if isinstance(mode, SolveMode) else SolveMode.from_str(mode)


def _native_mode(mode):
    asked = mode
    mode = _parse_mode(mode)
    if not mode.is_built:
        name = f"'{asked}'" if str(asked) == str(mode) else f"'{asked}' ('{mode}')"
        raise NotImplementedError(f"solve mode {name} is not built: the search serves 'standard' and 'no-cooperation'")
    return mode


# ------------------------------------------------------------------------------------------------ Solver
def _as_world(world):
    from .world import World
    if isinstance(world, World):
        return world
    if isinstance(world, _capi.Map):
        return World(None, _map=world)
    return World(str(world))


def _device_index(device):
    if device is None:
        return -1
    if isinstance(device, int):
        return device
    text = str(device)
    return int(text.split(":")[1]) if ":" in text else -1


class Solver:
    """Shortest joint plans of one world up to the horizon `t_max` ("auto": (width * height) // 2).

    `world`: an lle_amd.World, a Map or map text.  The Solver is FROZEN at construction, like the reference's, whose clause generator
    is built there: it keeps its own copy of the map as it is now (exits, source colours and flags), and the lower bound, every search
    and the cache of their results (one per mode and collect_gems) answer for that copy whatever happens to the world afterwards --
    build a new Solver for a changed world.  The world's dynamic state plays no part (plans start at the reset state).  `chunk`: environments of the search's own batch = work items per piece; `max_states`: records of the state pool
    (SolverCapacityError beyond it).  The device handle is made by the first search and freed with the Solver."""

    def __init__(self, world, t_max="auto", *, chunk=65536, max_states=1 << 22, device=None):
        self.world = _as_world(world)
        self.t_max = (self.world.width * self.world.height) // 2 if isinstance(t_max, str) and t_max == "auto" else int(t_max)
        if self.t_max < 0:
            raise ValueError(f"t_max must be non-negative, got {self.t_max}.")
        if int(chunk) < 1 or int(max_states) < 1:
            raise ValueError("chunk and max_states must be at least 1")
        if self.world.n_agents > LLE_SEARCH_MAX_AGENTS:
            raise ValueError(f"the search serves maps of at most {LLE_SEARCH_MAX_AGENTS} agents (5^A joint actions per state); this one has "
                             f"{self.world.n_agents}")
        batch = getattr(self.world, "_batch_obj", None)
        if batch is not None and getattr(batch, "_env_sources", False):
            raise ValueError("the world keeps per-environment sources: the search runs on the map's own source colours and flags")
        self.chunk, self.max_states = int(chunk), int(max_states)
        self._device = _device_index(device if device is not None else getattr(self.world, "_device", None))
        self._map = self.world._map.clone()  # frozen: later changes of the world's map do not reach this Solver
        self.solution_lower_bound = lower_bound(self._map)
        self.h = None
        self._cache = {}
        self.last_stats = None

    # ---- the device side
    def _handle(self):
        if self.h is None:
            L = lib()
            opt = SearchOptions(C.sizeof(SearchOptions), self._device, self.chunk, self.max_states, None)
            self.h = L.lle_search_create(self._map.h, C.byref(opt))
            if not self.h:
                raise RuntimeError(f"lle_search_create failed: {L.lle_search_last_error().decode()}")
        return self.h

    def _shortest(self, mode, collect_gems):
        """(plan as a list of rows of action values, or None) of the native search, cached per (mode, collect_gems)."""
        key = (str(mode), bool(collect_gems))
        if key not in self._cache:
            L, h = lib(), self._handle()
            args = SearchArgs(C.sizeof(SearchArgs), _NATIVE[mode.kind], int(bool(collect_gems)), self.t_max)
            res = SearchResult(C.sizeof(SearchResult))
            rc = L.lle_search_run(h, C.byref(args), C.byref(res))
            if rc == LLE_SEARCH_CAPACITY:
                raise SolverCapacityError(L.lle_search_last_error().decode())
            if rc != 0:
                raise RuntimeError(f"lle_search_run failed ({rc}): {L.lle_search_last_error().decode()}")
            A, plan = self.world.n_agents, None
            if res.length >= 0:
                buf = (C.c_uint8 * max(res.length * A, 1))()
                if L.lle_search_plan(h, buf, res.length * A) != res.length:
                    raise RuntimeError(f"lle_search_plan failed: {L.lle_search_last_error().decode()}")
                plan = [[int(buf[t * A + a]) for a in range(A)] for t in range(res.length)]
            cap = res.depth_reached + 2
            frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
            n = L.lle_search_stats(h, frontier, expanded, cap)
            stats = dict(frontier=[int(frontier[d]) for d in range(n)], expanded=[int(expanded[d]) for d in range(res.depth_reached)],
                         n_states=int(res.n_states), length=None if res.length < 0 else int(res.length))
            self._cache[key] = (plan, stats)
        plan, stats = self._cache[key]
        self.last_stats = dict(stats, frontier=list(stats["frontier"]), expanded=list(stats["expanded"]))
        return plan

    def _padded(self, rows, length):
        from .world import Action
        stay = [Action.STAY.value] * self.world.n_agents
        rows = rows + [stay] * (length - len(rows))
        return [tuple(Action(v) for v in row) for row in rows]

    def _check_mode(self, mode):
        """The parsed solve mode when this solver serves it; NotImplementedError otherwise.  (Subclasses over other libraries replace it.)"""
        return _native_mode(mode)

    # ---- the reference's interface
    def find_shortest(self, mode="standard", *, t_min=None, collect_gems=False, shuffle=False):
        """The shortest plan of at most t_max steps, padded with all-STAY rows up to `t_min`; None when there is none (or the padded
        plan would exceed t_max).  `shuffle` is accepted and has no effect (it randomises the SAT solver of the reference)."""
        mode = self._check_mode(mode)
        if t_min is None or t_min < self.solution_lower_bound:
            t_min = self.solution_lower_bound
        elif t_min > self.t_max:
            raise ValueError(f"t_min={t_min} exceeds this solver's t_max={self.t_max}.")
        if t_min > self.t_max:  # the lower bound itself exceeds the horizon: no length to try
            return None
        rows = self._shortest(mode, collect_gems)
        if rows is None or max(len(rows), t_min) > self.t_max:
            return None
        return self._padded(rows, max(len(rows), t_min))

    def solve(self, path_length="auto", *, mode="standard", collect_gems=False, shuffle=False):
        """A plan of exactly `path_length` joint actions ("auto": t_max), or None."""
        if isinstance(path_length, str) and path_length == "auto":
            path_length = self.t_max
        elif path_length < 0:
            raise ValueError(f"path_length must be non-negative, got {path_length}.")
        elif path_length > self.t_max:
            raise ValueError(f"path_length={path_length} exceeds this solver's t_max={self.t_max}. Construct a new Solver with a larger t_max.")
        mode = self._check_mode(mode)
        if path_length < self.solution_lower_bound:
            return None
        rows = self._shortest(mode, collect_gems)
        if rows is None or len(rows) > path_length:
            return None
        return self._padded(rows, path_length)

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_search_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()


def solve(world, t_max="auto", /, *, path_length="auto", mode="standard", collect_gems=False, shuffle=False, **solver_options):
    """`Solver(world, t_max).solve(path_length=...)` (python/lle/solver/solver.py:123-146); `solver_options`: chunk, max_states, device."""
    return Solver(world, t_max, **solver_options).solve(path_length=path_length, mode=mode, collect_gems=collect_gems, shuffle=shuffle)


__all__ = ["Solver", "SolveMode", "SolverCapacityError", "solve"]
