"""ctypes binding of liblle_trails.so (lle_amd/trails/trails.hip, C ABI include/lle_trails.h) and what the
reference builds on its solve mode no-sequence[-N]: `TrailSolver` (the `Solver` interface, serving "no-sequence[-N]" natively and every
mode of `HelpGraphSolver` through an inner one) and `TrailCharacterizer` (`HelpGraphCharacterizer` with is_sequential answered).

A sequence of length N is a TRAIL of N help edges (helper, beneficiary, t): each starts at the agent the one before ends at, the times
do not decrease, no temporal edge is used twice (`TemporalCooperationGraph.longest_trail_length`).  The flattened help relation does
not decide it -- the order of the help events does -- so the search walks (world state, trail lengths) records: L[a] is the length of
the longest trail that ends at agent a, and a trajectory is dropped the moment some L[a] reaches N:

    plan = TrailSolver(world, 10).find_shortest("no-sequence-3")     # a plan without a trail of three help edges, or None
    TrailCharacterizer(world, 10).is_sequential(3)                   # does every plan within 10 steps hold such a trail

Modes: "no-sequence[-N]" for 2 <= N <= 16, and everything `HelpGraphSolver` serves; "no-interdependence-N" for N >= 3 (a closed trail
over exactly N distinct agents) raises NotImplementedError here: `lle_amd.CycleSolver` (lle_amd.cycles) serves it.

The module is loaded only when such a solver is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _capi, helpgraph, solver
from .helpgraph import HelpGraphCharacterizer, HelpGraphSolver
from .solver import SolverCapacityError, _parse_mode

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_trails.so")

# include/lle_trails.h
LLE_TRAILS_CAPACITY = -20
LLE_TRAILS_DENSE = -21
LLE_TRAILS_MAX_AGENTS = 6
LLE_TRAILS_MAX_SOURCES = 32
LLE_TRAILS_MIN_LENGTH = 2
LLE_TRAILS_MAX_LENGTH = 16
LLE_TRAILS_WALK_BUDGET = 4096

EXPORTS = ["lle_trails_create", "lle_trails_free", "lle_trails_run", "lle_trails_plan", "lle_trails_stats", "lle_trails_last_error",
           "lle_trails_debug_launched", "lle_trails_debug_compiled"]


class TrailOptions(C.Structure):
    """lle_trails_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("chunk", C.c_int64), ("max_states", C.c_int64), ("stream", C.c_void_p)]


class TrailArgs(C.Structure):
    """lle_trails_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("length_n", C.c_int32), ("collect_gems", C.c_int32), ("t_max", C.c_int32)]


class TrailResult(C.Structure):
    """lle_trails_result."""
    _fields_ = [("struct_bytes", C.c_uint32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("trail", C.c_uint32),
                ("step_errors", C.c_int64)]


_lib = None


def lib():
    """Load liblle_trails.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the trail solver.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_trails_create.restype = vp
    L.lle_trails_create.argtypes = [vp, C.POINTER(TrailOptions)]
    L.lle_trails_free.restype = None
    L.lle_trails_free.argtypes = [vp]
    L.lle_trails_run.restype = i32
    L.lle_trails_run.argtypes = [vp, C.POINTER(TrailArgs), C.POINTER(TrailResult)]
    L.lle_trails_plan.restype = i32
    L.lle_trails_plan.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_trails_stats.restype = i32
    L.lle_trails_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_trails_last_error.restype = C.c_char_p
    L.lle_trails_last_error.argtypes = []
    for fn in (L.lle_trails_debug_launched, L.lle_trails_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_trails.so this process has launched (lle_trails_debug_launched)."""
    return solver._names(lib().lle_trails_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_trails_debug_compiled)."""
    return solver._names(lib().lle_trails_debug_compiled)


def trail_lengths(word, n_agents):
    """The per-agent L of a trail value: 4 bits per agent, agent a in bits 4 a .. 4 a + 3."""
    return [(int(word) >> (4 * a)) & 15 for a in range(n_agents)]


# ------------------------------------------------------------------------------------------------ solve modes
SERVED = ("'no-sequence[-N]' for N up to 16, " + helpgraph.SERVED)


def serves(mode):
    """Whether TrailSolver answers the solve mode (a SolveMode or its text)."""
    mode = _parse_mode(mode)
    if mode.kind == "no-sequence":
        return mode.n <= LLE_TRAILS_MAX_LENGTH
    return helpgraph.serves(mode)


def _served_mode(mode):
    asked = mode
    mode = _parse_mode(mode)
    if not serves(mode):
        name = f"'{asked}'" if str(asked) == str(mode) else f"'{asked}' ('{mode}')"
        if mode.kind == "no-sequence":
            raise NotImplementedError(f"solve mode {name} is not built: the trail search serves sequences of at most {LLE_TRAILS_MAX_LENGTH} help edges "
                                      "(a trail length is kept in 4 bits per agent)")
        raise NotImplementedError(f"solve mode {name} is not built: a closed trail over exactly N >= 3 distinct agents needs a visited set per trail, "
                                  f"not a trail length per agent; the trail search serves {SERVED}")
    return mode


class TrailSolver(solver.Solver):
    """`Solver` over liblle_trails.so: shortest joint plans of one world up to the horizon `t_max` that hold no trail of N help edges
    ("no-sequence[-N]", 2 <= N <= 16).  Same constructor, same freezing at construction, same `find_shortest` / `solve` /
    `solution_lower_bound` / `last_stats`, STAY padding and ValueErrors as `HelpGraphSolver`; every mode that one serves is handed to an
    inner `HelpGraphSolver`, made on first use, so one object answers everything but "no-interdependence-N" for N >= 3.  After a native
    search `last_stats` additionally carries `trail_lengths`, the per-agent length of the longest trail ending at the agent over the
    plan's states, and `longest_trail`, their maximum (both None without a plan).  `max_states` counts (world state, trail lengths)
    records: SolverCapacityError beyond it.  A state whose arcs allow more trail extensions than the walk's budget
    (LLE_TRAILS_WALK_BUDGET) ends the search with a RuntimeError: there is no answer then, never a partial one."""

    def __init__(self, world, t_max="auto", *, chunk=65536, max_states=1 << 22, device=None):
        super().__init__(world, t_max, chunk=chunk, max_states=max_states, device=device)
        self._inner = None  # the HelpGraphSolver that answers the modes over the flattened help relation, made when one is asked for

    def _check_mode(self, mode):
        return _served_mode(mode)

    # ---- the device side
    def _handle(self):
        if self.h is None:
            L = lib()
            opt = TrailOptions(C.sizeof(TrailOptions), self._device, self.chunk, self.max_states, None)
            self.h = L.lle_trails_create(self._map.h, C.byref(opt))
            if not self.h:
                raise RuntimeError(f"lle_trails_create failed: {L.lle_trails_last_error().decode()}")
        return self.h

    def _delegated(self, mode, collect_gems):
        if self._inner is None:
            self._inner = HelpGraphSolver(self._map, self.t_max, chunk=self.chunk, max_states=self.max_states, device=None if self._device < 0 else self._device)
        rows = self._inner._shortest(mode, collect_gems)
        self.last_stats = self._inner.last_stats
        return rows

    def _shortest(self, mode, collect_gems):
        """(plan as a list of rows of action values, or None) of the native search, cached per (mode, collect_gems)."""
        if mode.kind != "no-sequence":
            return self._delegated(mode, collect_gems)
        key = (str(mode), bool(collect_gems))
        if key not in self._cache:
            L, h = lib(), self._handle()
            args = TrailArgs(C.sizeof(TrailArgs), mode.n, int(bool(collect_gems)), self.t_max)
            res = TrailResult(C.sizeof(TrailResult))
            rc = L.lle_trails_run(h, C.byref(args), C.byref(res))
            if rc == LLE_TRAILS_CAPACITY:
                raise SolverCapacityError(L.lle_trails_last_error().decode())
            if rc == LLE_TRAILS_DENSE:
                raise RuntimeError(f"the trail search has no answer for '{mode}': {L.lle_trails_last_error().decode()}")
            if rc != 0:
                raise RuntimeError(f"lle_trails_run failed ({rc}): {L.lle_trails_last_error().decode()}")
            A, plan = self.world.n_agents, None
            if res.length >= 0:
                buf = (C.c_uint8 * max(res.length * A, 1))()
                if L.lle_trails_plan(h, buf, res.length * A) != res.length:
                    raise RuntimeError(f"lle_trails_plan failed: {L.lle_trails_last_error().decode()}")
                plan = [[int(buf[t * A + a]) for a in range(A)] for t in range(res.length)]
            cap = res.depth_reached + 2
            frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
            n = L.lle_trails_stats(h, frontier, expanded, cap)
            lengths = None if res.length < 0 else trail_lengths(res.trail, A)
            stats = dict(frontier=[int(frontier[d]) for d in range(n)], expanded=[int(expanded[d]) for d in range(res.depth_reached)],
                         n_states=int(res.n_states), length=None if res.length < 0 else int(res.length),
                         trail_lengths=lengths, longest_trail=None if lengths is None else max(lengths))
            self._cache[key] = (plan, stats)
        plan, stats = self._cache[key]
        self.last_stats = dict(stats, frontier=list(stats["frontier"]), expanded=list(stats["expanded"]),
                               trail_lengths=None if stats["trail_lengths"] is None else list(stats["trail_lengths"]))
        return plan

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_trails_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None
        inner = getattr(self, "_inner", None)
        if inner is not None:
            inner.free()


class TrailCharacterizer(HelpGraphCharacterizer):
    """`HelpGraphCharacterizer` over a `TrailSolver`: `is_sequential(length)` of python/lle/characterization/world_characterization.py
    is answered as well -- the world is solvable within t_max, the shortest plan holds a trail of `length` help edges (asked first: a
    cheap no saves a search), and NO plan within t_max avoids every such trail.  `is_interdependent(n >= 3)` keeps raising."""

    def __init__(self, world, t_max, **solver_options):
        self._solver = TrailSolver(world, t_max, **solver_options)
        self.world = self._solver.world
        self.t_max = self._solver.t_max
        self._results = {}

    def compute_shortest_path_without_sequence(self, length):
        """The shortest plan without a trail of `length` help edges, or None."""
        if length < 2:
            raise ValueError(f"Sequence length must be >= 2, got {length}.")
        return self._find(solver.SolveMode.no_sequence(length))

    def is_sequential(self, length=2):
        if length < 2:
            raise ValueError(f"Sequence length must be >= 2, got {length}.")
        if self.shortest_path is None:
            return False
        if not self._shortest_path_profile.is_sequential(length):
            return False
        return self.compute_shortest_path_without_sequence(length) is None

    def __eq__(self, other):
        return isinstance(other, TrailCharacterizer) and self.world == other.world and self.t_max == other.t_max

    def __hash__(self):
        return hash((self.world, self.t_max))


__all__ = ["TrailSolver", "TrailCharacterizer"]
