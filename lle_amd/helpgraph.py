"""ctypes binding of liblle_helpgraph.so (lle_amd/helpgraph/helpgraph.hip, C ABI include/lle_helpgraph.h) and
what the reference builds on its solve modes over the help graph: `HelpGraphSolver` (the `Solver` interface, serving the modes that
depend on who has helped whom) and `HelpGraphCharacterizer` (`WorldCharacterizer` with is_asymmetric, is_fully_coupled, is_mutual,
is_interdependent(2), is_convergent(k) and is_divergent(k) answered).

The reference encodes each mode as SAT clauses.  Here a breadth-first search walks (world state, help relation) records: the help
relation of a trajectory is the set of ordered pairs (helper, beneficiary) over all its states, the reset state included -- the same
thing as `TemporalCooperationGraph.flattened_edges()` -- and the five modes served depend on nothing else of a trajectory's past:

    plan = HelpGraphSolver(world, 10).find_shortest("no-mutual")       # a plan in which no two agents ever help each other, or None
    HelpGraphCharacterizer(world, 10).is_fully_coupled()               # does every plan make everybody help everybody else

Modes: "standard", "no-asymmetric", "no-mutual" = "no-interdependence[-2]", "no-fully-coupled", "no-convergence[-k]",
"no-divergence[-k]"; "no-cooperation" is answered by an inner `Solver` (a different rule: foreign beam tiles, on or off);
"no-sequence[-N]" and "no-interdependence-N" for N >= 3 need temporal trails and raise NotImplementedError.

The module is loaded only when such a solver is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _capi, solver
from .characterization import WorldCharacterizer, profile_plan
from .solver import SolveMode, SolverCapacityError, _parse_mode

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_helpgraph.so")

# include/lle_helpgraph.h
LLE_HELPGRAPH_CAPACITY = -20
(LLE_HELPGRAPH_STANDARD, LLE_HELPGRAPH_NO_ASYMMETRIC, LLE_HELPGRAPH_NO_MUTUAL, LLE_HELPGRAPH_NO_FULLY_COUPLED, LLE_HELPGRAPH_NO_CONVERGENCE,
 LLE_HELPGRAPH_NO_DIVERGENCE) = range(6)
LLE_HELPGRAPH_MAX_AGENTS = 6
LLE_HELPGRAPH_MAX_SOURCES = 32

EXPORTS = ["lle_helpgraph_create", "lle_helpgraph_free", "lle_helpgraph_run", "lle_helpgraph_plan", "lle_helpgraph_stats", "lle_helpgraph_last_error",
           "lle_helpgraph_debug_launched", "lle_helpgraph_debug_compiled"]


class HelpGraphOptions(C.Structure):
    """lle_helpgraph_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("chunk", C.c_int64), ("max_states", C.c_int64), ("stream", C.c_void_p)]


class HelpGraphArgs(C.Structure):
    """lle_helpgraph_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("mode", C.c_int32), ("param", C.c_int32), ("collect_gems", C.c_int32), ("t_max", C.c_int32)]


class HelpGraphResult(C.Structure):
    """lle_helpgraph_result."""
    _fields_ = [("struct_bytes", C.c_uint32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("pad", C.c_int32),
                ("step_errors", C.c_int64), ("help_lo", C.c_uint32), ("help_hi", C.c_uint32)]


_lib = None


def lib():
    """Load liblle_helpgraph.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the help-graph solver.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_helpgraph_create.restype = vp
    L.lle_helpgraph_create.argtypes = [vp, C.POINTER(HelpGraphOptions)]
    L.lle_helpgraph_free.restype = None
    L.lle_helpgraph_free.argtypes = [vp]
    L.lle_helpgraph_run.restype = i32
    L.lle_helpgraph_run.argtypes = [vp, C.POINTER(HelpGraphArgs), C.POINTER(HelpGraphResult)]
    L.lle_helpgraph_plan.restype = i32
    L.lle_helpgraph_plan.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_helpgraph_stats.restype = i32
    L.lle_helpgraph_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_helpgraph_last_error.restype = C.c_char_p
    L.lle_helpgraph_last_error.argtypes = []
    for fn in (L.lle_helpgraph_debug_launched, L.lle_helpgraph_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_helpgraph.so this process has launched (lle_helpgraph_debug_launched)."""
    return solver._names(lib().lle_helpgraph_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_helpgraph_debug_compiled)."""
    return solver._names(lib().lle_helpgraph_debug_compiled)


def help_edges(lo, hi=0):
    """The set of (helper, beneficiary) pairs of a help value: bit 8 h + b of the 48-bit value lo | hi << 32."""
    value = int(lo) | int(hi) << 32
    return {(h, b) for h in range(LLE_HELPGRAPH_MAX_AGENTS) for b in range(8) if (value >> (8 * h + b)) & 1}


# ------------------------------------------------------------------------------------------------ solve modes
_NATIVE = {"standard": LLE_HELPGRAPH_STANDARD, "no-asymmetric": LLE_HELPGRAPH_NO_ASYMMETRIC, "no-fully-coupled": LLE_HELPGRAPH_NO_FULLY_COUPLED,
           "no-interdependence": LLE_HELPGRAPH_NO_MUTUAL, "no-convergence": LLE_HELPGRAPH_NO_CONVERGENCE, "no-divergence": LLE_HELPGRAPH_NO_DIVERGENCE}
SERVED = ("'standard', 'no-cooperation', 'no-asymmetric', 'no-mutual' (= 'no-interdependence[-2]'), 'no-fully-coupled', 'no-convergence[-k]' and "
          "'no-divergence[-k]'")


def serves(mode):
    """Whether HelpGraphSolver answers the solve mode (a SolveMode or its text)."""
    mode = _parse_mode(mode)
    if mode.kind == "no-cooperation":
        return True
    if mode.kind == "no-interdependence":
        return mode.n == 2
    return mode.kind in _NATIVE


def _served_mode(mode):
    asked = mode
    mode = _parse_mode(mode)
    if not serves(mode):
        name = f"'{asked}'" if str(asked) == str(mode) else f"'{asked}' ('{mode}')"
        raise NotImplementedError(f"solve mode {name} is not built: it needs temporal trails, not a flattened help relation; the help-graph search "
                                  f"serves {SERVED}")
    return mode


class HelpGraphSolver(solver.Solver):
    """`Solver` over liblle_helpgraph.so: shortest joint plans of one world up to the horizon `t_max` whose flattened help relation
    avoids a shape of cooperation.  Same constructor, same freezing at construction, same `find_shortest` / `solve` /
    `solution_lower_bound` / `last_stats`, STAY padding and ValueErrors as `Solver`; `last_stats` additionally carries `help_edges`, the
    (helper, beneficiary) pairs of the plan's last state (None without a plan; absent after "no-cooperation", which the inner `Solver`
    answers).  `max_states` counts (world state, help relation) records: SolverCapacityError beyond it."""

    def __init__(self, world, t_max="auto", *, chunk=65536, max_states=1 << 22, device=None):
        super().__init__(world, t_max, chunk=chunk, max_states=max_states, device=device)
        self._inner = None  # the Solver that answers "no-cooperation", made when it is asked for

    def _check_mode(self, mode):
        return _served_mode(mode)

    # ---- the device side
    def _handle(self):
        if self.h is None:
            L = lib()
            opt = HelpGraphOptions(C.sizeof(HelpGraphOptions), self._device, self.chunk, self.max_states, None)
            self.h = L.lle_helpgraph_create(self._map.h, C.byref(opt))
            if not self.h:
                raise RuntimeError(f"lle_helpgraph_create failed: {L.lle_helpgraph_last_error().decode()}")
        return self.h

    def _no_cooperation(self, collect_gems):
        if self._inner is None:
            self._inner = solver.Solver(self._map, self.t_max, chunk=self.chunk, max_states=self.max_states, device=None if self._device < 0 else self._device)
        rows = self._inner._shortest(SolveMode.no_cooperation(), collect_gems)
        self.last_stats = self._inner.last_stats
        return rows

    def _shortest(self, mode, collect_gems):
        """(plan as a list of rows of action values, or None) of the native search, cached per (mode, collect_gems)."""
        if mode.kind == "no-cooperation":
            return self._no_cooperation(collect_gems)
        key = (str(mode), bool(collect_gems))
        if key not in self._cache:
            L, h = lib(), self._handle()
            args = HelpGraphArgs(C.sizeof(HelpGraphArgs), _NATIVE[mode.kind], mode.n or 2, int(bool(collect_gems)), self.t_max)
            res = HelpGraphResult(C.sizeof(HelpGraphResult))
            rc = L.lle_helpgraph_run(h, C.byref(args), C.byref(res))
            if rc == LLE_HELPGRAPH_CAPACITY:
                raise SolverCapacityError(L.lle_helpgraph_last_error().decode())
            if rc != 0:
                raise RuntimeError(f"lle_helpgraph_run failed ({rc}): {L.lle_helpgraph_last_error().decode()}")
            A, plan = self.world.n_agents, None
            if res.length >= 0:
                buf = (C.c_uint8 * max(res.length * A, 1))()
                if L.lle_helpgraph_plan(h, buf, res.length * A) != res.length:
                    raise RuntimeError(f"lle_helpgraph_plan failed: {L.lle_helpgraph_last_error().decode()}")
                plan = [[int(buf[t * A + a]) for a in range(A)] for t in range(res.length)]
            cap = res.depth_reached + 2
            frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
            n = L.lle_helpgraph_stats(h, frontier, expanded, cap)
            stats = dict(frontier=[int(frontier[d]) for d in range(n)], expanded=[int(expanded[d]) for d in range(res.depth_reached)],
                         n_states=int(res.n_states), length=None if res.length < 0 else int(res.length),
                         help_edges=None if res.length < 0 else help_edges(res.help_lo, res.help_hi))
            self._cache[key] = (plan, stats)
        plan, stats = self._cache[key]
        self.last_stats = dict(stats, frontier=list(stats["frontier"]), expanded=list(stats["expanded"]),
                               help_edges=None if stats["help_edges"] is None else set(stats["help_edges"]))
        return plan

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_helpgraph_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None
        inner = getattr(self, "_inner", None)
        if inner is not None:
            inner.free()


class HelpGraphCharacterizer(WorldCharacterizer):
    """`WorldCharacterizer` over a `HelpGraphSolver`: the predicates of python/lle/characterization/world_characterization.py that ask
    for a plan avoiding a shape of cooperation.  A predicate holds when the world is solvable within t_max and NO plan within t_max
    avoids the shape; as in the reference the profile of the shortest plan is asked first (a plan that shows the shape is implied by
    "no plan avoids it", so the answers are the same either way, and a cheap no saves a search).  `is_sequential` and
    `is_interdependent(n >= 3)` need temporal trails and raise as `WorldCharacterizer`'s do."""

    def __init__(self, world, t_max, **solver_options):
        self._solver = HelpGraphSolver(world, t_max, **solver_options)
        self.world = self._solver.world
        self.t_max = self._solver.t_max
        self._results = {}

    def _find(self, mode):
        return self._cached(str(mode), lambda: self._solver.find_shortest(mode))

    @property
    def _shortest_path_profile(self):
        """The cooperation profile of `shortest_path` (None for an unsolvable world), replayed on a world of the solver's frozen map."""
        def compute():
            if self.shortest_path is None:
                return None
            from .world import World
            return profile_plan(World(None, _map=self._solver._map.clone()), self.shortest_path)
        return self._cached("profile", compute)

    @property
    def shortest_non_asymmetric_path(self):
        return self._find(SolveMode.no_asymmetric())

    @property
    def shortest_non_fully_coupled_path(self):
        return self._find(SolveMode.no_fully_coupled())

    def compute_shortest_path_without_convergence(self, k):
        """The shortest plan in which no agent is helped by k distinct agents, or None."""
        if k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {k}.")
        return self._find(SolveMode.no_convergence(k))

    def compute_shortest_path_without_divergence(self, k):
        """The shortest plan in which no agent helps k distinct agents, or None."""
        if k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {k}.")
        return self._find(SolveMode.no_divergence(k))

    def compute_shortest_non_interdependent_path(self, order):
        """The shortest plan without a closed trail over exactly `order` agents, or None; order 2 only."""
        if order < 2:
            raise ValueError(f"Interdependence order must be >= 2, got {order}.")
        return self._find(SolveMode.no_interdependence(order))

    def is_asymmetric(self):
        if self.shortest_path is None:
            return False
        if self.n_laser_colours == 0:
            return False
        if not self._shortest_path_profile.is_asymmetric:
            return False
        if self.shortest_independent_path is not None:
            return False
        return self.shortest_non_asymmetric_path is None

    def is_fully_coupled(self):
        if self.shortest_path is None:
            return False
        return self.shortest_non_fully_coupled_path is None

    def is_convergent(self, k=2):
        if k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {k}.")
        if self.shortest_path is None:
            return False
        if not self._shortest_path_profile.is_convergent(k):
            return False
        return self.compute_shortest_path_without_convergence(k) is None

    def is_divergent(self, k=2):
        if k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {k}.")
        if k >= self.world.n_agents:
            return False
        if self.shortest_path is None:
            return False
        if not self._shortest_path_profile.is_divergent(k):
            return False
        return self.compute_shortest_path_without_divergence(k) is None

    def is_interdependent(self, n_agents=2):
        if n_agents < 2:
            raise ValueError(f"Interdependence only makes sense for >= 2 agents. Got {n_agents}.")
        if n_agents > 2:
            return super().is_interdependent(n_agents)  # raises: temporal trails
        if self.shortest_path is None:
            return False
        if not self._shortest_path_profile.is_interdependent(2):
            return False
        return self.compute_shortest_non_interdependent_path(2) is None

    def is_mutual(self):
        return self.is_interdependent(2)

    def __eq__(self, other):
        return isinstance(other, HelpGraphCharacterizer) and self.world == other.world and self.t_max == other.t_max

    def __hash__(self):
        return hash((self.world, self.t_max))


__all__ = ["HelpGraphSolver", "HelpGraphCharacterizer"]
