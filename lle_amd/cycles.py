"""ctypes binding of liblle_cycles.so (lle_amd/cycles/cycles.hip, C ABI include/lle_cycles.h) and what the
reference builds on its solve mode no-interdependence-N: `CycleSolver` (the `Solver` interface, serving "no-interdependence-N" for
N >= 3 natively and every mode of `TrailSolver` through an inner one) and `CycleCharacterizer` (`TrailCharacterizer` with
is_interdependent answered for every n).

A CLOSED TRAIL of order N is a trail of help edges (helper, beneficiary, t) -- each starts at the agent the one before ends at, the
times do not decrease, no temporal edge is used twice -- that returns to its first agent and visits exactly N distinct agents
(`TemporalCooperationGraph.has_closed_trail_of_order`).  Orders are not monotone: an order-4 ring need not hold an order-3 trail.
Neither the flattened help relation nor the trail lengths decide it, so the search walks (world state, triples) records: the triples
(anchor, current, support) say that some trail from `anchor` to `current` visits exactly the agents `support`, and a trajectory is
dropped the moment some (a, a, S) with |S| = N appears:

    plan = CycleSolver(world, 10).find_shortest("no-interdependence-3")   # a plan without a closed trail over three agents, or None
    CycleCharacterizer(world, 10).is_interdependent(3)                    # does every plan within 10 steps hold such a trail

Modes: "no-interdependence-N" for 3 <= N <= n_agents natively; N above the agents of the map is the `standard` answer (no such trail
can close); N = 2 ("no-mutual") and everything else `TrailSolver` serves go to an inner one, so one object answers every solve mode of
the reference -- only "no-sequence-17" and up still raise, with `TrailSolver`'s text.

The module is loaded only when such a solver is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _capi, solver, trails
from .solver import SolverCapacityError, _parse_mode
from .trails import TrailCharacterizer, TrailSolver

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_cycles.so")

# include/lle_cycles.h
LLE_CYCLES_CAPACITY = -20
LLE_CYCLES_DENSE = -21
LLE_CYCLES_MAX_AGENTS = 6
LLE_CYCLES_MAX_SOURCES = 32
LLE_CYCLES_MIN_ORDER = 2
LLE_CYCLES_MAX_ORDER = 6
LLE_CYCLES_WALK_BUDGET = 4096
LLE_CYCLES_VALUE_WORDS = 21

EXPORTS = ["lle_cycles_create", "lle_cycles_free", "lle_cycles_run", "lle_cycles_plan", "lle_cycles_stats", "lle_cycles_last_error",
           "lle_cycles_debug_launched", "lle_cycles_debug_compiled"]


class CycleOptions(C.Structure):
    """lle_cycles_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("chunk", C.c_int64), ("max_states", C.c_int64), ("stream", C.c_void_p)]


class CycleArgs(C.Structure):
    """lle_cycles_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("order_n", C.c_int32), ("collect_gems", C.c_int32), ("t_max", C.c_int32)]


class CycleResult(C.Structure):
    """lle_cycles_result."""
    _fields_ = [("struct_bytes", C.c_uint32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("value_words", C.c_int32),
                ("value", C.c_uint32 * LLE_CYCLES_VALUE_WORDS), ("step_errors", C.c_int64)]


_lib = None


def lib():
    """Load liblle_cycles.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the closed-trail solver.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_cycles_create.restype = vp
    L.lle_cycles_create.argtypes = [vp, C.POINTER(CycleOptions)]
    L.lle_cycles_free.restype = None
    L.lle_cycles_free.argtypes = [vp]
    L.lle_cycles_run.restype = i32
    L.lle_cycles_run.argtypes = [vp, C.POINTER(CycleArgs), C.POINTER(CycleResult)]
    L.lle_cycles_plan.restype = i32
    L.lle_cycles_plan.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_cycles_stats.restype = i32
    L.lle_cycles_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_cycles_last_error.restype = C.c_char_p
    L.lle_cycles_last_error.argtypes = []
    for fn in (L.lle_cycles_debug_launched, L.lle_cycles_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_cycles.so this process has launched (lle_cycles_debug_launched)."""
    return solver._names(lib().lle_cycles_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_cycles_debug_compiled)."""
    return solver._names(lib().lle_cycles_debug_compiled)


def _with_bit(p, k):
    """The mask p with a one inserted at bit k."""
    return (p >> k) << (k + 1) | 1 << k | p & ((1 << k) - 1)


def triples(words, n_agents):
    """The value of a record (include/lle_cycles.h: THE VALUE) as a set of (anchor, current, frozenset of agents): some trail of help
    edges from `anchor` to `current` visits exactly those agents.  `words`: 3 words for maps of up to 4 agents, 21 above.  The one
    place outside the library that knows the layout."""
    ac = 4 if n_agents <= 4 else 6
    words = [int(w) for w in words][:3 if ac == 4 else 21]
    if len(words) != (3 if ac == 4 else 21):
        raise ValueError(f"a value of a map of {n_agents} agents has {3 if ac == 4 else 21} words, got {len(words)}")
    value = sum(w << (32 * i) for i, w in enumerate(words))
    closed_bits, open_bits = 1 << (ac - 1), 1 << (ac - 2)
    out = set()
    for a in range(ac):
        for c in range(ac):
            if a == c:
                at, bits = a * closed_bits, closed_bits
            else:
                at, bits = ac * closed_bits + (a * (ac - 1) + c - (c > a)) * open_bits, open_bits
            for p in range(bits):
                if (value >> (at + p)) & 1:
                    mask = _with_bit(p, a) if a == c else _with_bit(_with_bit(p, min(a, c)), max(a, c))
                    out.add((a, c, frozenset(k for k in range(ac) if (mask >> k) & 1)))
    return out


# ------------------------------------------------------------------------------------------------ solve modes
SERVED = "'no-interdependence[-N]' for every N, " + trails.SERVED


def serves(mode):
    """Whether CycleSolver answers the solve mode (a SolveMode or its text)."""
    mode = _parse_mode(mode)
    return mode.kind == "no-interdependence" or trails.serves(mode)


def _served_mode(mode):
    parsed = _parse_mode(mode)
    if parsed.kind == "no-interdependence":
        return parsed
    return trails._served_mode(mode)  # (raises with TrailSolver's text for what nobody serves: no-sequence-17 and up)


class CycleSolver(solver.Solver):
    """`Solver` over liblle_cycles.so: shortest joint plans of one world up to the horizon `t_max` that hold no closed trail of help
    events over exactly N distinct agents ("no-interdependence-N").  Same constructor, same freezing at construction, same
    `find_shortest` / `solve` / `solution_lower_bound` / `last_stats`, STAY padding and ValueErrors as `TrailSolver`.  Routing of
    "no-interdependence-N": 3 <= N <= n_agents is searched natively; N > n_agents is the inner solver's `standard` answer (no closed
    trail of that order is possible), without a native search; N = 2 and every other mode go to an inner `TrailSolver`, made on first
    use -- so order 2 stays the FLATTENED "no-mutual" of `HelpGraphSolver`, as before.  After a native search `last_stats` additionally
    carries `triples`, the goal's value decoded to a set of (anchor, current, frozenset of agents), and `closed_orders`, the sorted
    orders below N of its closed triples (both None without a plan).  `max_states` counts (world state, triples) records:
    SolverCapacityError beyond it.  A state whose arcs allow more trail extensions than the walk's budget (LLE_CYCLES_WALK_BUDGET)
    ends the search with a RuntimeError: there is no answer then, never a partial one."""

    def __init__(self, world, t_max="auto", *, chunk=65536, max_states=1 << 22, device=None):
        super().__init__(world, t_max, chunk=chunk, max_states=max_states, device=device)
        self._inner = None  # the TrailSolver that answers every other mode, made when one is asked for

    def _check_mode(self, mode):
        return _served_mode(mode)

    # ---- the device side
    def _handle(self):
        if self.h is None:
            L = lib()
            opt = CycleOptions(C.sizeof(CycleOptions), self._device, self.chunk, self.max_states, None)
            self.h = L.lle_cycles_create(self._map.h, C.byref(opt))
            if not self.h:
                raise RuntimeError(f"lle_cycles_create failed: {L.lle_cycles_last_error().decode()}")
        return self.h

    def _delegated(self, mode, collect_gems):
        if self._inner is None:
            self._inner = TrailSolver(self._map, self.t_max, chunk=self.chunk, max_states=self.max_states, device=None if self._device < 0 else self._device)
        rows = self._inner._shortest(mode, collect_gems)
        self.last_stats = self._inner.last_stats
        return rows

    def _shortest(self, mode, collect_gems):
        """(plan as a list of rows of action values, or None), cached per (mode, collect_gems): routed as the class says."""
        if mode.kind != "no-interdependence" or mode.n == 2:
            return self._delegated(mode, collect_gems)
        if mode.n > self.world.n_agents:
            return self._delegated(solver.SolveMode.standard(), collect_gems)
        return self._native(mode.n, collect_gems)

    def shortest_without_closed_trail(self, order, collect_gems=False):
        """The shortest plan (rows of Actions, no padding) without a closed trail over exactly `order` agents, or None: always the
        native search, order 2 included (2 <= order <= n_agents).  TEMPORAL order 2 differs from the flattened "no-mutual": a helps b
        at t = 5 and b helps a at t = 3 is a mutual pair of the flattened relation and no closed trail, the times decrease."""
        order = int(order)
        if not LLE_CYCLES_MIN_ORDER <= order <= self.world.n_agents:
            raise ValueError(f"order must be 2 .. the map's agents ({self.world.n_agents}), got {order}")
        rows = self._native(order, collect_gems)
        return None if rows is None else self._padded(rows, len(rows))

    def _native(self, order, collect_gems):
        key = (f"closed-trail-{order}", bool(collect_gems))
        if key not in self._cache:
            L, h = lib(), self._handle()
            args = CycleArgs(C.sizeof(CycleArgs), order, int(bool(collect_gems)), self.t_max)
            res = CycleResult(C.sizeof(CycleResult))
            rc = L.lle_cycles_run(h, C.byref(args), C.byref(res))
            if rc == LLE_CYCLES_CAPACITY:
                raise SolverCapacityError(L.lle_cycles_last_error().decode())
            if rc == LLE_CYCLES_DENSE:
                raise RuntimeError(f"the closed-trail search has no answer for order {order}: {L.lle_cycles_last_error().decode()}")
            if rc != 0:
                raise RuntimeError(f"lle_cycles_run failed ({rc}): {L.lle_cycles_last_error().decode()}")
            A, plan = self.world.n_agents, None
            if res.length >= 0:
                buf = (C.c_uint8 * max(res.length * A, 1))()
                if L.lle_cycles_plan(h, buf, res.length * A) != res.length:
                    raise RuntimeError(f"lle_cycles_plan failed: {L.lle_cycles_last_error().decode()}")
                plan = [[int(buf[t * A + a]) for a in range(A)] for t in range(res.length)]
            cap = res.depth_reached + 2
            frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
            n = L.lle_cycles_stats(h, frontier, expanded, cap)
            found = None if res.length < 0 else frozenset(triples(list(res.value)[:res.value_words], A))
            stats = dict(frontier=[int(frontier[d]) for d in range(n)], expanded=[int(expanded[d]) for d in range(res.depth_reached)],
                         n_states=int(res.n_states), length=None if res.length < 0 else int(res.length), triples=found,
                         closed_orders=None if found is None else sorted({len(s) for a, c, s in found if a == c}))
            self._cache[key] = (plan, stats)
        plan, stats = self._cache[key]
        self.last_stats = dict(stats, frontier=list(stats["frontier"]), expanded=list(stats["expanded"]),
                               triples=None if stats["triples"] is None else set(stats["triples"]),
                               closed_orders=None if stats["closed_orders"] is None else list(stats["closed_orders"]))
        return plan

    def forget(self):
        """Drop the cached plans of this solver and of the inner ones; the device handles stay (for whoever times a search)."""
        solver_ = self
        while solver_ is not None:
            solver_._cache.clear()
            solver_ = getattr(solver_, "_inner", None)

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_cycles_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None
        inner = getattr(self, "_inner", None)
        if inner is not None:
            inner.free()


class CycleCharacterizer(TrailCharacterizer):
    """`TrailCharacterizer` over a `CycleSolver`: `is_interdependent(n)` of python/lle/characterization/world_characterization.py is
    answered for every n >= 2.  For n >= 3: the world is solvable within t_max, the shortest plan holds a closed trail over exactly n
    agents (asked first: a cheap no saves a search), and NO plan within t_max avoids every such trail.  For n = 2 the path is
    `HelpGraphCharacterizer`'s, over the flattened relation.  Each order is cached on its own."""

    def __init__(self, world, t_max, **solver_options):
        self._solver = CycleSolver(world, t_max, **solver_options)
        self.world = self._solver.world
        self.t_max = self._solver.t_max
        self._results = {}

    def compute_shortest_non_interdependent_path(self, order):
        """The shortest plan without a closed trail over exactly `order` agents ("no-interdependence-N"), or None."""
        if order < 2:
            raise ValueError(f"Interdependence order must be >= 2, got {order}.")
        return self._find(solver.SolveMode.no_interdependence(order))

    def is_interdependent(self, n_agents=2):
        if n_agents < 2:
            raise ValueError(f"Interdependence only makes sense for >= 2 agents. Got {n_agents}.")
        if n_agents == 2:
            return super().is_interdependent(2)
        if self.shortest_path is None:
            return False
        if not self._shortest_path_profile.is_interdependent(n_agents):
            return False
        return self.compute_shortest_non_interdependent_path(n_agents) is None

    def forget(self):
        """Drop every cached answer, here and in the solvers behind; the device handles stay."""
        self._results.clear()
        self._solver.forget()

    def __eq__(self, other):
        return isinstance(other, CycleCharacterizer) and self.world == other.world and self.t_max == other.t_max

    def __hash__(self):
        return hash((self.world, self.t_max))


__all__ = ["CycleSolver", "CycleCharacterizer"]
