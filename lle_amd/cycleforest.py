"""ctypes binding of liblle_cycleforest.so (lle_amd/cycleforest/cycleforest.hip, C ABI include/lle_cycleforest.h; INTEGRATION.md section
22) and what a filtered generator needs over it: `CycleForestSolver`, `solve_many`, `characterize_many`.

`lle_amd.helpforest` walks the help-graph and trail solve modes of many equally shaped maps in the same launches; `CycleSolver` answers
"no-interdependence-N" for N >= 3 -- no closed trail of help events over exactly N distinct agents -- one map per handle.  The cycle
forest is both: one batch made with lle_batch_create_multi, a segment of every array per map, records that carry the trail triples
of their trajectory -- and, per map, exactly the single search: the same lengths, per-depth counters and stored records.

    CycleForestSolver(worlds, 10).run("no-interdependence-3").length     # per map; -1: every plan closes a trail over three agents (or none exists)
    plans = solve_many(worlds, 10, mode="no-interdependence-3")          # [CycleSolver(w, 10).find_shortest("no-interdependence-3") for w in worlds]
    with characterize_many(worlds, 10) as c:                             # what CycleCharacterizer(w, 10) answers, as boolean arrays
        keep = c.is_interdependent(3)

Modes: everything `CycleSolver` serves, routed as it routes them: "no-interdependence-N" for 3 <= N <= n_agents is native, N above
the agents of the maps is the `standard` answer, N = 2 and every other mode go to an inner `HelpForestSolver`.  Which of several
shortest plans comes back may differ between runs; lengths and counters do not.  No fallback: a missing library raises.
"""
import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

from . import _capi, cycles, solver
from .cycles import LLE_CYCLES_CAPACITY, LLE_CYCLES_DENSE, LLE_CYCLES_MIN_ORDER, LLE_CYCLES_VALUE_WORDS, LLE_CYCLES_WALK_BUDGET, triples
from .forest import ForestResult, _groups
from .helpforest import HelpForestSolver, ManyHelpCharacterization, _HelpAnswered
from .helpforest import _refuse as _refuse_help
from .solver import SolveMode, SolverCapacityError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_cycleforest.so")

EXPORTS = ["lle_cycleforest_create", "lle_cycleforest_free", "lle_cycleforest_run", "lle_cycleforest_plan", "lle_cycleforest_value", "lle_cycleforest_stats",
           "lle_cycleforest_occupancy", "lle_cycleforest_last_error", "lle_cycleforest_debug_launched", "lle_cycleforest_debug_compiled"]
KERNELS = ["cf_commit<21>", "cf_commit<3>", "cf_expand", "cf_insert<21>", "cf_insert<3>", "cf_plans<21>", "cf_plans<3>", "cf_roots", "cf_seed<21>", "cf_seed<3>"]


class CycleForestOptions(C.Structure):
    """lle_cycleforest_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("envs_per_map", C.c_int64), ("max_states_per_map", C.c_int64), ("stream", C.c_void_p)]


class CycleForestArgs(C.Structure):
    """lle_cycleforest_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("order_n", C.c_int32), ("collect_gems", C.c_int32), ("t_max", C.c_int32)]


class CycleForestMapResult(C.Structure):
    """lle_cycleforest_result."""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("value_words", C.c_int32)]


_lib = None


def lib():
    """Load liblle_cycleforest.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the cycle forest.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_cycleforest_create.restype = vp
    L.lle_cycleforest_create.argtypes = [C.POINTER(vp), i32, C.POINTER(CycleForestOptions)]
    L.lle_cycleforest_free.restype = None
    L.lle_cycleforest_free.argtypes = [vp]
    L.lle_cycleforest_run.restype = i32
    L.lle_cycleforest_run.argtypes = [vp, C.POINTER(CycleForestArgs), C.POINTER(C.c_uint8), C.POINTER(CycleForestMapResult)]
    L.lle_cycleforest_plan.restype = i32
    L.lle_cycleforest_plan.argtypes = [vp, i32, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_cycleforest_value.restype = i32
    L.lle_cycleforest_value.argtypes = [vp, i32, C.POINTER(C.c_uint32)]
    L.lle_cycleforest_stats.restype = i32
    L.lle_cycleforest_stats.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_cycleforest_occupancy.restype = i32
    L.lle_cycleforest_occupancy.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lle_cycleforest_last_error.restype = C.c_char_p
    L.lle_cycleforest_last_error.argtypes = []
    for fn in (L.lle_cycleforest_debug_launched, L.lle_cycleforest_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_cycleforest.so this process has launched (lle_cycleforest_debug_launched)."""
    return solver._names(lib().lle_cycleforest_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_cycleforest_debug_compiled)."""
    return solver._names(lib().lle_cycleforest_debug_compiled)


# ------------------------------------------------------------------------------------------------ CycleForestSolver
@dataclass
class CycleForestResult(ForestResult):
    """One run of a cycle forest: `ForestResult` (status: 0, LLE_CYCLES_CAPACITY, or LLE_CYCLES_DENSE for a map one of whose states
    allows more trail extensions than the walk's budget), and per map what the goal's record carries after a native search."""
    triples: list = field(default_factory=list)        # per map: the goal's value decoded to a set of (anchor, current, frozenset of agents), or None
    closed_orders: list = field(default_factory=list)  # per map: the sorted orders of its closed triples (all below N), or None


def _from_inner(res, n_maps):
    """The result of the inner help forest as a CycleForestResult: nothing of a closed-trail search is carried."""
    return CycleForestResult(length=res.length, status=res.status, n_states=res.n_states, depth_reached=res.depth_reached, frontier=res.frontier,
                             expanded=res.expanded, plans=res.plans, valid_items=res.valid_items, launched_lanes=res.launched_lanes, pieces=res.pieces,
                             triples=[None] * n_maps, closed_orders=[None] * n_maps)


class CycleForestSolver(HelpForestSolver):
    """`ForestSolver` over liblle_cycleforest.so: shortest joint plans of many equally shaped worlds up to the horizon `t_max` that hold
    no closed trail of help events over exactly N distinct agents, searched together.  Same arguments, same refusals and same freezing
    at construction as `HelpForestSolver`.  `run` routes as `CycleSolver` does: "no-interdependence-N" for 3 <= N <= n_agents is
    searched natively; N > n_agents is the inner solver's `standard` answer; N = 2 and every other mode go to an inner
    `HelpForestSolver`, made on first use -- so order 2 stays the FLATTENED "no-mutual".  `max_states_per_map` counts (world state,
    triples) records.  Device memory: every solver that has run keeps its own batch of n_maps * envs_per_map environments and its own
    pool segments -- this one (made by the first native search only), the inner `HelpForestSolver` and that one's `ForestSolver` for
    "no-cooperation" -- so a characterisation that asks all three holds three of each until `free()`; that counts at an `envs_per_map`
    of 1024 or 4096."""

    def __init__(self, worlds, t_max="auto", *, envs_per_map=256, max_states_per_map=1 << 16, device=None):
        super().__init__(worlds, t_max, envs_per_map=envs_per_map, max_states_per_map=max_states_per_map, device=device)
        self._help = None  # the HelpForestSolver that answers every other mode, made when one is asked for

    def _handle(self):
        if self.h is None:
            L = lib()
            opt = CycleForestOptions(C.sizeof(CycleForestOptions), self._device, self.envs_per_map, self.max_states_per_map, None)
            handles = (C.c_void_p * self.n_maps)(*[m.h for m in self._maps])
            self.h = L.lle_cycleforest_create(handles, self.n_maps, C.byref(opt))
            if not self.h:
                message = L.lle_cycleforest_last_error().decode()
                if "must agree" in message:
                    raise ValueError(f"lle_cycleforest_create failed: {message}")
                raise RuntimeError(f"lle_cycleforest_create failed: {message}")
        return self.h

    def _delegated(self, mode, collect_gems, only):
        if self._help is None:
            self._help = HelpForestSolver(self._maps, self.t_max, envs_per_map=self.envs_per_map, max_states_per_map=self.max_states_per_map,
                                          device=None if self._device < 0 else self._device)
        return _from_inner(self._help.run(mode, collect_gems, only=only), self.n_maps)

    def run(self, mode="standard", collect_gems=False, only=None):
        """One search of every map in `mode`; `only`: a boolean per map, False = not searched (length -1, n_states 0, depth_reached 0,
        status 0).  The CycleForestResult is cached per (mode, collect_gems) when `only` is None."""
        mode = cycles._served_mode(mode)
        mask = self._mask(only)
        key = (str(mode), bool(collect_gems))
        if mask is None and key in self._cache:
            return self._cache[key]
        if mode.kind != "no-interdependence" or mode.n == 2:
            out = self._delegated(mode, collect_gems, mask)
        elif mode.n > self.n_agents:
            out = self._delegated(SolveMode.standard(), collect_gems, mask)
        else:
            out = self._native(mode.n, collect_gems, mask)
        if mask is None:
            self._cache[key] = out
        return out

    def run_closed_trail(self, order, collect_gems=False, only=None):
        """One search of every map for the shortest plan without a closed trail over exactly `order` agents: always the native search,
        order 2 included (2 <= order <= n_agents) -- the twin of `CycleSolver.shortest_without_closed_trail`.  Cached like `run`."""
        order = int(order)
        if not LLE_CYCLES_MIN_ORDER <= order <= self.n_agents:
            raise ValueError(f"order must be 2 .. the maps' agents ({self.n_agents}), got {order}")
        mask = self._mask(only)
        key = (f"closed-trail-{order}", bool(collect_gems))
        if mask is None and key in self._cache:
            return self._cache[key]
        out = self._native(order, collect_gems, mask)
        if mask is None:
            self._cache[key] = out
        return out

    def _native(self, order, collect_gems, mask):
        from .world import Action
        L, h, M, A = lib(), self._handle(), self.n_maps, self.n_agents
        args = CycleForestArgs(C.sizeof(CycleForestArgs), order, int(bool(collect_gems)), self.t_max)
        res = (CycleForestMapResult * M)()
        search = None if mask is None else (C.c_uint8 * M)(*[int(v) for v in mask])
        rc = L.lle_cycleforest_run(h, C.byref(args), search, res)
        if rc != 0:
            raise RuntimeError(f"lle_cycleforest_run failed ({rc}): {L.lle_cycleforest_last_error().decode()}")
        out = CycleForestResult(length=np.array([r.length for r in res], dtype=np.int32), status=np.array([r.status for r in res], dtype=np.int32),
                                n_states=np.array([r.n_states for r in res], dtype=np.int64),
                                depth_reached=np.array([r.depth_reached for r in res], dtype=np.int32))
        for m in range(M):
            length, depth = int(res[m].length), int(res[m].depth_reached)
            plan = found = None
            if length >= 0 and res[m].status == 0:
                buf = (C.c_uint8 * max(length * A, 1))()
                if L.lle_cycleforest_plan(h, m, buf, length * A) != length:
                    raise RuntimeError(f"lle_cycleforest_plan failed (map {m}): {L.lle_cycleforest_last_error().decode()}")
                plan = [tuple(Action(int(buf[t * A + a])) for a in range(A)) for t in range(length)]
                words = (C.c_uint32 * LLE_CYCLES_VALUE_WORDS)()
                n_words = L.lle_cycleforest_value(h, m, words)
                if n_words != res[m].value_words:
                    raise RuntimeError(f"lle_cycleforest_value failed (map {m}): {L.lle_cycleforest_last_error().decode()}")
                found = triples(list(words)[:n_words], A)
            out.plans.append(plan)
            out.triples.append(found)
            out.closed_orders.append(None if found is None else sorted({len(s) for a, c, s in found if a == c}))
            cap = depth + 2
            frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
            n = L.lle_cycleforest_stats(h, m, frontier, expanded, cap)
            out.frontier.append([int(frontier[d]) for d in range(n)])
            out.expanded.append([int(expanded[d]) for d in range(n - 1)])
        valid, lanes = C.c_int64(0), C.c_int64(0)
        L.lle_cycleforest_occupancy(h, C.byref(valid), C.byref(lanes))
        out.valid_items, out.launched_lanes = int(valid.value), int(lanes.value)
        out.pieces = out.launched_lanes // (M * self.envs_per_map)
        return out

    def forget(self):
        """Drop the cached results of this solver and of the inner ones; the device handles stay (for whoever times a run)."""
        solver_ = self
        while solver_ is not None:
            solver_._cache.clear()
            solver_ = getattr(solver_, "_help", None) or getattr(solver_, "_inner", None)

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_cycleforest_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None
        inner = getattr(self, "_help", None)
        if inner is not None:
            inner.free()


# ------------------------------------------------------------------------------------------------ many worlds of any shapes
def _refuse(res, m, k, forest, mode):
    """Raise what the single solver raises for map m of the run (index k of the caller's list) when it has no answer."""
    mode = cycles._served_mode(mode)
    if mode.kind != "no-interdependence" or mode.n == 2 or mode.n > forest.n_agents:
        return _refuse_help(res, m, k, forest, mode)  # (the inner help forest's statuses)
    if res.status[m] == LLE_CYCLES_CAPACITY:
        raise SolverCapacityError(f"map {k}: more than max_states_per_map = {forest.max_states_per_map} distinct records at depth "
                                  f"{int(res.depth_reached[m])} in mode '{mode}': the search has no answer for it; pass a larger max_states_per_map")
    if res.status[m] == LLE_CYCLES_DENSE:
        raise RuntimeError(f"the closed-trail search has no answer for '{mode}': map {k}: the arcs of one state allow more than {LLE_CYCLES_WALK_BUDGET} "
                           "trail extensions")


def solve_many(worlds, t_max="auto", *, mode="standard", collect_gems=False, **options):
    """[CycleSolver(w, t_max).find_shortest(mode, collect_gems=collect_gems) for w in worlds], searched together: the worlds are grouped
    by shape, every group is one cycle forest, the answers come in input order.  `options`: envs_per_map, max_states_per_map, device.
    A map over capacity raises SolverCapacityError naming its index; a map whose walk runs out of budget the RuntimeError of
    `CycleSolver`."""
    mode = cycles._served_mode(mode)
    worlds, groups = _groups(worlds)
    answers = [None] * len(worlds)
    for indices in groups:
        forest = CycleForestSolver([worlds[k] for k in indices], t_max, **options)
        try:
            res = forest.run(mode, collect_gems)
            for m, k in enumerate(indices):
                _refuse(res, m, k, forest, mode)
                answers[k] = res.plans[m]
        finally:
            forest.free()
    return answers


class _CycleAnswered(_HelpAnswered):
    """Entry i of a ManyCycleCharacterization behind WorldCharacterizer's questions."""

    def is_interdependent(self, n_agents=2):
        return bool(self._many.is_interdependent(n_agents)[self._i])


class ManyCycleCharacterization(ManyHelpCharacterization):
    """`ManyHelpCharacterization` whose `is_interdependent(n)` is answered for every n >= 2: what `CycleCharacterizer(worlds[i],
    t_max).is_interdependent(n)` answers, for every i.  For n >= 3 only the maps whose answer is open are searched: cooperative ones
    (a plan without a help edge closes no trail), of at least n agents, whose shortest plan holds a closed trail of order n by its
    host-side profile -- the same cheap no as in `CycleCharacterizer`.  `profiler(i, plan)` -> the cooperation profile of world i's plan."""

    def __init__(self, t_max, n_agents, runner, profiler, *, sequential=True, free=None, forests=()):
        super().__init__(t_max, n_agents, runner, sequential=sequential, free=free, forests=forests)
        self._profiler, self._profiles, self._interdependent = profiler, {}, {}

    def _profile(self, i):
        if i not in self._profiles:
            self._profiles[i] = self._profiler(i, self.shortest_paths[i])
        return self._profiles[i]

    def is_interdependent(self, n_agents=2):
        if n_agents < 2:
            raise ValueError(f"Interdependence only makes sense for >= 2 agents. Got {n_agents}.")
        if n_agents not in self._interdependent:  # (every entry asks: the array of an order is worked out once)
            if n_agents == 2:
                answer = super().is_interdependent(2)
            else:
                open_ = self.cooperative & (n_agents <= self.n_agents)
                for i in np.flatnonzero(open_):
                    open_[i] = bool(self._profile(int(i)).is_interdependent(n_agents))
                answer = self._required(SolveMode.no_interdependence(n_agents), open_)
            self._interdependent[n_agents] = answer
        return self._interdependent[n_agents].copy()

    def forget(self):
        """Drop every answer, plan and profile, here and in the forests behind; the device handles stay (for whoever times the runs)."""
        self._plans.clear()
        self._profiles.clear()
        self._interdependent.clear()
        self.runs.clear()
        for forest in self.forests:
            forest.forget()

    def entry(self, i, world=None):
        if not 0 <= i < len(self):
            raise IndexError(i)
        return _CycleAnswered(self, i, world)


def characterize_many(worlds, t_max, *, sequential=True, **options):
    """`ManyCycleCharacterization` of the worlds at the horizon t_max: per shape one cycle forest, made now (no device work yet) and
    run once per mode that is asked for.  `options`: envs_per_map, max_states_per_map, device."""
    from .helpgraph import profile_plan
    from .world import World
    worlds, groups = _groups(worlds)
    forests = [(indices, CycleForestSolver([worlds[k] for k in indices], t_max, **options)) for indices in groups]
    where = {k: (forest, m) for indices, forest in forests for m, k in enumerate(indices)}

    def runner(mode, only):
        plans = [None] * len(worlds)
        for indices, forest in forests:
            mask = only[indices]
            if not mask.any():
                continue
            res = forest.run(mode, only=None if mask.all() else mask)
            many.runs.append((str(mode), res))
            for m, k in enumerate(indices):
                if mask[m]:
                    _refuse(res, m, k, forest, mode)
                    plans[k] = res.plans[m]
        return plans

    def profiler(i, plan):
        forest, m = where[i]  # (replayed on a world of the forest's frozen map, as CycleCharacterizer replays on its solver's)
        return profile_plan(World(None, _map=forest._maps[m].clone()), plan)

    def free():
        for _indices, forest in forests:
            forest.free()

    t = forests[0][1].t_max if forests else t_max
    many = ManyCycleCharacterization(t, [w.n_agents for w in worlds], runner, profiler, sequential=sequential, free=free, forests=[f for _indices, f in forests])
    return many


__all__ = ["CycleForestSolver", "CycleForestResult", "ManyCycleCharacterization", "solve_many", "characterize_many"]
