"""ctypes binding of liblle_forest.so (lle_amd/forest/forest.hip, C ABI include/lle_forest.h) and what a
filtered generator needs over it: `ForestSolver`, `solve_many`, `characterize_many`.

`lle_amd.solver.Solver` answers for one map per handle; a level of its search is four launches and one host read for a few thousand
work items.  A generator that keeps the candidates a constraint accepts runs hundreds of such searches on equally shaped maps.  The
forest walks all their trees depth by depth in the same launches -- one batch made with lle_batch_create_multi, a segment of every
array per map -- and is, per map, exactly the single search: the same lengths, per-depth counters and stored states.

    plans = solve_many(worlds, 10)                       # [Solver(w, 10).find_shortest() for w in worlds]
    c = characterize_many(worlds, 10)                    # c.solvable, c.cooperative, c.independent: boolean arrays
    ForestSolver(worlds, 10, envs_per_map=64).run("no-cooperation").length

Which of several shortest plans comes back may differ between runs; lengths and counters do not.  No fallback: a missing library raises.
"""
import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

from . import _binding, _capi
from .solver import (LLE_SEARCH_CAPACITY, LLE_SEARCH_MAX_AGENTS, _NATIVE, SearchArgs, SolverCapacityError, _as_world, _device_index, _native_mode)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_forest.so")

EXPORTS = ["lle_forest_create", "lle_forest_free", "lle_forest_run", "lle_forest_plan", "lle_forest_stats", "lle_forest_occupancy",
           "lle_forest_last_error", "lle_forest_debug_launched", "lle_forest_debug_compiled"]
KERNELS = ["forest_commit", "forest_expand", "forest_insert<false>", "forest_insert<true>", "forest_plans", "forest_roots", "forest_seed"]


class ForestOptions(C.Structure):
    """lle_forest_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("envs_per_map", C.c_int64), ("max_states_per_map", C.c_int64), ("stream", C.c_void_p)]


class ForestMapResult(C.Structure):
    """lle_forest_result."""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("pad", C.c_int32)]


_lib = None


def lib():
    """Load liblle_forest.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the forest search.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_forest_create.restype = vp
    L.lle_forest_create.argtypes = [C.POINTER(vp), i32, C.POINTER(ForestOptions)]
    L.lle_forest_free.restype = None
    L.lle_forest_free.argtypes = [vp]
    L.lle_forest_run.restype = i32
    L.lle_forest_run.argtypes = [vp, C.POINTER(SearchArgs), C.POINTER(ForestMapResult)]
    L.lle_forest_plan.restype = i32
    L.lle_forest_plan.argtypes = [vp, i32, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_forest_stats.restype = i32
    L.lle_forest_stats.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_forest_occupancy.restype = i32
    L.lle_forest_occupancy.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lle_forest_last_error.restype = C.c_char_p
    L.lle_forest_last_error.argtypes = []
    for fn in (L.lle_forest_debug_launched, L.lle_forest_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_forest.so this process has launched (lle_forest_debug_launched)."""
    return _binding.names(lib().lle_forest_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_forest_debug_compiled)."""
    return _binding.names(lib().lle_forest_debug_compiled)


# ------------------------------------------------------------------------------------------------ shapes
_SHAPE = (("height", "height"), ("width", "width"), ("n_agents", "number of agents"), ("n_sources", "number of laser sources"), ("n_gems", "number of gems"))


def shape_key(map_):
    """What lle_batch_create_multi wants the maps of one batch to agree on: height, width, numbers of agents, sources and gems, the
    beam words of every source (a beam longer than 32 cells takes more than one) and the row alignment."""
    words = tuple(max(1, -(-int(s.length) // 32)) for s in map_.sources())
    return tuple(getattr(map_, name) for name, _ in _SHAPE) + (words, map_.obs_stride)


def _mismatch(first, other):
    """In what `other` differs from `first` (Maps), or None."""
    for name, label in _SHAPE:
        if getattr(first, name) != getattr(other, name):
            return f"{label} ({getattr(other, name)}, map 0 has {getattr(first, name)})"
    a, b = shape_key(first), shape_key(other)
    if a[-2] != b[-2]:
        return f"layout of the beam words ({list(b[-2])} words per source, map 0 has {list(a[-2])})"
    if a[-1] != b[-1]:
        return f"row alignment (an observation row of {b[-1]} bytes, map 0 has {a[-1]})"
    return None


# ------------------------------------------------------------------------------------------------ ForestSolver
@dataclass
class ForestResult:
    """One run of a forest.  Arrays have one entry per map, in the order given to ForestSolver."""
    length: np.ndarray          # int32: joint actions of the shortest plan, -1: none within t_max (or no answer)
    status: np.ndarray          # int32: 0, or LLE_SEARCH_CAPACITY for a map that met more than max_states_per_map states
    n_states: np.ndarray        # int64
    depth_reached: np.ndarray   # int32
    frontier: list = field(default_factory=list)   # per map: states first reached at depth d
    expanded: list = field(default_factory=list)   # per map: available joint actions over the states of depth d
    plans: list = field(default_factory=list)      # per map: rows of Action tuples, or None
    valid_items: int = 0        # lanes that served a work item
    launched_lanes: int = 0     # pieces * n_maps * envs_per_map, over the levels
    pieces: int = 0             # pieces of the run, four launches each

    @property
    def occupancy(self):
        """valid_items / launched_lanes of the run (0.0 for a run without a launch)."""
        return self.valid_items / self.launched_lanes if self.launched_lanes else 0.0


class ForestSolver:
    """Shortest joint plans of many equally shaped worlds up to the horizon `t_max` ("auto": (width * height) // 2), searched together.

    `worlds`: lle_amd.Worlds, Maps or map texts that agree on height, width, the numbers of agents, sources and gems, the layout of
    their beam words and the row alignment (ValueError names the first that does not match map 0, and in what).  FROZEN at
    construction like `Solver`: it keeps its own copies of the maps as they are now.  `envs_per_map`: environments per map = work items
    of a map per piece; `max_states_per_map`: records of every map's pool segment -- a map beyond it has status LLE_SEARCH_CAPACITY in
    the result and no answer, the others are untouched.  The device handle is made by the first run and freed with the ForestSolver."""

    def __init__(self, worlds, t_max="auto", *, envs_per_map=256, max_states_per_map=1 << 16, device=None):
        self.worlds = [_as_world(w) for w in worlds]
        if not self.worlds:
            raise ValueError("a forest needs at least one world")
        first = self.worlds[0]
        self.t_max = (first.width * first.height) // 2 if isinstance(t_max, str) and t_max == "auto" else int(t_max)
        if self.t_max < 0:
            raise ValueError(f"t_max must be non-negative, got {self.t_max}.")
        if int(envs_per_map) < 1 or int(max_states_per_map) < 1:
            raise ValueError("envs_per_map and max_states_per_map must be at least 1")
        if first.n_agents > LLE_SEARCH_MAX_AGENTS:
            raise ValueError(f"the search serves maps of at most {LLE_SEARCH_MAX_AGENTS} agents (5^A joint actions per state); map 0 has {first.n_agents}")
        for k, w in enumerate(self.worlds):
            batch = getattr(w, "_batch_obj", None)
            if batch is not None and getattr(batch, "_env_sources", False):
                raise ValueError(f"map {k} keeps per-environment sources: the search runs on the map's own source colours and flags")
            what = _mismatch(first._map, w._map)
            if what is not None:
                raise ValueError(f"map {k} does not match map 0 in {what}: the maps of a forest share one batch")
        self.envs_per_map, self.max_states_per_map = int(envs_per_map), int(max_states_per_map)
        self._device = _device_index(device if device is not None else getattr(first, "_device", None))
        self._maps = [w._map.clone() for w in self.worlds]  # frozen: later changes of the worlds do not reach this ForestSolver
        self.n_maps, self.n_agents = len(self._maps), first.n_agents
        self.h = None
        self._cache = {}

    def _handle(self):
        if self.h is None:
            L = lib()
            opt = ForestOptions(C.sizeof(ForestOptions), self._device, self.envs_per_map, self.max_states_per_map, None)
            handles = (C.c_void_p * self.n_maps)(*[m.h for m in self._maps])
            self.h = L.lle_forest_create(handles, self.n_maps, C.byref(opt))
            if not self.h:
                message = L.lle_forest_last_error().decode()
                if "must agree" in message:
                    raise ValueError(f"lle_forest_create failed: {message}")
                raise RuntimeError(f"lle_forest_create failed: {message}")
        return self.h

    def run(self, mode="standard", collect_gems=False):
        """One search of every map in `mode` ("standard" / "no-cooperation"); the ForestResult is cached per (mode, collect_gems)."""
        from .world import Action
        mode = _native_mode(mode)
        key = (str(mode), bool(collect_gems))
        if key in self._cache:
            return self._cache[key]
        L, h, M, A = lib(), self._handle(), self.n_maps, self.n_agents
        args = SearchArgs(C.sizeof(SearchArgs), _NATIVE[mode.kind], int(bool(collect_gems)), self.t_max)
        res = (ForestMapResult * M)()
        rc = L.lle_forest_run(h, C.byref(args), res)
        if rc != 0:
            raise RuntimeError(f"lle_forest_run failed ({rc}): {L.lle_forest_last_error().decode()}")
        out = ForestResult(length=np.array([r.length for r in res], dtype=np.int32), status=np.array([r.status for r in res], dtype=np.int32),
                           n_states=np.array([r.n_states for r in res], dtype=np.int64), depth_reached=np.array([r.depth_reached for r in res], dtype=np.int32))
        for m in range(M):
            length, depth = int(res[m].length), int(res[m].depth_reached)
            plan = None
            if length >= 0 and res[m].status == 0:
                buf = (C.c_uint8 * max(length * A, 1))()
                if L.lle_forest_plan(h, m, buf, length * A) != length:
                    raise RuntimeError(f"lle_forest_plan failed (map {m}): {L.lle_forest_last_error().decode()}")
                plan = [tuple(Action(int(buf[t * A + a])) for a in range(A)) for t in range(length)]
            out.plans.append(plan)
            cap = depth + 2
            frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
            n = L.lle_forest_stats(h, m, frontier, expanded, cap)
            out.frontier.append([int(frontier[d]) for d in range(n)])
            out.expanded.append([int(expanded[d]) for d in range(n - 1)])
        valid, lanes = C.c_int64(0), C.c_int64(0)
        L.lle_forest_occupancy(h, C.byref(valid), C.byref(lanes))
        out.valid_items, out.launched_lanes = int(valid.value), int(lanes.value)
        out.pieces =out.launched_lanes // (M * self.envs_per_map)
        self._cache[key] = out
        return out

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_forest_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()


# ------------------------------------------------------------------------------------------------ many worlds of any shapes
def _groups(worlds):
    """[(indices into worlds, their Worlds)] per shape, in order of first appearance."""
    worlds = [_as_world(w) for w in worlds]
    groups = {}
    for k, w in enumerate(worlds):
        groups.setdefault(shape_key(w._map), []).append(k)
    return worlds, list(groups.values())


def _run_groups(worlds, t_max, modes, collect_gems, options):
    """{mode: [(length or None, plan or None)] in input order}: one forest per shape, one run per mode."""
    worlds, groups = _groups(worlds)
    answers = {mode: [None] * len(worlds) for mode in modes}
    for indices in groups:
        forest = ForestSolver([worlds[k] for k in indices], t_max, **options)
        try:
            for mode in modes:
                res = forest.run(mode, collect_gems)
                for m, k in enumerate(indices):
                    if res.status[m] == LLE_SEARCH_CAPACITY:
                        raise SolverCapacityError(f"map {k}: more than max_states_per_map = {forest.max_states_per_map} distinct states at depth "
                                                  f"{int(res.depth_reached[m])} in mode '{mode}': the search has no answer for it; pass a larger max_states_per_map")
                    answers[mode][k] = res.plans[m]
        finally:
            forest.free()
    return answers


def solve_many(worlds, t_max="auto", *, mode="standard", collect_gems=False, **options):
    """[Solver(w, t_max).find_shortest(mode, collect_gems=collect_gems) for w in worlds], searched together: the worlds are grouped by
    shape, every group is one forest, the answers come in input order.  `options`: envs_per_map, max_states_per_map, device.  A map over
    capacity raises SolverCapacityError naming its index."""
    mode = _native_mode(mode)
    return _run_groups(worlds, t_max, [str(mode)], collect_gems, options)[str(mode)]


class ManyCharacterization:
    """What `WorldCharacterizer(worlds[i], t_max)` answers, for every i: boolean arrays `solvable`, `cooperative`, `independent`; int
    arrays `shortest_length`, `shortest_independent_length` (-1: none); `shortest_paths`, `shortest_independent_paths` (plans or None)."""

    def __init__(self, t_max, shortest_paths, shortest_independent_paths):
        self.t_max = t_max
        self.shortest_paths, self.shortest_independent_paths = shortest_paths, shortest_independent_paths
        self.shortest_length = np.array([-1 if p is None else len(p) for p in shortest_paths], dtype=np.int32)
        self.shortest_independent_length = np.array([-1 if p is None else len(p) for p in shortest_independent_paths], dtype=np.int32)
        self.solvable = self.shortest_length >= 0
        self.independent = self.solvable & (self.shortest_independent_length >= 0)
        self.cooperative = self.solvable & ~self.independent

    def __len__(self):
        return len(self.shortest_paths)


def characterize_many(worlds, t_max, **options):
    """`ManyCharacterization` of the worlds at the horizon t_max: per shape one forest and two runs ("standard", "no-cooperation")."""
    answers = _run_groups(worlds, t_max, ["standard", "no-cooperation"], False, options)
    return ManyCharacterization(t_max, answers["standard"], answers["no-cooperation"])


__all__ = ["ForestSolver", "ForestResult", "ManyCharacterization", "solve_many", "characterize_many"]
