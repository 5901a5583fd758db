"""ctypes binding of liblle_helpforest.so (lle_amd/helpforest/helpforest.hip, C ABI include/lle_helpforest.h)
and what a filtered generator needs over it: `HelpForestSolver`, `solve_many`, `characterize_many`.

`lle_amd.forest` walks the plain search of many equally shaped maps in the same launches; `HelpGraphSolver` and `TrailSolver` answer the
solve modes that depend on who has helped whom, one map per handle.  The help forest is both: one batch made with
lle_batch_create_multi, a segment of every array per map, records that carry the help relation or the trail lengths of their
trajectory -- and, per map, exactly the single search: the same lengths, per-depth counters and stored records.

    HelpForestSolver(worlds, 10).run("no-asymmetric").length           # per map; -1: every plan has an asymmetric edge (or none exists)
    plans = solve_many(worlds, 10, mode="no-sequence-3")               # [TrailSolver(w, 10).find_shortest("no-sequence-3") for w in worlds]
    with characterize_many(worlds, 10) as c:                           # what TrailCharacterizer(w, 10) answers, as boolean arrays
        keep = c.is_asymmetric() & ~c.is_sequential(3)

Modes: everything `TrailSolver` serves; "no-cooperation" is answered by an inner `ForestSolver`, "no-interdependence-N" for N >= 3
raises NotImplementedError here: the cycle forest (`lle_amd.cycleforest`, over this one) serves it.  Which of several shortest plans comes back may differ between runs; lengths and counters do not.  No
fallback: a missing library raises.
"""
import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

from . import _capi, helpgraph, solver, trails
from .characterization import WorldCharacterizer
from .forest import ForestResult, ForestSolver, _groups
from .helpgraph import LLE_HELPGRAPH_CAPACITY, help_edges
from .solver import SolveMode, SolverCapacityError
from .trails import LLE_TRAILS_DENSE, LLE_TRAILS_WALK_BUDGET, trail_lengths

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_helpforest.so")

# include/lle_helpforest.h
LLE_HELPFOREST_NO_SEQUENCE = 6
LLE_HELPFOREST_MAX_AGENTS = 6
LLE_HELPFOREST_MAX_SOURCES = 32

EXPORTS = ["lle_helpforest_create", "lle_helpforest_free", "lle_helpforest_run", "lle_helpforest_plan", "lle_helpforest_stats", "lle_helpforest_occupancy",
           "lle_helpforest_last_error", "lle_helpforest_debug_launched", "lle_helpforest_debug_compiled"]
KERNELS = ["hf_commit<help>", "hf_commit<trail>", "hf_expand", "hf_insert<help>", "hf_insert<trail>", "hf_plans", "hf_roots", "hf_seed<help>", "hf_seed<trail>"]


class HelpForestOptions(C.Structure):
    """lle_helpforest_options."""
    _fields_ = [("struct_bytes", C.c_uint32), ("device", C.c_int32), ("envs_per_map", C.c_int64), ("max_states_per_map", C.c_int64), ("stream", C.c_void_p)]


class HelpForestArgs(C.Structure):
    """lle_helpforest_args."""
    _fields_ = [("struct_bytes", C.c_uint32), ("mode", C.c_int32), ("param", C.c_int32), ("collect_gems", C.c_int32), ("t_max", C.c_int32)]


class HelpForestMapResult(C.Structure):
    """lle_helpforest_result."""
    _fields_ = [("status", C.c_int32), ("length", C.c_int32), ("n_states", C.c_int64), ("depth_reached", C.c_int32), ("help_lo", C.c_uint32),
                ("help_hi", C.c_uint32), ("trail", C.c_uint32)]


_lib = None


def lib():
    """Load liblle_helpforest.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`.  "
                          "lle_amd has no fallback for the help forest.")
    L = C.CDLL(LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.lle_helpforest_create.restype = vp
    L.lle_helpforest_create.argtypes = [C.POINTER(vp), i32, C.POINTER(HelpForestOptions)]
    L.lle_helpforest_free.restype = None
    L.lle_helpforest_free.argtypes = [vp]
    L.lle_helpforest_run.restype = i32
    L.lle_helpforest_run.argtypes = [vp, C.POINTER(HelpForestArgs), C.POINTER(C.c_uint8), C.POINTER(HelpForestMapResult)]
    L.lle_helpforest_plan.restype = i32
    L.lle_helpforest_plan.argtypes = [vp, i32, C.POINTER(C.c_uint8), C.c_int64]
    L.lle_helpforest_stats.restype = i32
    L.lle_helpforest_stats.argtypes = [vp, i32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32]
    L.lle_helpforest_occupancy.restype = i32
    L.lle_helpforest_occupancy.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.lle_helpforest_last_error.restype = C.c_char_p
    L.lle_helpforest_last_error.argtypes = []
    for fn in (L.lle_helpforest_debug_launched, L.lle_helpforest_debug_compiled):
        fn.restype = C.c_size_t
        fn.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_helpforest.so this process has launched (lle_helpforest_debug_launched)."""
    return solver._names(lib().lle_helpforest_debug_launched)


def compiled_kernels():
    """Every kernel the library holds (lle_helpforest_debug_compiled)."""
    return solver._names(lib().lle_helpforest_debug_compiled)


def native_mode(mode):
    """(mode constant, param) of include/lle_helpforest.h for a SolveMode the library itself serves."""
    if mode.kind == "no-sequence":
        return LLE_HELPFOREST_NO_SEQUENCE, mode.n
    return helpgraph._NATIVE[mode.kind], mode.n or 2


# ------------------------------------------------------------------------------------------------ HelpForestSolver
@dataclass
class HelpForestResult(ForestResult):
    """One run of a help forest: `ForestResult` (status: 0, LLE_HELPGRAPH_CAPACITY, or LLE_TRAILS_DENSE for a map one of whose states
    allows more trail extensions than the walk's budget), and per map what the goal's record carries."""
    help_edges: list = field(default_factory=list)   # per map: the (helper, beneficiary) pairs of the plan, None without a plan or in a trail mode
    trail: list = field(default_factory=list)        # per map: per-agent longest trail ending at the agent ("no-sequence-N"), else None


class HelpForestSolver(ForestSolver):
    """`ForestSolver` over liblle_helpforest.so: shortest joint plans of many equally shaped worlds up to the horizon `t_max` under a
    solve mode of `TrailSolver`, searched together.  Same arguments, same refusals (shape mismatch, per-environment sources, more than
    6 agents -- and more than 32 sources), same freezing at construction.  `max_states_per_map` counts (world state, help relation) or
    (world state, trail lengths) records."""

    def __init__(self, worlds, t_max="auto", *, envs_per_map=256, max_states_per_map=1 << 16, device=None):
        super().__init__(worlds, t_max, envs_per_map=envs_per_map, max_states_per_map=max_states_per_map, device=device)
        for k, m in enumerate(self._maps):
            if m.n_sources > LLE_HELPFOREST_MAX_SOURCES:
                raise ValueError(f"the help forest serves maps of at most {LLE_HELPFOREST_MAX_SOURCES} laser sources (one bit per source in a cell's "
                                 f"word); map {k} has {m.n_sources}")
        self._inner = None  # the ForestSolver that answers "no-cooperation", made when it is asked for

    def _handle(self):
        if self.h is None:
            L = lib()
            opt = HelpForestOptions(C.sizeof(HelpForestOptions), self._device, self.envs_per_map, self.max_states_per_map, None)
            handles = (C.c_void_p * self.n_maps)(*[m.h for m in self._maps])
            self.h = L.lle_helpforest_create(handles, self.n_maps, C.byref(opt))
            if not self.h:
                message = L.lle_helpforest_last_error().decode()
                if "must agree" in message:
                    raise ValueError(f"lle_helpforest_create failed: {message}")
                raise RuntimeError(f"lle_helpforest_create failed: {message}")
        return self.h

    def _mask(self, only):
        if only is None:
            return None
        mask = np.ascontiguousarray(np.asarray(only, dtype=bool))
        if mask.shape != (self.n_maps,):
            raise ValueError(f"`only` must have one entry per map ({self.n_maps}), got shape {mask.shape}")
        return mask

    def _no_cooperation(self, collect_gems, mask):
        if self._inner is None:
            self._inner = ForestSolver(self._maps, self.t_max, envs_per_map=self.envs_per_map, max_states_per_map=self.max_states_per_map,
                                       device=None if self._device < 0 else self._device)
        res = self._inner.run("no-cooperation", collect_gems)
        out = HelpForestResult(length=res.length.copy(), status=res.status.copy(), n_states=res.n_states.copy(), depth_reached=res.depth_reached.copy(),
                               frontier=[list(f) for f in res.frontier], expanded=[list(e) for e in res.expanded], plans=list(res.plans),
                               valid_items=res.valid_items, launched_lanes=res.launched_lanes, pieces=res.pieces,
                               help_edges=[None] * self.n_maps, trail=[None] * self.n_maps)
        for m in range(self.n_maps):
            if mask is not None and not mask[m]:  # (the plain forest has no mask: what it found for the others is left out)
                out.length[m], out.status[m], out.n_states[m], out.depth_reached[m] = -1, 0, 0, 0
                out.frontier[m], out.expanded[m], out.plans[m] = [], [], None
        return out

    def run(self, mode="standard", collect_gems=False, only=None):
        """One search of every map in `mode`; `only`: a boolean per map, False = not searched (idle from the first level: length -1,
        n_states 0, depth_reached 0, status 0).  The HelpForestResult is cached per (mode, collect_gems) when `only` is None."""
        from .world import Action
        mode = trails._served_mode(mode)
        mask = self._mask(only)
        key = (str(mode), bool(collect_gems))
        if mask is None and key in self._cache:
            return self._cache[key]
        if mode.kind == "no-cooperation":
            out = self._no_cooperation(collect_gems, mask)
        else:
            L, h, M, A = lib(), self._handle(), self.n_maps, self.n_agents
            native, param = native_mode(mode)
            args = HelpForestArgs(C.sizeof(HelpForestArgs), native, param, int(bool(collect_gems)), self.t_max)
            res = (HelpForestMapResult * M)()
            search = None if mask is None else (C.c_uint8 * M)(*[int(v) for v in mask])
            rc = L.lle_helpforest_run(h, C.byref(args), search, res)
            if rc != 0:
                raise RuntimeError(f"lle_helpforest_run failed ({rc}): {L.lle_helpforest_last_error().decode()}")
            out = HelpForestResult(length=np.array([r.length for r in res], dtype=np.int32), status=np.array([r.status for r in res], dtype=np.int32),
                                   n_states=np.array([r.n_states for r in res], dtype=np.int64),
                                   depth_reached=np.array([r.depth_reached for r in res], dtype=np.int32))
            sequence = mode.kind == "no-sequence"
            for m in range(M):
                length, depth = int(res[m].length), int(res[m].depth_reached)
                plan = None
                if length >= 0 and res[m].status == 0:
                    buf = (C.c_uint8 * max(length * A, 1))()
                    if L.lle_helpforest_plan(h, m, buf, length * A) != length:
                        raise RuntimeError(f"lle_helpforest_plan failed (map {m}): {L.lle_helpforest_last_error().decode()}")
                    plan = [tuple(Action(int(buf[t * A + a])) for a in range(A)) for t in range(length)]
                out.plans.append(plan)
                out.help_edges.append(None if plan is None or sequence else help_edges(res[m].help_lo, res[m].help_hi))
                out.trail.append(None if plan is None or not sequence else trail_lengths(res[m].trail, A))
                cap = depth + 2
                frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
                n = L.lle_helpforest_stats(h, m, frontier, expanded, cap)
                out.frontier.append([int(frontier[d]) for d in range(n)])
                out.expanded.append([int(expanded[d]) for d in range(n - 1)])
            valid, lanes = C.c_int64(0), C.c_int64(0)
            L.lle_helpforest_occupancy(h, C.byref(valid), C.byref(lanes))
            out.valid_items, out.launched_lanes = int(valid.value), int(lanes.value)
            out.pieces = out.launched_lanes // (M * self.envs_per_map)
        if mask is None:
            self._cache[key] = out
        return out

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_helpforest_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None
        inner = getattr(self, "_inner", None)
        if inner is not None:
            inner.free()


# ------------------------------------------------------------------------------------------------ many worlds of any shapes
def _refuse(res, m, k, forest, mode):
    """Raise what the single solver raises for map m of the run (index k of the caller's list) when it has no answer."""
    if res.status[m] == LLE_HELPGRAPH_CAPACITY:
        raise SolverCapacityError(f"map {k}: more than max_states_per_map = {forest.max_states_per_map} distinct records at depth "
                                  f"{int(res.depth_reached[m])} in mode '{mode}': the search has no answer for it; pass a larger max_states_per_map")
    if res.status[m] == LLE_TRAILS_DENSE:
        raise RuntimeError(f"the trail search has no answer for '{mode}': map {k}: the arcs of one state allow more than {LLE_TRAILS_WALK_BUDGET} "
                           "trail extensions")


def solve_many(worlds, t_max="auto", *, mode="standard", collect_gems=False, **options):
    """[TrailSolver(w, t_max).find_shortest(mode, collect_gems=collect_gems) for w in worlds], searched together: the worlds are grouped
    by shape, every group is one help forest, the answers come in input order.  `options`: envs_per_map, max_states_per_map, device.
    A map over capacity raises SolverCapacityError naming its index; a map whose walk runs out of budget the RuntimeError of
    `TrailSolver`."""
    mode = trails._served_mode(mode)
    worlds, groups = _groups(worlds)
    answers = [None] * len(worlds)
    for indices in groups:
        forest = HelpForestSolver([worlds[k] for k in indices], t_max, **options)
        try:
            res = forest.run(mode, collect_gems)
            for m, k in enumerate(indices):
                _refuse(res, m, k, forest, mode)
                answers[k] = res.plans[m]
        finally:
            forest.free()
    return answers


class _HelpAnswered(WorldCharacterizer):
    """Entry i of a ManyHelpCharacterization behind WorldCharacterizer's questions."""

    def __init__(self, many, i, world=None):  # (no Solver: the forests answer)
        self._many, self._i = many, i
        self.world, self.t_max = world, many.t_max

    @property
    def shortest_path(self):
        return self._many.shortest_paths[self._i]

    @property
    def shortest_independent_path(self):
        return self._many.shortest_independent_paths[self._i]

    def is_asymmetric(self):
        return bool(self._many.is_asymmetric()[self._i])

    def is_fully_coupled(self):
        return bool(self._many.is_fully_coupled()[self._i])

    def is_convergent(self, k=2):
        return bool(self._many.is_convergent(k)[self._i])

    def is_divergent(self, k=2):
        return bool(self._many.is_divergent(k)[self._i])

    def is_interdependent(self, n_agents=2):
        if n_agents > 2:
            return super().is_interdependent(n_agents)  # raises: a closed trail over N >= 3 agents is not built
        return bool(self._many.is_interdependent(n_agents)[self._i])

    def is_mutual(self):
        return self.is_interdependent(2)

    def is_sequential(self, length=2):
        if not self._many.sequential:
            return super().is_sequential(length)  # raises, as HelpGraphCharacterizer's does
        return bool(self._many.is_sequential(length)[self._i])


class ManyHelpCharacterization:
    """What `TrailCharacterizer(worlds[i], t_max)` answers, for every i, as boolean arrays: `solvable`, `cooperative`, `independent`,
    and the methods is_asymmetric(), is_fully_coupled(), is_mutual(), is_interdependent(2), is_convergent(k), is_divergent(k),
    is_sequential(n).  A predicate holds for a world that is solvable within t_max and has NO plan within t_max that avoids the shape.
    Every method runs at most one forest run per shape group and mode, on first use, and asks only for the maps whose answer is not
    decided already: an unsolvable map, a map with an independent plan (a plan without a help edge avoids every shape) and a map with
    too few agents for k are False without a search.

    `runner(mode, only)` -> one plan or None per world (None where `only` is False); `n_agents`: per world.  `sequential=False`:
    `entry(i).is_sequential` raises as `HelpGraphCharacterizer`'s does.  A context manager; `free()` releases the forests' handles."""

    def __init__(self, t_max, n_agents, runner, *, sequential=True, free=None, forests=()):
        self.t_max, self.sequential = t_max, sequential
        self.n_agents = np.asarray(n_agents, dtype=np.int64)
        self._runner, self._free, self._plans = runner, free, {}
        self.forests = list(forests)  # the HelpForestSolvers behind the runner, one per shape (for whoever wants their handles or statistics)
        self.runs = []                # (mode text, HelpForestResult) of every forest run so far, in order

    def __len__(self):
        return len(self.n_agents)

    def _ask(self, mode, only):
        """The plans in `mode` (a SolveMode) of the worlds `only` asks for, searched once."""
        key = str(mode)
        if key not in self._plans:
            only = np.asarray(only, dtype=bool)
            self._plans[key] = list(self._runner(mode, only)) if only.any() else [None] * len(self)
        return self._plans[key]

    def _found(self, mode, only):
        return np.array([p is not None for p in self._ask(mode, only)], dtype=bool)

    @property
    def shortest_paths(self):
        return self._ask(SolveMode.standard(), np.ones(len(self), dtype=bool))

    @property
    def shortest_independent_paths(self):
        return self._ask(SolveMode.no_cooperation(), self.solvable)

    @property
    def solvable(self):
        return np.array([p is not None for p in self.shortest_paths], dtype=bool)

    @property
    def independent(self):
        return self.solvable & self._found(SolveMode.no_cooperation(), self.solvable)

    @property
    def cooperative(self):
        return self.solvable & ~self.independent

    def _required(self, mode, candidates=None):
        """The worlds of `candidates` (default: the cooperative ones) without a plan in `mode`."""
        candidates = self.cooperative if candidates is None else candidates
        return candidates & ~self._found(mode, candidates)

    def is_asymmetric(self):
        return self._required(SolveMode.no_asymmetric())

    def is_fully_coupled(self):
        return self._required(SolveMode.no_fully_coupled())

    def is_convergent(self, k=2):
        if k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {k}.")
        return self._required(SolveMode.no_convergence(k), self.cooperative & (k < self.n_agents))

    def is_divergent(self, k=2):
        if k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {k}.")
        return self._required(SolveMode.no_divergence(k), self.cooperative & (k < self.n_agents))

    def is_interdependent(self, n_agents=2):
        if n_agents < 2:
            raise ValueError(f"Interdependence only makes sense for >= 2 agents. Got {n_agents}.")
        mode = trails._served_mode(SolveMode.no_interdependence(n_agents))  # raises for N >= 3
        return self._required(mode)

    def is_mutual(self):
        return self.is_interdependent(2)

    def is_sequential(self, length=2):
        if length < 2:
            raise ValueError(f"Sequence length must be >= 2, got {length}.")
        mode = trails._served_mode(SolveMode.no_sequence(length))  # raises beyond 16
        return self._required(mode)

    def entry(self, i, world=None):
        """Entry i behind `WorldCharacterizer`'s questions, answered from the arrays (a question asked first runs the forests)."""
        if not 0 <= i < len(self):
            raise IndexError(i)
        return _HelpAnswered(self, i, world)

    def free(self):
        if self._free is not None:
            self._free()
            self._free = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def characterize_many(worlds, t_max, *, sequential=True, **options):
    """`ManyHelpCharacterization` of the worlds at the horizon t_max: per shape one help forest, made now (no device work yet) and
    run once per mode that is asked for.  `options`: envs_per_map, max_states_per_map, device."""
    worlds, groups = _groups(worlds)
    forests = [(indices, HelpForestSolver([worlds[k] for k in indices], t_max, **options)) for indices in groups]

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

    def free():
        for _indices, forest in forests:
            forest.free()

    t = forests[0][1].t_max if forests else t_max
    many = ManyHelpCharacterization(t, [w.n_agents for w in worlds], runner, sequential=sequential, free=free, forests=[f for _indices, f in forests])
    return many


__all__ = ["HelpForestSolver", "HelpForestResult", "ManyHelpCharacterization", "solve_many", "characterize_many"]
