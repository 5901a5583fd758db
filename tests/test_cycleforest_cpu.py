"""The cycle forest without a GPU: header / exports / binding of liblle_cycleforest.so, every host-side refusal, CycleForestSolver's
argument errors and routing against a stubbed library, ManyCycleCharacterization over hand-made answers, the generator's path for
CycleCharacterizer, the fixed input sets against the figures the issue states and the golden file against the restatement, and the
insert and commit bodies over cl::CycleKind under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/hostsim/cycleforest_pieces.cpp).  The search itself runs on the MI355X (tests/test_gpu_cycleforest.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lle_amd
from lle_amd import Map, World, cycleforest, cycles, forest, generator, helpforest, solver
from lle_amd.generator import Constraint, Cooperative, Interdependent
from tests import cycleforest_ref
from tests.cycleforest_ref import SET_F, SET_M, SET_T, SET_X, SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "S0 . . X"
THREE = "S0 S1 S2 X X X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
GOLDEN = cycleforest_ref.load_golden()


def handles(maps):
    return (C.c_void_p * len(maps))(*[m.h for m in maps])


def options(envs_per_map=0, max_states_per_map=0, struct_bytes=None, device=-1):
    return cycleforest.CycleForestOptions(C.sizeof(cycleforest.CycleForestOptions) if struct_bytes is None else struct_bytes, device, envs_per_map,
                                          max_states_per_map, None)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_exports_sizes_and_constants():
    """liblle_cycleforest.so exports every function include/lle_cycleforest.h declares, and the binding knows exactly those; the header
    is plain C; struct sizes, field offsets and constants of the binding are the header's."""
    L = cycleforest.lib()
    header = open(os.path.join(ROOT, "include", "lle_cycleforest.h")).read()
    declared = set(re.findall(r"\b(lle_cycleforest_[a-z_0-9]+)\s*\(", header))
    assert declared == set(cycleforest.EXPORTS) and len(cycleforest.EXPORTS) == 10
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "cycleforest", "cycleforest.hip")).read()
    assert '#include "../../include/lle_cycleforest.h"' in source and '#include "../forest/forest_core.hpp"' in source and '#include "../cycles/cycles_logic.hpp"' in source
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    for foreign in ("lle_cycles_create", "lle_helpforest_create", "lle_forest_create", "lle_search_create"):
        assert foreign not in source  # no symbol of the single-map library or of the other forests
    assert "__syncthreads" not in source  # no staged table, no barrier: an idle lane may return at once
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "lle_cycleforest.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d", '
            'sizeof(lle_cycleforest_options), sizeof(lle_cycleforest_args), sizeof(lle_cycleforest_result), offsetof(lle_cycleforest_options, stream), '
            'offsetof(lle_cycleforest_args, t_max), offsetof(lle_cycleforest_result, n_states), offsetof(lle_cycleforest_result, depth_reached), '
            'offsetof(lle_cycleforest_result, value_words), (int)LLE_CYCLES_CAPACITY, (int)LLE_CYCLES_DENSE, (int)LLE_CYCLES_VALUE_WORDS, (int)LLE_CYCLES_MAX_ORDER); '
            'return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    R = cycleforest.CycleForestMapResult
    assert got == [C.sizeof(cycleforest.CycleForestOptions), C.sizeof(cycleforest.CycleForestArgs), C.sizeof(R), cycleforest.CycleForestOptions.stream.offset,
                   cycleforest.CycleForestArgs.t_max.offset, R.n_states.offset, R.depth_reached.offset, R.value_words.offset, cycles.LLE_CYCLES_CAPACITY,
                   cycles.LLE_CYCLES_DENSE, cycles.LLE_CYCLES_VALUE_WORDS, cycles.LLE_CYCLES_MAX_ORDER]
    assert sorted(cycleforest.compiled_kernels()) == sorted(cycleforest.KERNELS) and len(cycleforest.KERNELS) == 10
    assert cycleforest.launched_kernels() == []


def test_the_core_carries_values_of_any_width():
    """forest_core.hpp: the winner buffer holds Kind::Value at the size the library says, the root and goal words have the library's
    stride, a map's goal holds up to MAX_EXTRA words, the insert launch takes the library's dynamic LDS."""
    core = open(os.path.join(ROOT, "lle_amd", "forest", "forest_core.hpp")).read()
    assert "EXTRA_STRIDE" not in core and "uint64_t* cand" not in core
    for text in ("typename Kind::Value* cand", "size_t cand_bytes", "lanes * lib.cand_bytes", "uint32_t extra[sl::MAX_EXTRA]", "size_t insert_lds = 0", "l.insert_lds"):
        assert text in core, text
    source = open(os.path.join(ROOT, "lle_amd", "cycleforest", "cycleforest.hip")).read()
    assert "(size_t)W * fc::THREADS * 4" in source and "slabs + threadIdx.x, fc::THREADS" in source  # W * 256 * 4 bytes; a slab by the lane inside the WORKGROUP


def test_build_knows_the_library():
    from lle_amd import build
    assert '("cycleforest", "liblle_cycleforest.so")' in open(build.__file__).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "cycleforest.EXPORTS" in entry and "liblle_cycleforest.so does not export" in entry
    assert os.path.exists(cycleforest.LIB_PATH)
    ignored = subprocess.run(["git", "check-ignore", "-q", cycleforest.LIB_PATH], cwd=ROOT)
    assert ignored.returncode in (0, 128)  # ignored (128: not a git checkout)


def test_lazy_names():
    assert lle_amd.CycleForestSolver is cycleforest.CycleForestSolver and lle_amd.CycleForestResult is cycleforest.CycleForestResult
    assert lle_amd.ManyCycleCharacterization is cycleforest.ManyCycleCharacterization
    assert {"CycleForestSolver", "CycleForestResult", "ManyCycleCharacterization"} <= set(lle_amd.__all__)
    assert issubclass(cycleforest.CycleForestSolver, forest.ForestSolver) and issubclass(cycleforest.CycleForestResult, forest.ForestResult)
    assert issubclass(cycleforest.ManyCycleCharacterization, helpforest.ManyHelpCharacterization)
    assert lle_amd.solve_many is forest.solve_many and lle_amd.characterize_many is forest.characterize_many  # the plain forest keeps its names


def test_host_side_refusals():
    L = cycleforest.lib()
    line, other = Map(LINE), Map("S0 . X .")

    def refused(maps, n, opt, word):
        got = L.lle_cycleforest_create(maps, n, None if opt is None else C.byref(opt))
        message = L.lle_cycleforest_last_error()
        assert got is None and word in message, (word, message)

    two = handles([line, other])
    refused(None, 1, None, b"NULL maps")
    refused(two, 0, None, b"n_maps must be at least 1")
    refused((C.c_void_p * 2)(line.h, None), 2, None, b"NULL map (entry 1)")
    refused(two, 2, options(struct_bytes=4), b"lle_cycleforest_options.struct_bytes")
    for E, cap, word in ((-1, 0, b"envs_per_map must be"), (0, -1, b"max_states_per_map"), (1 << 30, 0, b"n_maps * envs_per_map")):
        refused(two, 2, options(E, cap), word)
    narrow, seven, three = Map("S0 . X"), Map(SEVEN), Map(THREE)
    refused(handles([line, narrow]), 2, None, b"lle_batch_create_multi: the maps of a batch must agree on height, width")
    refused(handles([seven]), 1, None, b"more than 6 agents")
    # nothing wrong with the arguments: where they are refused all the same, what is missing is the device
    for maps, n, opt in ((two, 2, None), (handles([three]), 1, options(7, 128))):
        got = L.lle_cycleforest_create(maps, n, None if opt is None else C.byref(opt))
        assert got is not None or b"no HIP device: the cycle forest" in L.lle_cycleforest_last_error(), L.lle_cycleforest_last_error()
        L.lle_cycleforest_free(got)
    # the arguments of a run are judged before the handle is looked at
    res = (cycleforest.CycleForestMapResult * 2)()

    def run_refused(word, order=3, t_max=3, struct_bytes=None):
        args = cycleforest.CycleForestArgs(C.sizeof(cycleforest.CycleForestArgs) if struct_bytes is None else struct_bytes, order, 0, t_max)
        assert L.lle_cycleforest_run(None, C.byref(args), None, res) < 0 and word in L.lle_cycleforest_last_error(), (word, L.lle_cycleforest_last_error())

    run_refused(b"struct_bytes", struct_bytes=8)
    run_refused(b"order_n must be 2 .. 6", order=1)
    run_refused(b"order_n must be 2 .. 6", order=7)
    run_refused(b"t_max must not be negative", t_max=-1)
    run_refused(b"NULL handle")
    args = cycleforest.CycleForestArgs(C.sizeof(cycleforest.CycleForestArgs), 3, 0, 3)
    assert L.lle_cycleforest_run(None, C.byref(args), None, None) == -1 and b"NULL arguments or results" in L.lle_cycleforest_last_error()
    assert L.lle_cycleforest_plan(None, 0, None, 0) == -1
    assert L.lle_cycleforest_value(None, 0, None) == -1
    assert L.lle_cycleforest_stats(None, 0, None, None, 0) == -1
    assert L.lle_cycleforest_occupancy(None, None, None) == -1
    L.lle_cycleforest_free(None)


# ---------------------------------------------------------------------------------------------------------------- CycleForestSolver
def test_solver_forms_freezing_and_refusals(monkeypatch):
    """Refusals come before any device work: nothing here makes a handle."""
    w = World("S0 . X X")
    f = cycleforest.CycleForestSolver([w, Map(LINE), "S0 X . ."], 7, envs_per_map=3, max_states_per_map=5)
    assert isinstance(f, forest.ForestSolver) and (f.t_max, f.envs_per_map, f.max_states_per_map, f.n_maps, f.n_agents, f.h) == (7, 3, 5, 3, 1, None)
    w.exit_pos = [(0, 3)]  # frozen at construction
    assert f._maps[0].positions(1) == [(0, 2), (0, 3)]
    assert cycleforest.CycleForestSolver([LINE]).t_max == 2 and cycleforest.CycleForestSolver([LINE]).envs_per_map == 256
    with pytest.raises(ValueError, match="at least one world"):
        cycleforest.CycleForestSolver([], 5)
    with pytest.raises(ValueError, match="non-negative"):
        cycleforest.CycleForestSolver([LINE], -1)
    with pytest.raises(ValueError, match="at least 1"):
        cycleforest.CycleForestSolver([LINE], 5, envs_per_map=0)
    with pytest.raises(ValueError, match=r"map 2 does not match map 0 in width \(3, map 0 has 4\)"):
        cycleforest.CycleForestSolver([LINE, LINE, "S0 . X"], 5)
    with pytest.raises(ValueError, match="at most 6 agents"):
        cycleforest.CycleForestSolver([SEVEN], 4)
    with pytest.raises(ValueError, match="at most 6 agents"):
        cycleforest.solve_many([SEVEN, SEVEN], 4, mode="no-interdependence-3")
    two_sources = "S0 . X .\nL0E . . .\nL0E . . ."
    monkeypatch.setattr(helpforest, "LLE_HELPFOREST_MAX_SOURCES", 1)
    with pytest.raises(ValueError, match=r"at most 1 laser sources.*map 0 has 2"):
        cycleforest.CycleForestSolver([two_sources, two_sources], 4)
    f = cycleforest.CycleForestSolver([THREE, THREE], 5)
    for call in (lambda: f.run("no-interdependence-3", only=[True]), lambda: f.run_closed_trail(3, only=[True, False, True]), lambda: f.run("no-mutual", only=[True])):
        with pytest.raises(ValueError, match="one entry per map"):
            call()
    for order in (1, 4, 7):  # 2 .. the maps' agents
        with pytest.raises(ValueError, match=r"order must be 2 \.\. the maps' agents \(3\)"):
            f.run_closed_trail(order)
    with pytest.raises(NotImplementedError, match="at most 16"):  # what nobody serves keeps TrailSolver's text
        f.run("no-sequence-17")
    with pytest.raises(ValueError, match="nonsense|Unknown solve mode"):
        f.run("nonsense")
    assert f.h is None and f._help is None


def test_routing_against_a_stubbed_library(monkeypatch):
    """`run` routes as CycleSolver does: 3 <= N <= agents natively, N above the agents to the inner solver's standard, N = 2 and every
    other mode to the inner HelpForestSolver; `run_closed_trail` is native for every order, 2 included; results are cached per
    (mode, collect_gems) when no mask is given."""
    calls = []

    def native(self, order, collect_gems, mask):
        calls.append(("native", order, collect_gems, None if mask is None else mask.tolist()))
        return cycleforest.CycleForestResult(length=np.array([1] * self.n_maps), status=np.zeros(self.n_maps, dtype=np.int32), n_states=np.ones(self.n_maps),
                                             depth_reached=np.ones(self.n_maps), triples=[set()] * self.n_maps, closed_orders=[[]] * self.n_maps)

    def inner(self, mode="standard", collect_gems=False, only=None):
        calls.append(("inner", str(mode), collect_gems, None if only is None else only.tolist()))
        return helpforest.HelpForestResult(length=np.array([2] * self.n_maps), status=np.zeros(self.n_maps, dtype=np.int32), n_states=np.ones(self.n_maps),
                                           depth_reached=np.ones(self.n_maps), plans=[None] * self.n_maps)

    monkeypatch.setattr(cycleforest.CycleForestSolver, "_native", native)
    monkeypatch.setattr(helpforest.HelpForestSolver, "run", inner)
    f = cycleforest.CycleForestSolver([THREE, THREE], 5, envs_per_map=64, max_states_per_map=99)
    res = f.run("no-interdependence-3")
    assert calls == [("native", 3, False, None)] and isinstance(res, cycleforest.CycleForestResult)
    assert f.run(solver.SolveMode.no_interdependence(3)) is res and len(calls) == 1  # cached
    f.run("no-interdependence-3", collect_gems=True)
    assert calls[-1] == ("native", 3, True, None)
    masked = f.run("no-interdependence-3", only=[True, False])
    assert calls[-1] == ("native", 3, False, [True, False]) and f.run("no-interdependence-3", only=[True, False]) is not masked  # a masked run is not cached
    for asked, routed in (("no-interdependence-2", "no-interdependence"), ("no-mutual", "no-interdependence"), ("no-interdependence", "no-interdependence"),
                          ("no-interdependence-4", "standard"), ("no-interdependence-6", "standard"), ("standard", "standard"), ("no-cooperation", "no-cooperation"),
                          ("no-asymmetric", "no-asymmetric"), ("no-sequence-3", "no-sequence-3"), ("no-divergence-2", "no-divergence")):
        res = f.run(asked)
        assert calls[-1] == ("inner", routed, False, None), asked
        assert isinstance(res, cycleforest.CycleForestResult) and res.length.tolist() == [2, 2] and res.triples == [None, None] and res.closed_orders == [None, None]
    assert (f._help.envs_per_map, f._help.max_states_per_map, f._help.t_max, f._help.n_maps) == (64, 99, 5, 2)  # the inner forest has the outer one's options
    f.run("no-interdependence-4", only=[False, True])
    assert calls[-1] == ("inner", "standard", False, [False, True])
    n = len(calls)
    assert f.run_closed_trail(2) is f.run_closed_trail(2) and calls[n:] == [("native", 2, False, None)]  # order 2 natively: the TEMPORAL order 2
    assert f.run_closed_trail(3) is not f.run("no-interdependence-3")  # (cached under its own key)
    assert f.h is None


# ---------------------------------------------------------------------------------------------------------------- ManyCycleCharacterization
class _Profile:
    def __init__(self, orders):
        self.orders = orders

    def is_interdependent(self, n):
        return n in self.orders


def hand_made():
    """Six worlds with known answers: 0 unsolvable, 1 independent, 2 .. 5 cooperative; the shortest plan of 2 closes no trail, that of
    3, 4 and 5 one of order 3; 3 has a plan that avoids it, 4 has none, 5 has two agents only.  `asked` records (mode, the worlds asked
    for), `profiled` the worlds whose shortest plan was replayed."""
    plan = [("a",)] * 4
    plans = {"standard": [None, plan, plan, plan, plan, plan], "no-cooperation": [None, plan[:3], None, None, None, None],
             "no-interdependence-3": [None, None, None, plan, None, None], "no-interdependence": [None, None, plan, plan, None, plan]}
    asked, profiled = [], []

    def runner(mode, only):
        asked.append((str(mode), [int(i) for i in np.flatnonzero(only)]))
        return [p if keep else None for p, keep in zip(plans[str(mode)], only)]

    def profiler(i, path):
        assert path is plan
        profiled.append(i)
        return _Profile({3} if i >= 3 else set())

    return cycleforest.ManyCycleCharacterization(9, [3, 3, 3, 3, 4, 2], runner, profiler), asked, profiled


def test_many_cycle_characterization_over_hand_made_answers():
    many, asked, profiled = hand_made()
    assert len(many) == 6 and asked == [] and profiled == []  # nothing runs before it is asked for
    assert many.is_interdependent(3).tolist() == [False, False, False, False, True, False]
    # only the maps whose answer is open are searched: cooperative, n <= n_agents, a shortest plan that closes a trail of order n
    assert asked == [("standard", [0, 1, 2, 3, 4, 5]), ("no-cooperation", [1, 2, 3, 4, 5]), ("no-interdependence-3", [3, 4])] and profiled == [2, 3, 4]
    assert many.is_interdependent(4).tolist() == [False] * 6 and [a[0] for a in asked].count("no-interdependence-4") == 0  # nobody's plan closes order 4: no run
    assert many.is_interdependent(5).tolist() == [False] * 6 and profiled == [2, 3, 4]  # more agents than any map has; every profile is made once
    assert many.is_interdependent(2).tolist() == [False, False, False, False, True, False] and asked[-1] == ("no-interdependence", [2, 3, 4, 5])
    assert many.is_mutual().tolist() == many.is_interdependent(2).tolist()
    n = len(asked)
    many.is_interdependent(3), many.is_interdependent(2), many.solvable
    assert len(asked) == n
    with pytest.raises(ValueError, match=">= 2 agents"):
        many.is_interdependent(1)
    e = many.entry(4)
    assert isinstance(e, lle_amd.WorldCharacterizer) and e.is_interdependent(3) is True and e.is_interdependent(2) is True and e.is_interdependent(4) is False
    assert many.entry(3).is_interdependent(3) is False and many.entry(3).is_cooperative() and len(asked) == n  # answered from the arrays
    assert Interdependent(3).holds(many.entry(4)) is True and Constraint(9, Cooperative() & ~Interdependent(3))._accepts(many.entry(3)) is True
    with pytest.raises(IndexError):
        many.entry(6)
    # the array of an order is kept; forget() drops answers, plans and profiles, and the next question runs again
    first = many.is_interdependent(3)
    first[:] = True
    assert many.is_interdependent(3).tolist() == [False, False, False, False, True, False] and len(asked) == n
    many.forget()
    assert many.runs == [] and many.is_interdependent(3).tolist() == [False, False, False, False, True, False]
    assert [a[0] for a in asked[n:]] == ["standard", "no-cooperation", "no-interdependence-3"] and profiled == [2, 3, 4, 2, 3, 4]
    with many as same:
        assert same is many
    # the help forest's own characterisation keeps raising
    with pytest.raises(NotImplementedError, match="no-interdependence-3"):
        helpforest.ManyHelpCharacterization(9, [3], lambda mode, only: [None]).is_interdependent(3)


# ---------------------------------------------------------------------------------------------------------------- the generator
def test_satisfied_by_many_paths(monkeypatch):
    """characterizer=CycleCharacterizer goes through cycleforest.characterize_many -- unless `options` holds a key of the single solver:
    that call keeps the loop of one characterizer per world."""
    calls = []

    def cycled(worlds, t_max, **options):
        calls.append(("cycleforest", len(worlds), t_max, options))
        return hand_made()[0]

    def single(self, world, *, characterizer=None, **solver_options):
        calls.append(("single", world, characterizer, solver_options))
        return world == "b"

    monkeypatch.setattr(cycleforest, "characterize_many", cycled)
    monkeypatch.setattr(generator.Constraint, "is_satisfied_by", single)
    six = [LINE] * 6
    got = Constraint(9, Interdependent(3)).satisfied_by_many(six, characterizer=lle_amd.CycleCharacterizer, envs_per_map=64)
    assert got.dtype == bool and got.tolist() == [False, False, False, False, True, False] and calls == [("cycleforest", 6, 9, dict(envs_per_map=64))]
    got = Constraint(9, Cooperative() & ~Interdependent(3), min_solution_length=4).satisfied_by_many(six, characterizer=lle_amd.CycleCharacterizer)
    assert got.tolist() == [False, False, True, True, False, True] and calls[-1] == ("cycleforest", 6, 9, {})
    for key in ("chunk", "max_states"):
        n = len(calls)
        got = Constraint(4, Interdependent(3)).satisfied_by_many(["a", "b"], characterizer=lle_amd.CycleCharacterizer, **{key: 8})
        assert got.tolist() == [False, True] and calls[n:] == [("single", "a", lle_amd.CycleCharacterizer, {key: 8}), ("single", "b", lle_amd.CycleCharacterizer, {key: 8})]
    # the other classes go where they went
    with pytest.raises(NotImplementedError, match="needs the solve mode 'no-interdependence-3'"):
        monkeypatch.setattr(helpforest, "characterize_many", lambda worlds, t_max, **o: helpforest.ManyHelpCharacterization(9, [3] * len(worlds), None))
        Constraint(9, Interdependent(3)).satisfied_by_many(six, characterizer=lle_amd.TrailCharacterizer)
    for doc in (Constraint.satisfied_by_many.__doc__, generator.generate_n.__doc__, Interdependent.__doc__):
        assert "CycleCharacterizer" in doc and "cycle forest" in doc and "does not answer" not in doc and "one world at a time" not in doc
    assert "chunk" in Constraint.satisfied_by_many.__doc__


# ---------------------------------------------------------------------------------------------------------------- the fixed input sets
def test_sets_have_the_stated_shapes():
    shapes = {"T": (6, 7, 3, 3, 7, 8, (2, 3)), "F": (7, 9, 4, 4, 3, 6, (3, 4)), "X": (4, 8, 6, 2, 2, 3, (2, 3)), "M": (4, 4, 2, 2, 4, 6, (2,))}
    assert set(shapes) == set(SETS)
    for name, (h, w, agents, sources, count, t_max, orders) in shapes.items():
        s = SETS[name]
        assert len(s.maps) == count == len(s.names) == len(s.changes) and s.t_max == t_max and s.orders == orders
        assert {forest.shape_key(Map(t)) for t in s.maps} == {forest.shape_key(Map(s.maps[0]))}, name
        m = Map(s.maps[0])
        assert (m.height, m.width, m.n_agents, m.n_sources, m.n_gems) == (h, w, agents, sources, 0), name
    assert SET_T.names == ("closes-in-one-state", "cycle-against-time", "paper-interdependent-3", "three-agent-temporal-cycle", "paper-fully-coupled-legacy",
                           "paper-fully-coupled", "three-agent-with-two-agent-cycle")
    assert SET_F.base == ("ring-of-four", "sequence-4-with-mutual", "ring-of-four") and SET_F.changes == (None, None, cycleforest_ref.OFF1)
    assert SET_X.names == ("six-mutual", "six-converge")
    assert SET_M.base == ("two-agent-mutual-compact",) * 3 + ("mutual-at-reset",) and SET_M.changes == (None, cycleforest_ref.OFF1, cycleforest_ref.RECOLOUR1, None)
    assert len(set(SET_M.maps[:3])) == 1 and len(set(SET_M.names)) == 4 and SET_F.maps[0] == SET_F.maps[2]  # one layout, several edge rules
    worlds = SET_M.worlds  # the worlds the device is given: the sources as the changes leave them
    assert worlds[0] == SET_M.maps[0] and all(isinstance(w, World) for w in worlds[1:3])
    assert [[(s.is_enabled, s.agent_id) for s in sorted(w.laser_sources, key=lambda s: s.laser_id)] for w in worlds[1:3]] == [[(True, 0), (False, 1)], [(True, 0), (True, 0)]]


def test_golden_file_holds_what_the_issue_states():
    assert set(GOLDEN) == set(SETS)
    for name, s in SETS.items():
        assert set(GOLDEN[name]) == {str(o) for o in s.orders} and all(len(rows) == len(s.maps) for rows in GOLDEN[name].values())
    for (name, map_name, order), want in cycleforest_ref.STATED.items():
        row = GOLDEN[name][str(order)][SETS[name].names.index(map_name)]
        assert (row["length"], row["states"]) == want, (name, map_name, order)
    assert len(cycleforest_ref.STATED) == 16
    # the orders decide different things on the same forest; some maps are solved at depth 5 while others walk all 8 levels
    two, three = GOLDEN["T"]["2"], GOLDEN["T"]["3"]
    assert [r["length"] for r in two] != [r["length"] for r in three] and {len(r["expanded"]) for r in three} >= {5, 8}
    assert GOLDEN["M"]["2"][3] == dict(length=None, frontier=[1], expanded=[], states=1)  # the reset state closes already: nothing expanded
    assert len({(r["length"], r["states"]) for r in GOLDEN["M"]["2"][:3]}) == 3  # one layout under three edge rules, three answers
    assert GOLDEN["F"]["3"][2] != GOLDEN["F"]["3"][0]  # ring-of-four with a source disabled is another world
    over = [SET_T.names[m] for m, r in enumerate(three) if r["states"] > 256]
    assert len(over) == 5 and "closes-in-one-state" not in over and "paper-interdependent-3" not in over  # capacity isolation has both kinds of map


def test_an_embedded_map_has_the_single_searchs_recorded_figures():
    """Where an embedded map is an unchanged map of kat_cycles.json at the same t_max and order, the recorded figures are equal."""
    same = 0
    for name, s in SETS.items():
        for order in s.orders:
            for m, row in enumerate(GOLDEN[name][str(order)]):
                single = cycleforest_ref.single_search(s.base[m], s.t_max, order) if s.changes[m] is None else None
                if single is not None:
                    assert row == single, (name, s.names[m], order)
                    same += 1
    assert same >= 10  # closes-in-one-state twice, ring-of-four and sequence-4-with-mutual twice each, and all of set X


ENTRIES = [(name, m, order) for name in sorted(SETS) for order in SETS[name].orders for m in range(len(SETS[name].maps))]


@pytest.mark.parametrize("name, m, order", ENTRIES, ids=[f"{n}-{SETS[n].names[m]}-{o}" for n, m, o in ENTRIES])
def test_the_restatement_still_gives_the_golden_file(name, m, order):
    """Every entry (the largest restatement, paper-fully-coupled-legacy under order 3, takes 20 s)."""
    assert cycleforest_ref.row_of(cycleforest_ref.search(SETS[name], m, order)) == GOLDEN[name][str(order)][m]


# ---------------------------------------------------------------------------------------------------------------- the kernel bodies on the host
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_insert_and_commit_under_sanitizers(tmp_path):
    """tests/hostsim/cycleforest_pieces.cpp: its own main over cycles_logic.hpp and the forest's logic headers, built with g++
    -fsanitize=address,undefined and run as a child process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "cycleforest_pieces")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "cycleforest_pieces.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    out = dict(kv.split("=") for kv in res.stdout.split()[1:])
    assert res.stdout.startswith("OK ") and int(out["lanes"]) > 5000 and int(out["records"]) > 100
    assert int(out["tag_matches"]) > 100 and int(out["pool_matches"]) > 100  # duplicates met inside a piece and across pieces
    assert int(out["dropped_closed"]) > 100  # trajectories that closed a trail of the order
