"""The trail solver without a GPU: header / exports / binding of liblle_trails.so, every refusal of its ABI that needs no device, the
solve modes it serves, the restatement (tests/trails_ref.py) against the reference's stated `sequential` values
(tests/golden/kat_trails.json) and the recorded searches, and lle_amd/trails/trails_logic.hpp under AddressSanitizer +
UndefinedBehaviorSanitizer in a stand-alone program (tests/hostsim/trails_logic.cpp).  The search itself runs on the MI355X
(tests/test_gpu_trails.py)."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, characterization, generator, helpgraph, solver, trails
from tests import trails_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = trails_ref.load_cases()
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"] if "map" in c}, **CASES["maps"])
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
KERNELS = ["tr_commit", "tr_expand", "tr_insert<false>", "tr_insert<true>"]
LAYOUTS = ["level-6", "one-way-detour", "single-laser-asymmetric", "sequence-4-with-mutual", "sequence-3-without-cycle", "paper-sequence-2",
           "paper-sequence-2-not-interdependent-3", "paper-convergent-2", "two-agent-mutual-with-detours", "temporal-flattening-counterexample",
           "three-agent-temporal-cycle", "three-agent-with-two-agent-cycle", "paper-interdependent-3", "four-agent-interdependent-4-sequence-6"]
# Left out of the comparison with the restatement, which reaches a state by replaying its whole prefix: each of these walks 70 000 to
# 320 000 work items for one stated value, 10 to 45 seconds a value.  The restatement was run on every one of them when the fixture
# was made and gave the stated value each time; tests/test_gpu_trails.py holds them to their stated values on the device.
# level-6 has no map text in the fixture and overflows the pool at its t_max (tests/golden/make_kat_trails.py).
BEYOND_THE_RESTATEMENT = ("level-6", "paper-sequence-2-not-interdependent-3", "temporal-flattening-counterexample", "three-agent-with-two-agent-cycle",
                          "four-agent-interdependent-4-sequence-6")


def search_id(s):
    return f"{s['map']}{trails_ref.changes_label(s.get('changes'))}-t{s['t_max']}-n{s['n']}" + ("-gems" if s["collect_gems"] else "")


def recorded(map_name, n, collect_gems=False, changes=None, t_max=None):
    """The first recorded search of the map under `changes` (None: the unchanged world) with this N (and this t_max)."""
    return next(s for s in CASES["searches"] if (s["map"], s["n"], s["collect_gems"], s.get("changes")) == (map_name, n, collect_gems, changes)
                and t_max in (None, s["t_max"]))


def test_kat_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location("make_kat_trails", os.path.join(ROOT, "tests", "golden", "make_kat_trails.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CATALOGUE == CASES["catalogue"] and mod.MAPS == CASES["maps"] and mod.SEARCHES == CASES["searches"]
    assert [c["name"] for c in CASES["catalogue"]] == LAYOUTS and set(BEYOND_THE_RESTATEMENT) <= set(LAYOUTS)
    for c in CASES["catalogue"]:
        assert c["ref"].startswith("python/tests/world_layouts.py:") and c["expect"] and ("map" in c) != ("level" in c)
        for e in c["expect"].values():
            assert set(e) == {"sequential"} and e["sequential"] and all(int(n) >= 2 and isinstance(v, bool) for n, v in e["sequential"].items())
    horizons = {c["name"]: sorted(int(t) for t in c["expect"]) for c in CASES["catalogue"]}
    assert horizons["one-way-detour"] == list(range(6, 12)) and horizons["two-agent-mutual-with-detours"] == [6]
    assert horizons["temporal-flattening-counterexample"] == [20] and horizons["level-6"] == [21]
    assert CASES["catalogue"][-1]["expect"]["14"]["sequential"] == {"2": True, "3": True, "4": True, "5": True, "6": True, "7": False}
    hg = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_helpgraph.json")))
    theirs = dict({c["name"]: c["map"] for c in hg["catalogue"]}, **hg["maps"])
    for name in ("two-agent-mutual-compact", "gem-detour", "three-beam-cell", "six-mutual", "six-converge", "single-laser-asymmetric",
                 "paper-convergent-2", "two-agent-mutual-with-detours"):
        assert MAPS[name] == theirs[name]  # the maps both fixtures hold are the same text
    ids = [search_id(s) for s in CASES["searches"]]
    assert len(set(ids)) == len(ids) == 23 + 15 + 9
    for s in CASES["searches"]:
        assert s["map"] in MAPS and 2 <= s["n"] <= 16 and sum(s["frontier"]) == s["states"] <= 4540
        assert len(s["expanded"]) == len(s["frontier"]) - 1 and (s["length"] is None or s["length"] == len(s["expanded"]))
        assert set(s) - {"changes"} == {"map", "t_max", "n", "collect_gems", "length", "states", "frontier", "expanded"}
    assert [s for s in CASES["searches"] if "changes" not in s][:23] == CASES["searches"][:23], "the entries before long-trails stand where they stood"
    assert [(s["t_max"], s["n"]) for s in CASES["searches"] if s["map"] == "long-trails" and "changes" not in s] == [(24, n) for n in range(2, 17)]
    changed = [(s["map"], trails_ref.changes_label(s["changes"]), s["t_max"], s["n"]) for s in CASES["searches"] if "changes" in s]
    compact = "two-agent-mutual-compact"
    assert changed == [(compact, "-source1-off", 8, 2), (compact, "-source1-off", 8, 3), (compact, "-source0-off", 8, 2), (compact, "-source0-off", 8, 3),
                       (compact, "-source1-colour0", 8, 2), (compact, "-source1-colour0", 8, 3), ("long-trails", "-source1-off", 24, 16),
                       (compact, "-source0-off-source1-off", 8, 2), (compact, "-source0-off-source1-off", 8, 16)]


def test_library_exports():
    """liblle_trails.so exports every function include/lle_trails.h declares, and the binding knows exactly those; the header is plain C
    and the one the library is compiled against; struct sizes and constants of the binding are the header's."""
    L = trails.lib()
    header = open(os.path.join(ROOT, "include", "lle_trails.h")).read()
    declared = set(re.findall(r"\b(lle_trails_[a-z_0-9]+)\s*\(", header))
    assert declared == set(trails.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "trails", "trails.hip")).read()
    assert '#include "../../include/lle_trails.h"' in source and '#include "trails_logic.hpp"' in source
    assert '#include "../search/search_logic.hpp"' in source and '#include "../search/search_device.hpp"' in source
    logic = open(os.path.join(ROOT, "lle_amd", "trails", "trails_logic.hpp")).read()
    assert '#include "../helpgraph/helpgraph_logic.hpp"' in logic and "state_edges" in source  # the edge rule is the help-graph search's
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    assert not re.search(r"lle_(helpgraph|search)_(create|run|plan|stats|free)\b", source)  # no symbol of another search library
    assert not re.search(r"\b(__)?asm(__)?\b", source + logic)  # plain C++ only
    names = ["LLE_TRAILS_CAPACITY", "LLE_TRAILS_DENSE", "LLE_TRAILS_MAX_AGENTS", "LLE_TRAILS_MAX_SOURCES", "LLE_TRAILS_MIN_LENGTH", "LLE_TRAILS_MAX_LENGTH",
             "LLE_TRAILS_WALK_BUDGET"]
    prog = ('#include <stdio.h>\n#include "lle_trails.h"\nint main(void) { printf("%zu %zu %zu' + " %d" * len(names) + '", sizeof(lle_trails_options), '
            'sizeof(lle_trails_args), sizeof(lle_trails_result), ' + ", ".join(names) + '); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(trails.TrailOptions), C.sizeof(trails.TrailArgs), C.sizeof(trails.TrailResult)] + [getattr(trails, n) for n in names]
    assert trails.LLE_TRAILS_CAPACITY == solver.LLE_SEARCH_CAPACITY != trails.LLE_TRAILS_DENSE
    assert sorted(trails.compiled_kernels()) == KERNELS
    from lle_amd import build
    assert '("trails", "liblle_trails.so")' in open(build.__file__).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "trails.EXPORTS" in entry and "liblle_trails.so does not export" in entry


def test_lazy_names():
    assert lle_amd.TrailSolver is trails.TrailSolver and lle_amd.TrailCharacterizer is trails.TrailCharacterizer
    assert issubclass(trails.TrailSolver, solver.Solver) and issubclass(trails.TrailCharacterizer, helpgraph.HelpGraphCharacterizer)
    assert {"TrailSolver", "TrailCharacterizer"} <= set(lle_amd.__all__)


def test_host_side_refusals():
    """NULL and bad-argument refusals of every ABI call that can be made without a device.  lle_trails_run judges its arguments before it
    looks at the handle, so N = 1 and N = 17 are refused here as they are on a machine with a device."""
    L, line, seven = trails.lib(), Map(LINE), Map(SEVEN)
    assert L.lle_trails_create(None, None) is None and b"NULL" in L.lle_trails_last_error()
    bad = trails.TrailOptions(4, -1, 0, 0, None)
    assert L.lle_trails_create(line.h, C.byref(bad)) is None and b"struct_bytes" in L.lle_trails_last_error()
    for chunk, max_states, word in ((-1, 0, b"chunk"), ((1 << 30) + 1, 0, b"chunk"), (0, -1, b"max_states"), (0, 1 << 31, b"max_states"), (0, (1 << 30) + 1, b"max_states")):
        opt = trails.TrailOptions(C.sizeof(trails.TrailOptions), -1, chunk, max_states, None)
        assert L.lle_trails_create(line.h, C.byref(opt)) is None and word in L.lle_trails_last_error()
    assert L.lle_trails_create(seven.h, None) is None and b"more than 6 agents" in L.lle_trails_last_error()
    size = C.sizeof(trails.TrailArgs)
    good, res = trails.TrailArgs(size, 2, 0, 5), trails.TrailResult(C.sizeof(trails.TrailResult))
    assert L.lle_trails_run(None, None, None) == -1 and L.lle_trails_run(None, C.byref(good), None) == -1
    assert L.lle_trails_run(None, C.byref(good), C.byref(res)) == -1 and b"NULL handle" in L.lle_trails_last_error()
    assert L.lle_trails_run(None, C.byref(trails.TrailArgs(size, 16, 1, 0)), C.byref(res)) == -1  # N = 16 passes the argument checks
    for n in (1, 17, 0, -3):
        assert L.lle_trails_run(None, C.byref(trails.TrailArgs(size, n, 0, 5)), C.byref(res)) == -2 and b"length_n must be 2 .. 16" in L.lle_trails_last_error()
    assert L.lle_trails_run(None, C.byref(trails.TrailArgs(size - 4, 2, 0, 5)), C.byref(res)) == -2 and b"lle_trails_args.struct_bytes" in L.lle_trails_last_error()
    assert L.lle_trails_run(None, C.byref(good), C.byref(trails.TrailResult(8))) == -2 and b"lle_trails_result.struct_bytes" in L.lle_trails_last_error()
    assert L.lle_trails_run(None, C.byref(trails.TrailArgs(size, 2, 0, -1)), C.byref(res)) == -2 and b"t_max" in L.lle_trails_last_error()
    assert L.lle_trails_plan(None, None, 0) == -1
    assert L.lle_trails_stats(None, None, None, 0) == -1
    L.lle_trails_free(None)


def test_trail_lengths():
    assert trails.trail_lengths(0, 3) == [0, 0, 0]
    assert trails.trail_lengths(0x00F0A021, 6) == [1, 2, 0, 10, 0, 15] and trails.trail_lengths(0x00F0A021, 2) == [1, 2]


# ------------------------------------------------------------------------------------------------ the mode table
REFERENCE_MODES = ["standard", "no-cooperation", "no-asymmetric", "no-mutual", "no-fully-coupled", "no-sequence", "no-sequence-2", "no-sequence-3",
                   "no-sequence-16", "no-sequence-17", "no-interdependence", "no-interdependence-2", "no-interdependence-3", "no-interdependence-4",
                   "no-convergence", "no-convergence-2", "no-convergence-3", "no-divergence", "no-divergence-2", "no-divergence-3"]
UNBUILT = {"no-sequence-17", "no-interdependence-3", "no-interdependence-4"}


@pytest.mark.parametrize("text", REFERENCE_MODES)
def test_every_mode_of_the_reference_is_served_or_named(text):
    s = trails.TrailSolver(LINE, 1)  # (the lower bound, 3, exceeds t_max: a served mode answers None without a search, without a device)
    mode = solver.SolveMode.from_str(text)
    assert trails.serves(text) == trails.serves(mode) == (text not in UNBUILT)
    if text in UNBUILT:
        for call, name in ((lambda: s.find_shortest(text), text), (lambda: s.find_shortest(mode), str(mode)), (lambda: s.solve(mode=text), text)):
            with pytest.raises(NotImplementedError, match=re.escape(f"'{name}'")) as err:  # the mode as the caller wrote it
                call()
            if text == "no-sequence-17":
                assert "at most 16" in str(err.value)  # the limit is named
            else:
                assert "'no-sequence[-N]'" in str(err.value) and "'no-mutual'" in str(err.value) and "'no-convergence[-k]'" in str(err.value)  # what is served
    else:
        assert s.find_shortest(text) is None and s.find_shortest(mode) is None and s.solve(0, mode=text) is None
    assert s.h is None and s._inner is None


def test_modes_of_the_help_graph_are_delegated(monkeypatch):
    """Everything but no-sequence goes to an inner HelpGraphSolver over the frozen map, made on first use and kept; no-sequence does not."""
    calls = []

    def fake(self, mode, collect_gems):
        calls.append((self, str(mode), collect_gems))
        self.last_stats = dict(length=3, marker=len(calls))
        return [[4], [4], [4]]

    monkeypatch.setattr(helpgraph.HelpGraphSolver, "_shortest", fake)
    s = trails.TrailSolver(LINE, 5, chunk=7, max_states=11)
    assert s._inner is None
    plan = s.find_shortest("no-mutual")
    assert plan is not None and len(plan) == 3 and len(calls) == 1 and calls[0][1:] == ("no-interdependence", False)
    inner = s._inner
    assert type(inner) is helpgraph.HelpGraphSolver and calls[0][0] is inner and (inner.t_max, inner.chunk, inner.max_states) == (5, 7, 11)
    assert inner._map is not s.world._map and s.last_stats == dict(length=3, marker=1)
    for text in ("standard", "no-cooperation", "no-convergence-3"):
        s.find_shortest(text, collect_gems=True)
    assert s._inner is inner and [c[1:] for c in calls[1:]] == [("standard", True), ("no-cooperation", True), ("no-convergence-3", True)]
    assert s.h is None  # no handle of liblle_trails.so was needed


def test_the_solver_interface_without_a_search():
    w = World(LINE)
    s = trails.TrailSolver(w, 7, chunk=3, max_states=5)
    assert s.world is w and s.t_max == 7 and (s.chunk, s.max_states) == (3, 5) and s.last_stats is None and s.solution_lower_bound == 3
    assert trails.TrailSolver(LINE).t_max == 2
    with pytest.raises(ValueError, match="exceeds this solver's t_max"):
        s.find_shortest("no-sequence", t_min=8)
    with pytest.raises(ValueError, match="exceeds this solver's t_max=7"):
        s.solve(8, mode="no-sequence-3")
    with pytest.raises(ValueError, match="non-negative"):
        s.solve(-1, mode="no-sequence-3")
    assert s.solve(2, mode="no-sequence-16") is None  # below the lower bound: no search, no device
    for bad in (dict(t_max=-1), dict(chunk=0), dict(max_states=0)):
        with pytest.raises(ValueError):
            trails.TrailSolver(LINE, **dict(dict(t_max=5), **bad))
    with pytest.raises(ValueError, match="at most 6 agents"):
        trails.TrailSolver(SEVEN, 4)
    with pytest.raises(ValueError):
        s.find_shortest("no-sequence-1")
    with pytest.raises(ValueError):
        s.find_shortest("nonsense")
    w2 = World("S0 . X X")  # frozen at construction, like Solver
    s2 = trails.TrailSolver(w2, 5)
    w2.exit_pos = [(0, 3)]
    assert s2.solution_lower_bound == 2 and trails.TrailSolver(w2, 5).solution_lower_bound == 3


def test_the_characterizer_without_a_search():
    w = World("S0 L1S X\n. . .\n. . X\nS1 . L0N")
    c = trails.TrailCharacterizer(w, 6)
    assert c.world is w and c.t_max == 6 and c.n_laser_colours == 2 and type(c._solver) is trails.TrailSolver
    assert c == trails.TrailCharacterizer(w, 6) and hash(c) == hash(trails.TrailCharacterizer(w, 6)) and c != trails.TrailCharacterizer(w, 7)
    assert c != helpgraph.HelpGraphCharacterizer(w, 6)
    with pytest.raises(NotImplementedError, match="no-interdependence-3"):
        c.is_interdependent(3)
    for call in (lambda: c.is_sequential(1), lambda: c.is_sequential(0), lambda: c.compute_shortest_path_without_sequence(1), lambda: c.is_interdependent(1),
                 lambda: c.is_convergent(1)):
        with pytest.raises(ValueError):
            call()
    assert c._solver.h is None
    assert generator.Constraint.is_satisfied_by.__kwdefaults__["characterizer"] is characterization.WorldCharacterizer  # the generator is unchanged


# ------------------------------------------------------------------------------------------------ the restatement
def _stated():
    for c in CASES["catalogue"]:
        if c["name"] in BEYOND_THE_RESTATEMENT:
            continue
        for t, e in c["expect"].items():
            for n, want in e["sequential"].items():
                yield pytest.param(c["map"], int(t), int(n), want, id=f"{c['name']}-t{t}-{n}")


@pytest.mark.parametrize("text,t_max,n,want", list(_stated()))
def test_the_restatement_reproduces_the_reference(text, t_max, n, want):
    """Every stated value of the golden file within the restatement's reach, through the reference's predicate definition over
    tests/trails_ref.py: the link between the reference and what the GPU tests compare the library with."""
    assert trails_ref.is_sequential(text, t_max, n) is want
    res = trails_ref.search(text, t_max, n)
    if res.plan is not None:
        assert max(trails_ref.check_plan(text, res.plan, n, length=res.length)) < n


@pytest.mark.parametrize("s", CASES["searches"], ids=[search_id(s) for s in CASES["searches"]])
def test_the_restatement_reproduces_the_recorded_searches(s):
    changes = s.get("changes")
    res = trails_ref.search(MAPS[s["map"]], s["t_max"], s["n"], s["collect_gems"], changes=changes)
    assert (res.length, res.n_states, res.frontier, res.expanded) == (s["length"], s["states"], s["frontier"], s["expanded"])
    if res.plan is not None:
        assert trails_ref.check_plan(MAPS[s["map"]], res.plan, s["n"], s["collect_gems"], length=s["length"], changes=changes) == res.trails


def test_layer_update_from_the_definition():
    up = trails_ref.layer_update
    assert up((0, 0, 0), []) == (0, 0, 0) and up((3, 1, 2), set()) == (3, 1, 2)
    assert up((0, 0, 0), {(0, 1), (1, 2)}) == (0, 1, 2)            # two arcs of one state chain
    assert up(up((0, 0, 0), {(1, 2)}), {(0, 1)}) == (0, 1, 1)      # decreasing times do not
    assert up(up((0, 0, 0), {(0, 1)}), {(1, 2)}) == (0, 1, 2)
    assert up((0, 0), {(0, 1), (1, 0)}) == (2, 2) and up((2, 2), {(0, 1), (1, 0)}) == (4, 4)  # a mutual pair held: two more per state
    assert up((0, 0, 0), {(0, 2), (2, 0), (0, 1), (2, 1)}) == (2, 3, 2)  # three-beam-cell's state: 2 -> 0 -> 2 -> 1
    assert up((0, 5, 0), {(1, 2)}) == (0, 5, 6) and up((0, 5, 0), {(0, 2)}) == (0, 5, 1)


# ------------------------------------------------------------------------------------------------ the maps, by what they are for
def test_the_small_maps_show_what_they_are_named_for():
    """The shapes tests/test_gpu_trails.py needs, each on a map of a few cells, as the restatement sees them."""
    # two arcs in one state chain
    chain = trails_ref.search(MAPS["chain-in-one-state"], 8, 3)
    assert trails_ref.search(MAPS["chain-in-one-state"], 8, 2).length is None and (chain.length, chain.trails) == (5, (0, 1, 2))
    _L, edges, _w = trails_ref.replay_trails(MAPS["chain-in-one-state"], chain.plan)
    assert any((0, 1, t) in edges and (1, 2, t) in edges for t in range(chain.length + 1))  # in ONE state
    # a reset state with an edge, and one the mode rejects: one record, no level
    at_reset = trails_ref.replay_trails(MAPS["chain-at-reset"], [])
    assert at_reset[0] == (0, 1, 2) and sorted(at_reset[1]) == [(0, 1, 0), (1, 2, 0)]
    rejected = trails_ref.search(MAPS["chain-at-reset"], 6, 2)
    assert (rejected.length, rejected.frontier, rejected.expanded) == (None, [1], []) and trails_ref.search(MAPS["chain-at-reset"], 6, 3).trails == (0, 1, 2)
    # decreasing times do not chain: the flattened relation holds 0 -> 1 -> 2, the longest trail has one edge
    late = trails_ref.search(MAPS["decreasing-times"], 8, 2)
    _L, edges, _w = trails_ref.replay_trails(MAPS["decreasing-times"], late.plan)
    assert late.length == 6 and late.trails == (0, 1, 1) and {(h, b) for h, b, _t in edges} == {(0, 1), (1, 2)}
    assert max(t for h, b, t in edges if (h, b) == (1, 2)) < min(t for h, b, t in edges if (h, b) == (0, 1))
    from tests import helpgraph_ref
    assert helpgraph_ref.search(MAPS["decreasing-times"], 8).length == 6
    # a mutual pair held over a STAY: the help-graph search sees one relation, the trails grow by two a step
    compact = [recorded("two-agent-mutual-compact", n) for n in (2, 3, 4, 5, 16)]
    assert [s["length"] for s in compact] == [None, 5, 5, 5, 5] and [s["states"] for s in compact] == [100, 119, 125, 126, 126]
    assert trails_ref.search(MAPS["two-agent-mutual-compact"], 6, 16).peak == 4  # N = 4 is the largest the horizon can reach, N = 5 rejects nothing
    assert helpgraph_ref.search(MAPS["two-agent-mutual-compact"], 6).n_states == 123  # (world state, flattened relation) records: another count
    # a mutual pair and a cycle inside one layer: a trail of three edges from one state
    beam = [recorded("three-beam-cell", n) for n in (2, 3, 4, 7, 8, 16)]
    assert [s["length"] for s in beam] == [None, None, 4, 4, 4, 4] and trails_ref.search(MAPS["three-beam-cell"], 5, 16).peak == 7
    assert trails_ref.search(MAPS["three-beam-cell"], 5, 4).trails == (2, 3, 2)
    # two candidates of one level with one world state: stored twice under different L, once under equal L from different parents
    for name, n in (("two-agent-mutual-compact", 3), ("decreasing-times", 2), ("six-mutual", 3)):
        res = trails_ref.search(MAPS[name], recorded(name, n)["t_max"], n)
        assert res.twins > 0 and res.merges > 0
    # six agents: agent 5's field
    assert trails_ref.search(MAPS["six-mutual"], 3, 3).trails == (0, 0, 0, 1, 0, 2) and trails_ref.search(MAPS["six-converge"], 3, 3).trails == (0, 0, 0, 2, 2, 1)
    # gems
    assert recorded("gem-detour", 3, True)["length"] == 7 > recorded("gem-detour", 3)["length"] == 5 and recorded("gem-detour", 2, True)["length"] is None


# ------------------------------------------------------------------------------------------------ long trails, changed worlds
LONG_T_MAX = 24


def test_long_trails_store_every_field_up_to_15():
    """What tests/test_gpu_trails_edges.py leans on, from the restatement itself: for every N in 2 .. 16 long-trails has no plan, stores
    100 + 76 (N - 2) records whose greatest field is N - 1, and its frontier runs empty at depth N + 5 < t_max -- so every N has its own
    counters, and a device that clips a field, mis-shifts its stack or compares N off by one gives those of another N or of none."""
    text = MAPS["long-trails"]
    results = {n: trails_ref.search(text, LONG_T_MAX, n) for n in range(2, 17)}
    for n, res in results.items():
        s = recorded("long-trails", n)
        assert (s["t_max"], s["length"], s["states"], s["frontier"], s["expanded"]) == (LONG_T_MAX, None, res.n_states, res.frontier, res.expanded)
        assert res.length is None and res.plan is None and res.trails is None
        assert res.n_states == 100 + 76 * (n - 2) and res.peak == n - 1
        assert len(res.expanded) == n + 5 < LONG_T_MAX and len(res.frontier) == n + 6 and res.frontier[-1] == 0 and all(res.frontier[:-1])
    assert (results[15].n_states, results[16].n_states) == (1088, 1164)
    assert len({(tuple(r.frontier), tuple(r.expanded)) for r in results.values()}) == 15  # every N has counters of its own
    last = results[16]
    assert last.frontier == [1, 3, 6, 13, 35, 68, 74] + [76] * 10 + [75, 70, 48, 11, 0]
    assert last.expanded == [6, 29, 61, 172, 426, 786, 847] + [865] * 10 + [853, 784, 483, 102]
    assert max(f * 25 for f in last.frontier) == 1900 and -(-1900 // 64) == 30  # work items of the largest level: 30 pieces of 64
    assert max(last.expanded) == 865  # of which 865 are joint actions the masks allow
    # the walls change nothing before the pair is formed: up to depth 4 the levels are two-agent-mutual-compact's
    assert last.frontier[:5] == recorded("two-agent-mutual-compact", 16)["frontier"][:5]
    assert trails_ref.is_sequential(text, LONG_T_MAX, 2) is False and trails_ref.is_sequential(text, LONG_T_MAX, 16) is False  # not solvable at all


@pytest.mark.parametrize("size, name, n", [((20, 20), "long-trails", 16), ((255, 6), "long-trails", 16), ((6, 255), "long-trails", 3), ((64, 64), "long-trails", 3),
                                           ((65, 66), "chain-in-one-state", 3), ((6, 255), "chain-in-one-state", 2)], ids=str)
def test_an_embedded_layout_has_the_small_layouts_counters(size, name, n):
    """`helpgraph_ref.embed` puts the layout in the far corner of a map of walls: the same world to the restatement, so the GPU tests may
    hold the device to the small layout's recorded counters on the big map."""
    from tests import helpgraph_ref
    s = recorded(name, n)
    res = trails_ref.search(helpgraph_ref.embed(MAPS[name], *size), s["t_max"], n)
    assert (res.length, res.n_states, res.frontier, res.expanded) == (s["length"], s["states"], s["frontier"], s["expanded"])


def test_one_layout_four_worlds_four_answers():
    """two-agent-mutual-compact at t_max 8 under no-sequence-2: unchanged, source 1 disabled, source 0 disabled, source 1 recoloured to
    0 -- four different (length, records), so a search that reads another world's rule gives another world's answer."""
    from tests import helpgraph_ref
    text, compact = MAPS["two-agent-mutual-compact"], "two-agent-mutual-compact"
    maker = importlib.util.spec_from_file_location("make_kat_trails", os.path.join(ROOT, "tests", "golden", "make_kat_trails.py"))
    mod = importlib.util.module_from_spec(maker)
    maker.loader.exec_module(mod)
    variants = [None, mod.OFF1, mod.OFF0, mod.RECOLOUR1]
    got = []
    for changes in variants:
        res = trails_ref.search(text, 8, 2, changes=changes)
        got.append((res.length, res.n_states))
        if changes is not None:
            s = recorded(compact, 2, changes=changes)
            assert (s["t_max"], s["length"], s["states"]) == (8, res.length, res.n_states)
    assert got == [(None, 100), (5, 164), (5, 130), (None, 107)] and len(set(got)) == 4
    # None is the unchanged world, computed once: the entry without `changes` is the same object as before
    assert trails_ref.search(text, 8, 2, changes=None) is trails_ref.search(text, 8, 2)
    assert trails_ref.search(text, 6, 2).n_states == recorded(compact, 2, t_max=6)["states"] == 100
    # the predicate under changes: unchanged every plan holds a mutual pair; without source 1 a plan avoids every trail of two edges
    assert trails_ref.is_sequential(text, 8, 2) is True and trails_ref.is_sequential(text, 8, 2, changes=mod.OFF1) is False
    assert trails_ref.is_sequential(text, 8, 2, changes=mod.RECOLOUR1) is False  # (not solvable at all in that world)
    # every source disabled: no arc anywhere, so every N walks the plain search of the changed world
    plain = helpgraph_ref.search(text, 8, changes=mod.ALL_OFF)
    for n in (2, 16):
        res, s = trails_ref.search(text, 8, n, changes=mod.ALL_OFF), recorded(compact, n, changes=mod.ALL_OFF)
        assert (res.length, res.frontier, res.expanded, res.peak) == (plain.length, plain.frontier, plain.expanded, 0) == (5, s["frontier"], s["expanded"], 0)
        assert res.trails == (0, 0) and plain.edges == set() and s["states"] == 151
    # a plan found in one world is refused in another: the replay is under the entry's changes
    plan = trails_ref.search(text, 8, 2, changes=mod.OFF1).plan
    assert trails_ref.check_plan(text, plan, 2, length=5, changes=mod.OFF1) == (0, 1)
    with pytest.raises(Exception):
        trails_ref.check_plan(text, plan, 2, changes=None)
    long_off = trails_ref.search(MAPS["long-trails"], LONG_T_MAX, 16, changes=mod.OFF1)
    assert (long_off.length, long_off.n_states, long_off.peak) == (None, 198, 1) and long_off.n_states == recorded("long-trails", 16, changes=mod.OFF1)["states"]


def test_check_plan_refuses_a_plan_with_a_longer_trail():
    text = MAPS["two-agent-mutual-compact"]
    plan = trails_ref.search(text, 6, 3).plan
    assert trails_ref.check_plan(text, plan, 3) == (2, 1)
    with pytest.raises(AssertionError):
        trails_ref.check_plan(text, plan, 2)
    with pytest.raises(AssertionError):
        trails_ref.check_plan(text, plan[:-1], 3)


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_logic_under_sanitizers(tmp_path):
    """tests/hostsim/trails_logic.cpp: its own main over trails_logic.hpp, built with g++ -fsanitize=address,undefined and run as a child
    process; nothing sanitized is loaded into this interpreter.  The longest_trail cases of tests/golden/kat_coop.json go to it as a
    text file."""
    exe, kat = str(tmp_path / "trails_logic"), str(tmp_path / "longest_trail.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "trails_logic.cpp"), "-o", exe] + SAN, check=True)
    graphs = [g for g in json.load(open(os.path.join(ROOT, "tests", "golden", "kat_coop.json")))["graphs"] if "longest_trail" in g["expect"]]
    fits = [g for g in graphs if all(0 <= h < 6 and 0 <= b < 6 and t >= 0 for h, b, t in g["edges"])]
    assert len(fits) >= 15 and {"trail_decreasing_times", "trail_may_not_revisit_same_edge", "trail_same_time"} <= {g["name"] for g in fits}
    with open(kat, "w") as f:
        for g in fits:
            f.write(" ".join(str(v) for v in [g["expect"]["longest_trail"], len(g["edges"])] + [x for e in g["edges"] for x in e]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed), kat], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["graphs"]) + int(out["dense_graphs"]) == 6000 and int(out["dense_graphs"]) < 60
        assert int(out["fields"]) > 20000 and int(out["reached"]) > 5000 and int(out["same_time_cycles"]) > 1000 and int(out["kat"]) == len(fits)
        assert int(out["dense"]) + int(out["answered"]) == 16 and int(out["dense"]) >= 1 and int(out["answered"]) >= 10
        assert (int(out["stored"]), int(out["duplicates"])) == (4, 8)
