"""The closed-trail solver without a GPU: header / exports / binding of liblle_cycles.so, every refusal of its ABI that needs no device,
the solve modes it serves and how they are routed, the restatement (tests/cycles_ref.py) against the package's host-side graph on
random temporal graphs, against the reference's stated `interdependent` values (tests/golden/kat_cycles.json) and the recorded
searches, and lle_amd/cycles/cycles_logic.hpp under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/hostsim/cycles_logic.cpp).  The search itself runs on the MI355X (tests/test_gpu_cycles.py)."""
import ctypes as C
import importlib.util
import os
import random
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, characterization, cycles, generator, solver, trails
from tests import cycles_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cycles_ref.load_cases()
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"]}, **CASES["maps"])
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
KERNELS = ["cy_commit<21>", "cy_commit<3>", "cy_expand", "cy_insert<false, 21>", "cy_insert<false, 3>", "cy_insert<true, 21>", "cy_insert<true, 3>"]
LAYOUTS = ["one-way-detour", "sequence-4-with-mutual", "sequence-3-without-cycle", "paper-sequence-2-not-interdependent-3", "paper-fully-coupled",
           "paper-fully-coupled-legacy", "two-agent-mutual-with-detours", "temporal-flattening-counterexample", "three-agent-temporal-cycle",
           "three-agent-with-two-agent-cycle", "paper-interdependent-3", "four-agent-interdependent-4-sequence-6"]


def search_id(s):
    return f"{s['map']}{cycles_ref.changes_label(s.get('changes'))}-t{s['t_max']}-n{s['n']}" + ("-gems" if s["collect_gems"] else "")


def agents_of(text):
    return len(set(re.findall(r"S(\d)", text)))


def test_kat_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location("make_kat_cycles", os.path.join(ROOT, "tests", "golden", "make_kat_cycles.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CATALOGUE == CASES["catalogue"] and mod.MAPS == CASES["maps"] and mod.SEARCHES == CASES["searches"]
    assert [c["name"] for c in CASES["catalogue"]] == LAYOUTS
    for c in CASES["catalogue"]:
        assert c["ref"].startswith("python/tests/world_layouts.py:") and c["expect"] and c["map"].strip()
        for e in c["expect"].values():
            assert set(e) == {"interdependent"} and e["interdependent"] and all(int(n) >= 3 and isinstance(v, bool) for n, v in e["interdependent"].items())
    horizons = {c["name"]: sorted(int(t) for t in c["expect"]) for c in CASES["catalogue"]}
    assert horizons["one-way-detour"] == list(range(6, 12)) and horizons["temporal-flattening-counterexample"] == [20]
    assert CASES["catalogue"][-1]["expect"]["14"]["interdependent"] == {"3": True, "4": True, "5": False}
    import json
    hg = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_helpgraph.json")))
    theirs = dict({c["name"]: c["map"] for c in hg["catalogue"]}, **hg["maps"])
    for name in ("two-agent-mutual-compact", "gem-detour", "six-mutual", "six-converge", "paper-fully-coupled", "two-agent-mutual-with-detours"):
        assert MAPS[name] == theirs[name]  # the maps both fixtures hold are the same text
    ids = [search_id(s) for s in CASES["searches"]]
    assert len(set(ids)) == len(ids) == 13 + 16 + 2
    for s in CASES["searches"]:
        assert s["map"] in MAPS and 2 <= s["n"] <= agents_of(MAPS[s["map"]]) and sum(s["frontier"]) == s["states"] <= 21345
        assert len(s["expanded"]) == len(s["frontier"]) - 1 and (s["length"] is None or s["length"] == len(s["expanded"]))
        assert set(s) - {"changes"} == {"map", "t_max", "n", "collect_gems", "length", "states", "frontier", "expanded"}
    # every stated value of an order within the map's agents has its search, at the stated t_max
    have = {(s["map"], s["t_max"], s["n"]) for s in CASES["searches"] if "changes" not in s and not s["collect_gems"]}
    for c in CASES["catalogue"]:
        for t, e in c["expect"].items():
            for n in e["interdependent"]:
                assert int(n) > agents_of(c["map"]) or (c["name"], int(t), int(n)) in have, (c["name"], t, n)


def test_library_exports():
    """liblle_cycles.so exports every function include/lle_cycles.h declares, and the binding knows exactly those; the header is plain C
    and the one the library is compiled against; struct sizes and constants of the binding are the header's."""
    L = cycles.lib()
    header = open(os.path.join(ROOT, "include", "lle_cycles.h")).read()
    declared = set(re.findall(r"\b(lle_cycles_[a-z_0-9]+)\s*\(", header))
    assert declared == set(cycles.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "cycles", "cycles.hip")).read()
    assert '#include "../../include/lle_cycles.h"' in source and '#include "cycles_logic.hpp"' in source and '#include "../search/search_core.hpp"' in source
    assert '#include "../search/search_logic.hpp"' in source and '#include "../search/search_device.hpp"' in source
    logic = open(os.path.join(ROOT, "lle_amd", "cycles", "cycles_logic.hpp")).read()
    assert '#include "../helpgraph/helpgraph_logic.hpp"' in logic and "state_edges" in logic  # the edge rule is the help-graph search's
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    assert not re.search(r"lle_(helpgraph|search|trails)_(create|run|plan|stats|free)\b", source)  # no symbol of another search library
    assert not re.search(r"\b(__)?asm(__)?\b", source + logic)  # plain C++ only
    # the pruning rule stands in the same words in the header, the logic and the restatement
    rule = ["a triple with |S| > N is never stored, because supports only grow;", "a trajectory is dropped the moment some (a, a, S) with |S| = N appears;",
            "kept are (a, c, S) with a != c and |S| <= N, and (a, a, S) with |S| < N."]
    for text in (header, logic, open(os.path.join(ROOT, "tests", "cycles_ref.py")).read()):
        assert all(line in text for line in rule)
    names = ["LLE_CYCLES_CAPACITY", "LLE_CYCLES_DENSE", "LLE_CYCLES_MAX_AGENTS", "LLE_CYCLES_MAX_SOURCES", "LLE_CYCLES_MIN_ORDER", "LLE_CYCLES_MAX_ORDER",
             "LLE_CYCLES_WALK_BUDGET", "LLE_CYCLES_VALUE_WORDS"]
    prog = ('#include <stdio.h>\n#include "lle_cycles.h"\nint main(void) { printf("%zu %zu %zu' + " %d" * len(names) + '", sizeof(lle_cycles_options), '
            'sizeof(lle_cycles_args), sizeof(lle_cycles_result), ' + ", ".join(names) + '); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(cycles.CycleOptions), C.sizeof(cycles.CycleArgs), C.sizeof(cycles.CycleResult)] + [getattr(cycles, n) for n in names]
    assert cycles.LLE_CYCLES_CAPACITY == solver.LLE_SEARCH_CAPACITY != cycles.LLE_CYCLES_DENSE and cycles.LLE_CYCLES_WALK_BUDGET == trails.LLE_TRAILS_WALK_BUDGET
    assert sorted(cycles.compiled_kernels()) == KERNELS
    from lle_amd import build
    text = open(build.__file__).read()
    assert '("cycles", "liblle_cycles.so")' in text and text.index('("trails", "liblle_trails.so")') < text.index('("cycles", "liblle_cycles.so")')
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "cycles.EXPORTS" in entry and "liblle_cycles.so does not export" in entry


def test_lazy_names():
    assert lle_amd.CycleSolver is cycles.CycleSolver and lle_amd.CycleCharacterizer is cycles.CycleCharacterizer
    assert issubclass(cycles.CycleSolver, solver.Solver) and issubclass(cycles.CycleCharacterizer, trails.TrailCharacterizer)
    assert {"CycleSolver", "CycleCharacterizer"} <= set(lle_amd.__all__)


def test_host_side_refusals():
    """NULL and bad-argument refusals of every ABI call that can be made without a device.  lle_cycles_run judges its arguments before it
    looks at the handle, so N = 1 and N = 7 are refused here as they are on a machine with a device."""
    L, line, seven = cycles.lib(), Map(LINE), Map(SEVEN)
    assert L.lle_cycles_create(None, None) is None and b"NULL" in L.lle_cycles_last_error()
    bad = cycles.CycleOptions(4, -1, 0, 0, None)
    assert L.lle_cycles_create(line.h, C.byref(bad)) is None and b"struct_bytes" in L.lle_cycles_last_error()
    for chunk, max_states, word in ((-1, 0, b"chunk"), ((1 << 30) + 1, 0, b"chunk"), (0, -1, b"max_states"), (0, (1 << 30) + 1, b"max_states")):
        opt = cycles.CycleOptions(C.sizeof(cycles.CycleOptions), -1, chunk, max_states, None)
        assert L.lle_cycles_create(line.h, C.byref(opt)) is None and word in L.lle_cycles_last_error()
    assert L.lle_cycles_create(seven.h, None) is None and b"more than 6 agents" in L.lle_cycles_last_error()
    size = C.sizeof(cycles.CycleArgs)
    good, res = cycles.CycleArgs(size, 2, 0, 5), cycles.CycleResult(C.sizeof(cycles.CycleResult))
    assert L.lle_cycles_run(None, None, None) == -1 and L.lle_cycles_run(None, C.byref(good), None) == -1
    assert L.lle_cycles_run(None, C.byref(good), C.byref(res)) == -1 and b"NULL handle" in L.lle_cycles_last_error()
    assert L.lle_cycles_run(None, C.byref(cycles.CycleArgs(size, 6, 1, 0)), C.byref(res)) == -1  # N = 6 passes the argument checks
    for n in (1, 7, 0, -3):
        assert L.lle_cycles_run(None, C.byref(cycles.CycleArgs(size, n, 0, 5)), C.byref(res)) == -2 and b"order_n must be 2 .. 6" in L.lle_cycles_last_error()
    assert L.lle_cycles_run(None, C.byref(cycles.CycleArgs(size - 4, 2, 0, 5)), C.byref(res)) == -2 and b"lle_cycles_args.struct_bytes" in L.lle_cycles_last_error()
    assert L.lle_cycles_run(None, C.byref(good), C.byref(cycles.CycleResult(8))) == -2 and b"lle_cycles_result.struct_bytes" in L.lle_cycles_last_error()
    assert L.lle_cycles_run(None, C.byref(cycles.CycleArgs(size, 2, 0, -1)), C.byref(res)) == -2 and b"t_max" in L.lle_cycles_last_error()
    assert L.lle_cycles_plan(None, None, 0) == -1
    assert L.lle_cycles_stats(None, None, None, 0) == -1
    L.lle_cycles_free(None)


def test_triples_decode():
    """cycles.triples against the layout as include/lle_cycles.h words it, both classes."""
    assert cycles.triples([0, 0, 0], 3) == set() and cycles.triples([0] * 21, 6) == set()
    # class 4: closed field a = 8 bits at 8 a; open field (a, c) = 4 bits at 32 + 4 (3 a + c - (c > a))
    assert cycles.triples([1 << 8, 0, 0], 4) == {(1, 1, frozenset({1}))}
    assert cycles.triples([1 << (8 + 1), 0, 0], 2) == {(1, 1, frozenset({0, 1}))}
    assert cycles.triples([0, 1 << 0, 0], 4) == {(0, 1, frozenset({0, 1}))} and cycles.triples([0, 1 << 3, 0], 4) == {(0, 1, frozenset({0, 1, 2, 3}))}
    assert cycles.triples([0, 0, 1 << (4 * (3 * 3 + 2 - 8) + 1)], 4) == {(3, 2, frozenset({0, 2, 3}))}
    # class 6: closed field a = word a; open field (a, c) = 16 bits at 192 + 16 (5 a + c - (c > a))
    words = [0] * 21
    words[5] = 1 << 0b01000  # p = 01000 with a one inserted at bit 5: agents {3, 5}
    at = 192 + 16 * (5 * 5 + 3)  # (5, 3)
    words[at // 32] |= 1 << (at % 32 + 0b0001)  # p = 0001, ones inserted at bits 3 and 5: agents {0, 3, 5}
    assert cycles.triples(words, 6) == {(5, 5, frozenset({3, 5})), (5, 3, frozenset({0, 3, 5}))} == cycles.triples(words, 5)
    with pytest.raises(ValueError):
        cycles.triples([0, 0, 0], 6)


# ------------------------------------------------------------------------------------------------ the mode table
REFERENCE_MODES = ["standard", "no-cooperation", "no-asymmetric", "no-mutual", "no-fully-coupled", "no-sequence", "no-sequence-2", "no-sequence-3",
                   "no-sequence-16", "no-sequence-17", "no-interdependence", "no-interdependence-2", "no-interdependence-3", "no-interdependence-4",
                   "no-interdependence-6", "no-interdependence-9", "no-convergence", "no-convergence-2", "no-convergence-3", "no-divergence", "no-divergence-2",
                   "no-divergence-3"]
UNBUILT = {"no-sequence-17"}


@pytest.mark.parametrize("text", REFERENCE_MODES)
def test_every_mode_of_the_reference_is_served_or_named(text):
    s = cycles.CycleSolver(LINE, 1)  # (the lower bound, 3, exceeds t_max: a served mode answers None without a search, without a device)
    mode = solver.SolveMode.from_str(text)
    assert cycles.serves(text) == cycles.serves(mode) == (text not in UNBUILT)
    if text in UNBUILT:
        for call, name in ((lambda: s.find_shortest(text), text), (lambda: s.find_shortest(mode), str(mode)), (lambda: s.solve(mode=text), text)):
            with pytest.raises(NotImplementedError, match=re.escape(f"'{name}'")) as err:
                call()
            assert "at most 16" in str(err.value)  # TrailSolver's text: the limit is named
    else:
        assert s.find_shortest(text) is None and s.find_shortest(mode) is None and s.solve(0, mode=text) is None
    assert s.h is None and s._inner is None


def test_routing(monkeypatch):
    """no-interdependence-N: 3 <= N <= n_agents is native, N > n_agents is the inner solver's `standard`, N = 2 and every other mode go to
    the inner TrailSolver over the frozen map, made on first use and kept."""
    calls, native = [], []

    def fake(self, mode, collect_gems):
        calls.append((self, str(mode), collect_gems))
        self.last_stats = dict(length=3, marker=len(calls))
        return [[4, 4, 4]] * 3

    def fake_native(self, order, collect_gems):
        native.append((order, collect_gems))
        self.last_stats = dict(length=3, native=True)
        return [[4, 4, 4]] * 3

    monkeypatch.setattr(trails.TrailSolver, "_shortest", fake)
    monkeypatch.setattr(cycles.CycleSolver, "_native", fake_native)
    s = cycles.CycleSolver("S0 S1 S2 . X X X", 5, chunk=7, max_states=11)
    assert s._inner is None and s.world.n_agents == 3
    assert s.find_shortest("no-interdependence-3") is not None and native == [(3, False)] and calls == [] and s._inner is None and s.last_stats["native"]
    s.find_shortest("no-interdependence-4", collect_gems=True)
    inner = s._inner
    assert native == [(3, False)] and [c[1:] for c in calls] == [("standard", True)] and type(inner) is trails.TrailSolver and calls[0][0] is inner
    assert (inner.t_max, inner.chunk, inner.max_states) == (5, 7, 11) and inner._map is not s.world._map and s.last_stats == dict(length=3, marker=1)
    for text in ("no-mutual", "no-interdependence-2", "no-sequence-3", "standard", "no-convergence-3", "no-interdependence-6"):
        s.find_shortest(text)
    assert s._inner is inner and native == [(3, False)]
    assert [c[1] for c in calls[1:]] == ["no-interdependence", "no-interdependence", "no-sequence-3", "standard", "no-convergence-3", "standard"]
    assert s.shortest_without_closed_trail(2, collect_gems=True) is not None and native[-1] == (2, True)  # order 2 natively, on request only
    for bad in (1, 4, 7):
        with pytest.raises(ValueError, match="order must be 2"):
            s.shortest_without_closed_trail(bad)
    assert s.h is None


def test_the_solver_interface_without_a_search():
    w = World(LINE)
    s = cycles.CycleSolver(w, 7, chunk=3, max_states=5)
    assert s.world is w and s.t_max == 7 and (s.chunk, s.max_states) == (3, 5) and s.last_stats is None and s.solution_lower_bound == 3
    with pytest.raises(ValueError, match="exceeds this solver's t_max"):
        s.find_shortest("no-interdependence-3", t_min=8)
    with pytest.raises(ValueError, match="non-negative"):
        s.solve(-1, mode="no-interdependence-3")
    assert s.solve(2, mode="no-interdependence-3") is None  # below the lower bound: no search, no device
    with pytest.raises(ValueError, match="at most 6 agents"):
        cycles.CycleSolver(SEVEN, 4)
    with pytest.raises(ValueError):
        s.find_shortest("no-interdependence-1")
    assert s.h is None


def test_the_characterizer_without_a_search():
    w = World("S0 L1S X\n. . .\n. . X\nS1 . L0N")
    c = cycles.CycleCharacterizer(w, 6)
    assert c.world is w and c.t_max == 6 and c.n_laser_colours == 2 and type(c._solver) is cycles.CycleSolver
    assert c == cycles.CycleCharacterizer(w, 6) and hash(c) == hash(cycles.CycleCharacterizer(w, 6)) and c != cycles.CycleCharacterizer(w, 7)
    assert c != trails.TrailCharacterizer(w, 6)
    for call in (lambda: c.is_interdependent(1), lambda: c.is_interdependent(0), lambda: c.compute_shortest_non_interdependent_path(1), lambda: c.is_sequential(1)):
        with pytest.raises(ValueError):
            call()
    assert c._solver.h is None
    # every order is cached on its own, under the mode's name
    seen = []
    c._solver.find_shortest = lambda mode, **kw: seen.append(str(mode)) or None
    assert c.compute_shortest_non_interdependent_path(3) is None and c.compute_shortest_non_interdependent_path(4) is None
    assert c.compute_shortest_non_interdependent_path(3) is None and seen == ["no-interdependence-3", "no-interdependence-4"]
    assert generator.Constraint.is_satisfied_by.__kwdefaults__["characterizer"] is characterization.WorldCharacterizer  # the generator is unchanged
    for doc in (generator.Interdependent.__doc__, generator.Constraint.is_satisfied_by.__doc__):
        assert "CycleCharacterizer" in doc
    with pytest.raises(NotImplementedError, match="no-interdependence-3"):
        trails.TrailCharacterizer(w, 6).is_interdependent(3)  # as before


# ------------------------------------------------------------------------------------------------ the restatement
def random_graph(rng, agents, layers, arcs_per_layer):
    out = []
    for _t in range(layers):
        arcs = set()
        for _ in range(rng.randint(0, arcs_per_layer)):
            h, b = rng.randrange(agents), rng.randrange(agents)
            if h != b:
                arcs.add((h, b))
        out.append(sorted(arcs))
    return out


def test_the_update_unpruned_is_the_graphs_predicate():
    """On seeded random temporal graphs of 3 to 6 agents: some (a, a, S) with |S| = k is in R exactly when
    TemporalCooperationGraph.has_closed_trail_of_order(k), for every k; and the pruned update keeps exactly the unpruned triples of at
    most n agents up to the layer at which order n closes."""
    from lle_amd.characterization import DependencyEdge, TemporalCooperationGraph
    rng, cases = random.Random(20261020), 0
    for _g in range(900):
        agents = rng.randint(3, 6)
        layers = random_graph(rng, agents, rng.randint(1, 4), 6)
        R, edges = frozenset(), []
        pruned = {n: frozenset() for n in range(2, agents + 1)}
        for t, arcs in enumerate(layers):
            R = cycles_ref.layer_update(R, arcs)
            edges += [DependencyEdge(h, b, t) for h, b in arcs]
            for n in pruned:
                if pruned[n] is not None:
                    pruned[n] = cycles_ref.layer_update(pruned[n], arcs, n)
                    assert pruned[n] == {x for x in R if len(x[2]) <= n}
                    if cycles_ref.closes(pruned[n], n):
                        pruned[n] = None  # the search drops the trajectory here
        graph = TemporalCooperationGraph(edges)
        for k in range(2, agents + 2):
            assert graph.has_closed_trail_of_order(k) == cycles_ref.closes(R, k), (layers, k)
            cases += 1
    assert cases > 3000


def test_layer_update_from_the_definition():
    up, f = cycles_ref.layer_update, frozenset
    assert up(f(), []) == f() and up(f(), {(0, 1)}) == {(0, 1, f({0, 1}))}
    assert up(f(), {(0, 1), (1, 2)}) == {(0, 1, f({0, 1})), (1, 2, f({1, 2})), (0, 2, f({0, 1, 2}))}          # two arcs of one state chain
    assert up(up(f(), {(1, 2)}), {(0, 1)}) == {(1, 2, f({1, 2})), (0, 1, f({0, 1}))}                              # decreasing times do not
    assert (0, 0, f({0, 1})) in up(f(), {(0, 1), (1, 0)}) and (1, 1, f({0, 1})) in up(f(), {(0, 1), (1, 0)})
    revisit = up(up(f(), {(0, 1), (1, 0)}), {(0, 2), (2, 0)})
    assert cycles_ref.closes(revisit, 3) and (0, 0, f({0, 1, 2})) in revisit and not any(a == c != 0 and len(s) == 3 for a, c, s in revisit)
    ring = f()
    for arc in ((0, 1), (1, 2), (2, 3), (3, 0)):
        ring = up(ring, {arc})
    assert cycles_ref.closes(ring, 4) and not cycles_ref.closes(ring, 3) and not cycles_ref.closes(ring, 2)       # orders are not monotone
    assert up(f(), {(0, 1), (1, 2)}, 2) == {(0, 1, f({0, 1})), (1, 2, f({1, 2}))}                                  # |S| > N is never stored


def _stated():
    for c in CASES["catalogue"]:
        for t, e in c["expect"].items():
            for n, want in e["interdependent"].items():
                yield pytest.param(c["map"], int(t), int(n), want, id=f"{c['name']}-t{t}-{n}")


@pytest.mark.parametrize("text,t_max,n,want", list(_stated()))
def test_the_restatement_reproduces_the_reference(text, t_max, n, want):
    """Every stated value of the golden file through the reference's predicate definition over tests/cycles_ref.py (an order above the
    map's agents: no closed trail is possible, solvable is the whole question): the link between the reference and what the GPU tests
    compare the library with."""
    if n > agents_of(text):
        from tests import helpgraph_ref
        assert want is False and helpgraph_ref.search(text, t_max).length is not None
        return
    assert cycles_ref.is_interdependent(text, t_max, n) is want


@pytest.mark.parametrize("s", CASES["searches"], ids=[search_id(s) for s in CASES["searches"]])
def test_the_restatement_reproduces_the_recorded_searches(s):
    changes = s.get("changes")
    res = cycles_ref.search(MAPS[s["map"]], s["t_max"], s["n"], s["collect_gems"], changes=changes)
    assert (res.length, res.n_states, res.frontier, res.expanded) == (s["length"], s["states"], s["frontier"], s["expanded"])
    if res.plan is not None:
        assert cycles_ref.check_plan(MAPS[s["map"]], res.plan, s["n"], s["collect_gems"], length=s["length"], changes=changes, triples=res.triples,
                                     closed_orders=res.closed_orders) == res.triples


def test_the_small_maps_show_what_they_are_named_for():
    """The shapes tests/test_gpu_cycles.py needs, as the restatement sees them."""
    f = frozenset
    # closes-in-one-state: the reset state holds 0 -> 1 -> 2 chained; under N = 2 a plan exists and its replay closes order 3 through them
    R0, edges0, _w = cycles_ref.replay_triples(MAPS["closes-in-one-state"], [])
    assert sorted(edges0) == [(0, 1, 0), (1, 2, 0)] and (0, 2, f({0, 1, 2})) in R0
    plan = cycles_ref.search(MAPS["closes-in-one-state"], 8, 2).plan
    R, edges, _w = cycles_ref.replay_triples(MAPS["closes-in-one-state"], plan)
    assert cycles_ref.closes(R, 3) and {(h, b) for h, b, _t in edges} == {(0, 1), (1, 2), (2, 0)}
    assert not any((h, b) == (0, 1) and t > 0 for h, b, t in edges), "0 -> 1 happens at the reset only: the closure needs the two arcs of that one state"
    assert cycles_ref.search(MAPS["closes-in-one-state"], 8, 3).length is None
    # cycle-against-time: the flattened 3-cycle, times decreasing
    res = cycles_ref.search(MAPS["cycle-against-time"], 7, 3)
    _R, edges, _w = cycles_ref.replay_triples(MAPS["cycle-against-time"], res.plan)
    first = {arc: min(t for h, b, t in edges if (h, b) == arc) for arc in ((2, 0), (1, 2), (0, 1))}
    assert res.length == 5 and res.closed_orders == [] and first[(2, 0)] < first[(1, 2)] < first[(0, 1)]
    # revisited-anchor: no flattened cycle over three agents, and still no plan under N = 3
    from tests import helpgraph_ref
    std = helpgraph_ref.search(MAPS["revisited-anchor"], 8)
    assert std.length == 6 and std.edges == {(0, 1), (1, 0), (0, 2), (2, 0)} and cycles_ref.search(MAPS["revisited-anchor"], 8, 3).length is None
    # ring-of-four, mutual-at-reset, twins and merges
    assert cycles_ref.search(MAPS["mutual-at-reset"], 4, 2).frontier == [1]
    for name, t, n in (("cycle-against-time", 7, 3), ("closes-in-one-state", 8, 2), ("two-agent-mutual-compact", 6, 2)):
        res = cycles_ref.search(MAPS[name], t, n)
        assert res.merges > 0 and (res.twins > 0 or name == "closes-in-one-state")
    assert cycles_ref.search(MAPS["cycle-against-time"], 7, 3).twins > 0


def test_check_plan_refuses_a_plan_with_the_closed_trail():
    text = MAPS["closes-in-one-state"]
    plan = cycles_ref.search(text, 8, 2).plan
    cycles_ref.check_plan(text, plan, 2)
    with pytest.raises(AssertionError):
        cycles_ref.check_plan(text, plan, 3)
    with pytest.raises(AssertionError):
        cycles_ref.check_plan(text, plan[:-1], 2)


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_logic_under_sanitizers(tmp_path):
    """tests/hostsim/cycles_logic.cpp: its own main over cycles_logic.hpp, built with g++ -fsanitize=address,undefined and run as a child
    process; nothing sanitized is loaded into this interpreter.  The cases go to it as a text file: seeded random temporal graphs with the
    triples the restatement finds under a random order, layer by layer as the search prunes."""
    exe, cases = str(tmp_path / "cycles_logic"), str(tmp_path / "cases.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "cycles_logic.cpp"), "-o", exe] + SAN, check=True)
    rng, count = random.Random(7), 2500
    with open(cases, "w") as out:
        for _g in range(count):
            agents = rng.randint(2, 6)
            n, layers = rng.randint(2, agents), random_graph(rng, agents, rng.randint(1, 4), 5)
            R, closed = frozenset(), 0
            for arcs in layers:
                if not closed:
                    R = cycles_ref.layer_update(R, arcs, n)
                    closed = int(cycles_ref.closes(R, n))
            row = [agents, n, len(layers)]
            for arcs in layers:
                row += [len(arcs)] + [v for arc in arcs for v in arc]
            row.append(closed)
            if not closed:
                row.append(len(R))
                for a, c, s in sorted(R, key=lambda x: (x[0], x[1], sorted(x[2]))):
                    row += [a, c, sum(1 << k for k in s)]
            out.write(" ".join(map(str, row)) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    got = dict(kv.split("=") for kv in res.stdout.split()[1:])
    assert res.stdout.startswith("OK ") and int(got["cases"]) == count and int(got["small_and_large"]) > 1000
    assert int(got["closed"]) > 1000 and int(got["triples"]) > 8000 and int(got["dense"]) == 2
