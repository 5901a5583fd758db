"""The help-graph solver without a GPU: header / exports / binding of liblle_helpgraph.so, every refusal of its ABI, the solve modes
it serves, the restatement (tests/helpgraph_ref.py) against the reference's stated values (tests/golden/kat_helpgraph.json) and the
recorded searches, and lle_amd/helpgraph/helpgraph_logic.hpp under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/hostsim/helpgraph_logic.cpp).  The search itself runs on the MI355X (tests/test_gpu_helpgraph.py)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, characterization, generator, helpgraph, solver
from tests import helpgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = helpgraph_ref.load_cases()
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"]}, **CASES["maps"])
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
KERNELS = ["hg_commit", "hg_expand", "hg_insert<false>", "hg_insert<true>"]
LAYOUTS = ["single-laser-asymmetric", "double-disjoint-asymmetric", "convergent-2-tight", "divergent-2-tight", "divergent-2-with-detour",
           "paper-convergent-2", "paper-fully-coupled", "paper-fully-coupled-legacy", "fully-coupled-4agents", "two-agent-mutual-compact",
           "two-agent-mutual-with-detours"]


def search_id(s):
    return f"{s['map']}-t{s['t_max']}-{s['mode']}-{s['param']}" + ("-gems" if s["collect_gems"] else "") + helpgraph_ref.changes_label(s.get("changes"))


def test_kat_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location("make_kat_helpgraph", os.path.join(ROOT, "tests", "golden", "make_kat_helpgraph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CATALOGUE == CASES["catalogue"] and mod.MAPS == CASES["maps"] and mod.SEARCHES == CASES["searches"]
    assert [c["name"] for c in CASES["catalogue"]] == LAYOUTS
    fields = {"asymmetric", "fully_coupled", "convergent", "divergent", "interdependent"}
    for c in CASES["catalogue"]:
        assert c["ref"].startswith("python/tests/world_layouts.py:") and c["expect"]
        for e in c["expect"].values():
            assert e and set(e) <= fields and set(e.get("interdependent", {"2": 0})) == {"2"}
    horizons = {c["name"]: sorted(int(t) for t in c["expect"]) for c in CASES["catalogue"]}
    assert horizons["divergent-2-tight"] == [2, 8] and horizons["divergent-2-with-detour"] == [2, 5, 6, 8]
    assert horizons["two-agent-mutual-with-detours"] == list(range(5, 15))
    assert not {s["map"] for s in CASES["searches"]} & set(BEYOND_THE_RESTATEMENT)
    for s in CASES["searches"]:
        assert s["map"] in MAPS and s["mode"] in helpgraph_ref.MODES and sum(s["frontier"]) == s["states"] <= 7599
        assert len(s["expanded"]) == len(s["frontier"]) - 1 and (s["length"] is None or s["length"] == len(s["expanded"]))
    # what the restatement walks: no search added later expands more items than the largest of the first 37
    ids = [search_id(s) for s in CASES["searches"]]
    assert len(set(ids)) == len(ids) == 68
    largest = max(CASES["searches"][:37], key=lambda s: sum(s["expanded"]))
    assert search_id(largest) == "paper-fully-coupled-legacy-t10-no-fully-coupled-2" and sum(largest["expanded"]) == 247075
    assert all(sum(s["expanded"]) <= 247075 for s in CASES["searches"])
    assert all("changes" not in s for s in CASES["searches"][:37])


def test_library_exports():
    """liblle_helpgraph.so exports every function include/lle_helpgraph.h declares, and the binding knows exactly those; the header is
    plain C and the one the library is compiled against; struct sizes and constants of the binding are the header's."""
    L = helpgraph.lib()
    header = open(os.path.join(ROOT, "include", "lle_helpgraph.h")).read()
    declared = set(re.findall(r"\b(lle_helpgraph_[a-z_0-9]+)\s*\(", header))
    assert declared == set(helpgraph.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "helpgraph", "helpgraph.hip")).read()
    assert '#include "../../include/lle_helpgraph.h"' in source and '#include "helpgraph_logic.hpp"' in source
    assert '#include "../search/search_logic.hpp"' in source and '#include "../search/search_device.hpp"' in source
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    names = ["LLE_HELPGRAPH_CAPACITY", "LLE_HELPGRAPH_STANDARD", "LLE_HELPGRAPH_NO_ASYMMETRIC", "LLE_HELPGRAPH_NO_MUTUAL", "LLE_HELPGRAPH_NO_FULLY_COUPLED",
             "LLE_HELPGRAPH_NO_CONVERGENCE", "LLE_HELPGRAPH_NO_DIVERGENCE", "LLE_HELPGRAPH_MAX_AGENTS", "LLE_HELPGRAPH_MAX_SOURCES"]
    prog = ('#include <stdio.h>\n#include "lle_helpgraph.h"\nint main(void) { printf("%zu %zu %zu' + " %d" * len(names) + '", sizeof(lle_helpgraph_options), '
            'sizeof(lle_helpgraph_args), sizeof(lle_helpgraph_result), ' + ", ".join(names) + '); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(helpgraph.HelpGraphOptions), C.sizeof(helpgraph.HelpGraphArgs), C.sizeof(helpgraph.HelpGraphResult)] + [getattr(helpgraph, n) for n in names]
    assert helpgraph.LLE_HELPGRAPH_CAPACITY == solver.LLE_SEARCH_CAPACITY
    assert sorted(helpgraph.compiled_kernels()) == KERNELS


def test_lazy_names():
    assert lle_amd.HelpGraphSolver is helpgraph.HelpGraphSolver and lle_amd.HelpGraphCharacterizer is helpgraph.HelpGraphCharacterizer
    assert issubclass(helpgraph.HelpGraphSolver, solver.Solver) and issubclass(helpgraph.HelpGraphCharacterizer, characterization.WorldCharacterizer)
    assert {"HelpGraphSolver", "HelpGraphCharacterizer"} <= set(lle_amd.__all__)


def test_host_side_refusals():
    """NULL and bad-argument refusals of every ABI call that can be made without a device."""
    L, line, seven = helpgraph.lib(), Map(LINE), Map(SEVEN)
    assert L.lle_helpgraph_create(None, None) is None and b"NULL" in L.lle_helpgraph_last_error()
    bad = helpgraph.HelpGraphOptions(4, -1, 0, 0, None)
    assert L.lle_helpgraph_create(line.h, C.byref(bad)) is None and b"struct_bytes" in L.lle_helpgraph_last_error()
    for chunk, max_states, word in ((-1, 0, b"chunk"), ((1 << 30) + 1, 0, b"chunk"), (0, -1, b"max_states"), (0, 1 << 31, b"max_states"), (0, (1 << 30) + 1, b"max_states")):
        opt = helpgraph.HelpGraphOptions(C.sizeof(helpgraph.HelpGraphOptions), -1, chunk, max_states, None)
        assert L.lle_helpgraph_create(line.h, C.byref(opt)) is None and word in L.lle_helpgraph_last_error()
    assert L.lle_helpgraph_create(seven.h, None) is None and b"more than 6 agents" in L.lle_helpgraph_last_error()
    args, res = helpgraph.HelpGraphArgs(C.sizeof(helpgraph.HelpGraphArgs), 0, 2, 0, 5), helpgraph.HelpGraphResult(C.sizeof(helpgraph.HelpGraphResult))
    assert L.lle_helpgraph_run(None, None, None) == -1 and L.lle_helpgraph_run(None, C.byref(args), C.byref(res)) == -1
    assert L.lle_helpgraph_plan(None, None, 0) == -1
    assert L.lle_helpgraph_stats(None, None, None, 0) == -1
    L.lle_helpgraph_free(None)


def test_help_edges():
    assert helpgraph.help_edges(0, 0) == set()
    assert helpgraph.help_edges(1 << 1 | 1 << 8 | 1 << (8 * 3 + 5), 1 << (8 * 5 + 4 - 32)) == {(0, 1), (1, 0), (3, 5), (5, 4)}


# ------------------------------------------------------------------------------------------------ the mode table
REFERENCE_MODES = ["standard", "no-cooperation", "no-asymmetric", "no-mutual", "no-fully-coupled", "no-sequence", "no-sequence-2", "no-sequence-3",
                   "no-interdependence", "no-interdependence-2", "no-interdependence-3", "no-interdependence-4", "no-convergence", "no-convergence-2",
                   "no-convergence-3", "no-divergence", "no-divergence-2", "no-divergence-3"]
UNBUILT = {"no-sequence", "no-sequence-2", "no-sequence-3", "no-interdependence-3", "no-interdependence-4"}


@pytest.mark.parametrize("text", REFERENCE_MODES)
def test_every_mode_of_the_reference_is_served_or_named(text):
    s = helpgraph.HelpGraphSolver(LINE, 1)  # (the lower bound, 3, exceeds t_max: a served mode answers None without a search, without a device)
    mode = solver.SolveMode.from_str(text)
    assert helpgraph.serves(text) == helpgraph.serves(mode) == (text not in UNBUILT)
    if text in UNBUILT:
        for call, name in ((lambda: s.find_shortest(text), text), (lambda: s.find_shortest(mode), str(mode)), (lambda: s.solve(mode=text), text)):
            with pytest.raises(NotImplementedError, match=re.escape(f"'{name}'")) as err:  # the mode as the caller wrote it
                call()
            assert "'no-mutual'" in str(err.value) and "'no-convergence[-k]'" in str(err.value)  # the message lists what is served
    else:
        assert s.find_shortest(text) is None and s.find_shortest(mode) is None and s.solve(0, mode=text) is None
    assert s.h is None


def test_mutual_is_interdependence_2():
    M = solver.SolveMode
    assert M.from_str("no-mutual") == M.from_str("no-interdependence") == M.from_str("no-interdependence-2") == M.no_mutual()
    assert helpgraph._served_mode("no-mutual").kind == "no-interdependence" and helpgraph._NATIVE["no-interdependence"] == helpgraph.LLE_HELPGRAPH_NO_MUTUAL
    with pytest.raises(ValueError):
        helpgraph.HelpGraphSolver(LINE, 5).find_shortest("nonsense")
    with pytest.raises(ValueError):
        helpgraph.HelpGraphSolver(LINE, 5).find_shortest("no-convergence-1")


def test_the_solver_interface_without_a_search():
    w = World(LINE)
    s = helpgraph.HelpGraphSolver(w, 7, chunk=3, max_states=5)
    assert s.world is w and s.t_max == 7 and (s.chunk, s.max_states) == (3, 5) and s.last_stats is None and s.solution_lower_bound == 3
    assert helpgraph.HelpGraphSolver(LINE).t_max == 2
    with pytest.raises(ValueError, match="exceeds this solver's t_max"):
        s.find_shortest("no-mutual", t_min=8)
    with pytest.raises(ValueError, match="exceeds this solver's t_max=7"):
        s.solve(8, mode="no-asymmetric")
    with pytest.raises(ValueError, match="non-negative"):
        s.solve(-1, mode="no-asymmetric")
    assert s.solve(2, mode="no-divergence-3") is None  # below the lower bound: no search, no device
    for bad in (dict(t_max=-1), dict(chunk=0), dict(max_states=0)):
        with pytest.raises(ValueError):
            helpgraph.HelpGraphSolver(LINE, **dict(dict(t_max=5), **bad))
    with pytest.raises(ValueError, match="at most 6 agents"):
        helpgraph.HelpGraphSolver(SEVEN, 4)
    w2 = World("S0 . X X")  # frozen at construction, like Solver
    s2 = helpgraph.HelpGraphSolver(w2, 5)
    w2.exit_pos = [(0, 3)]
    assert s2.solution_lower_bound == 2 and helpgraph.HelpGraphSolver(w2, 5).solution_lower_bound == 3


def test_the_characterizer_without_a_search():
    w = World("S0 L1S X\n. . .\n. . X\nS1 . L0N")
    c = helpgraph.HelpGraphCharacterizer(w, 6)
    assert c.world is w and c.t_max == 6 and c.n_laser_colours == 2
    assert c == helpgraph.HelpGraphCharacterizer(w, 6) and hash(c) == hash(helpgraph.HelpGraphCharacterizer(w, 6)) and c != helpgraph.HelpGraphCharacterizer(w, 7)
    for call, mode in ((c.is_sequential, "no-sequence-2"), (lambda: c.is_sequential(3), "no-sequence-3"), (lambda: c.is_interdependent(3), "no-interdependence-3")):
        with pytest.raises(NotImplementedError, match=mode):
            call()
    for call in (lambda: c.is_sequential(1), lambda: c.is_convergent(1), lambda: c.is_divergent(0), lambda: c.is_interdependent(1),
                 lambda: c.compute_shortest_path_without_convergence(1), lambda: c.compute_shortest_path_without_divergence(1),
                 lambda: c.compute_shortest_non_interdependent_path(1)):
        with pytest.raises(ValueError):
            call()
    assert c.is_divergent(2) is False and c.is_divergent(5) is False  # k >= n_agents: no search
    assert "characterizer" in generator.Constraint.is_satisfied_by.__kwdefaults__
    assert generator.Constraint.is_satisfied_by.__kwdefaults__["characterizer"] is characterization.WorldCharacterizer


# ------------------------------------------------------------------------------------------------ the restatement
# fully-coupled-4agents stores 84 128 records within its t_max of 8 (625 joint actions each): hours of replay for the restatement, and
# more than the 7 599 records every listed search stays within.  It has no search in the golden file and no test here or on the GPU
# compares it with the restatement (tests/golden/make_kat_helpgraph.py says what the searches through World.step find on it).
BEYOND_THE_RESTATEMENT = ("fully-coupled-4agents",)


def _stated():
    for c in CASES["catalogue"]:
        if c["name"] in BEYOND_THE_RESTATEMENT:
            continue
        for t, e in c["expect"].items():
            for key, want in e.items():
                for k, v in (want.items() if isinstance(want, dict) else [(None, want)]):
                    yield pytest.param(c["map"], int(t), key, k, v, id=f"{c['name']}-t{t}-{key}" + (f"-{k}" if k else ""))


@pytest.mark.parametrize("text,t_max,key,k,want", list(_stated()))
def test_the_restatement_reproduces_the_reference(text, t_max, key, k, want):
    """Every stated value of the golden file, through the reference's predicate definitions over tests/helpgraph_ref.py: the link between
    the reference and what the GPU tests compare the library with."""
    answers = helpgraph_ref.characterize(text, t_max)
    assert (answers[key]() if k is None else answers[key](int(k))) is want


@pytest.mark.parametrize("s", CASES["searches"], ids=[search_id(s) for s in CASES["searches"]])
def test_the_restatement_reproduces_the_recorded_searches(s):
    changes = s.get("changes")
    res = helpgraph_ref.search(MAPS[s["map"]], s["t_max"], s["mode"], s["param"], s["collect_gems"], changes=changes)
    assert (res.length, res.n_states, res.frontier, res.expanded) == (s["length"], s["states"], s["frontier"], s["expanded"])
    if res.plan is not None:
        edges = helpgraph_ref.check_plan(MAPS[s["map"]], res.plan, s["mode"], s["param"], s["collect_gems"], length=s["length"], changes=changes)
        assert edges == res.edges


# ------------------------------------------------------------------------------------------------ changed worlds
def recorded(map_name, mode="standard", param=2, collect_gems=False, changes=None):
    return next(s for s in CASES["searches"] if (s["map"], s["mode"], s["param"], s["collect_gems"], s.get("changes")) == (map_name, mode, param, collect_gems, changes))


OFF0 = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}]}
RECOLOURED = {"sources": [{"laser_id": 0, "enabled": None, "colour": 1}]}


def test_changes_reach_the_oracle_world_and_the_cache_key():
    """`changes` is applied before the reset and is part of the cache key; None is the map as written.  The figures are the ones the
    hook was specified with, worked out independently of it: on single-laser-asymmetric at t_max 6, source 0 disabled: `standard` finds
    length 2 with 17 records and no edges, `no-asymmetric` length 2 (no plan on the map as written); source 0 recoloured to 1:
    `standard` finds length 4 with the edge (1, 0), `no-asymmetric` no plan with 26 records."""
    text = MAPS["single-laser-asymmetric"]
    plain = helpgraph_ref.search(text, 6)
    assert helpgraph_ref.search(text, 6, changes=None) is plain and (plain.length, plain.n_states, plain.edges) == (2, 14, {(0, 1)})
    off = helpgraph_ref.search(text, 6, changes=OFF0)
    assert off is not plain and off is helpgraph_ref.search(text, 6, changes={"sources": [{"colour": None, "enabled": False, "laser_id": 0}]})
    assert (off.length, off.n_states, off.edges) == (2, 17, set())
    assert helpgraph_ref.search(text, 6, "no-asymmetric").length is None and helpgraph_ref.search(text, 6, "no-asymmetric", changes=OFF0).length == 2
    red = helpgraph_ref.search(text, 6, changes=RECOLOURED)
    assert (red.length, red.edges) == (4, {(1, 0)})
    none = helpgraph_ref.search(text, 6, "no-asymmetric", changes=RECOLOURED)
    assert (none.length, none.n_states) == (None, 26)
    assert helpgraph_ref.check_plan(text, red.plan, changes=RECOLOURED) == {(1, 0)}
    with pytest.raises(Exception):  # the plan of the recoloured world kills agent 0 on the map as written
        helpgraph_ref.check_plan(text, red.plan)
    w = helpgraph_ref.oracle_world(text, {"exits": [[1, 1], [2, 2]]})
    assert sorted(w.exit_pos) == [(1, 1), (2, 2)] and (1, 1) in {(i, j) for i, j, *_ in w.lasers()}  # an exit under the beam
    answers = helpgraph_ref.characterize(text, 6, changes=OFF0)
    assert answers["solvable"] and not answers["asymmetric"]() and helpgraph_ref.characterize(text, 6)["asymmetric"]()
    assert [helpgraph_ref.changes_label(c) for c in (None, OFF0, RECOLOURED, {"exits": [[1, 1], [2, 2]]})] == ["", "-source0-off", "-source0-colour1", "-exits-1.1-2.2"]


def test_changes_reach_a_world_of_the_package():
    """`apply_changes` does to an lle_amd.World, through its public mutators, what `oracle_world` does to the oracle's: the sources and
    the exits of the two agree afterwards (no device: a World parses on the host)."""
    for name, changes in (("single-laser-asymmetric", OFF0), ("single-laser-asymmetric", RECOLOURED), ("two-agent-mutual-compact", {"exits": [[3, 0], [2, 2]]}),
                          ("three-beam-cell", {"sources": [{"laser_id": 2, "enabled": False, "colour": None}, {"laser_id": 0, "colour": 1}], "exits": [[4, 1], [4, 3], [3, 2]]}),
                          ("paper-fully-coupled", None)):
        ours, theirs = helpgraph_ref.apply_changes(World(MAPS[name]), changes), helpgraph_ref.oracle_world(MAPS[name], changes)
        assert [(s.laser_id, s.agent_id, s.is_enabled) for s in ours.laser_sources] == [(l, src[3], bool(src[4])) for l, src in enumerate(theirs.sources())]
        assert sorted(ours.exit_pos) == sorted(theirs.exit_pos)
    w = helpgraph_ref.apply_changes(World(MAPS["single-laser-asymmetric"]), OFF0)
    assert [s.is_enabled for s in w.laser_sources] == [False] and [s.is_enabled for s in World(MAPS["single-laser-asymmetric"]).laser_sources] == [True]
    assert helpgraph_ref.apply_changes(w, {"sources": [{"laser_id": 0, "enabled": True}]}).laser_sources[0].is_enabled


# ------------------------------------------------------------------------------------------------ the maps of this project's making
NEW_MAPS = ("shared-colour", "three-beam-cell", "six-mutual", "six-converge")


def edges_by_source(text, plan, changes=None):
    """{laser_id: the (helper, beneficiary) pairs that source gives over the states of `plan`}, the rule of tests/coop_ref.py per source."""
    world = helpgraph_ref.oracle_world(text, changes)
    world.reset()
    out = {}
    for joint in [None] + list(plan):
        if joint is not None:
            world.step([int(a) for a in joint])
        on_beam = {}
        for i, j, laser_id, colour, _on, enabled in world.lasers():
            if enabled and world.tile_agent(i, j) >= 0:
                on_beam.setdefault((laser_id, colour), set()).add(world.tile_agent(i, j))
        for (laser_id, colour), agents in on_beam.items():
            if colour in agents and len(agents) > 1:
                out.setdefault(laser_id, set()).update((colour, b) for b in agents if b != colour)
    return out


@pytest.mark.parametrize("name", NEW_MAPS)
def test_a_new_map_discriminates(name):
    """Some recorded mode of the map differs from `standard` in length or frontier, and every new map is not one of the reference's."""
    mine = [s for s in CASES["searches"] if s["map"] == name and "changes" not in s and not s["collect_gems"]]
    standard = next(s for s in mine if s["mode"] == "standard")
    assert name in CASES["maps"] and standard["length"] is not None
    assert any((s["length"], s["frontier"]) != (standard["length"], standard["frontier"]) for s in mine)


def test_shared_colour_has_two_sources_of_one_colour():
    """Two laser_ids of colour 0 whose beams share no cell; the plan's edges come from the second source (and from the first: a rule that
    kept only one source per colour loses edges whichever it keeps)."""
    text = MAPS["shared-colour"]
    world = helpgraph_ref.oracle_world(text)
    assert [(src[3], bool(src[4])) for src in world.sources()] == [(0, True), (0, True)]
    cells = [{(i, j) for i, j, laser_id, *_ in world.lasers() if laser_id == l} for l in (0, 1)]
    assert cells[0] and cells[1] and not cells[0] & cells[1]
    res = helpgraph_ref.search(text, 6)
    assert edges_by_source(text, res.plan) == {0: {(0, 1)}, 1: {(0, 1)}} and res.edges == {(0, 1)}
    # without the second source's edges the plan would be independent of agent 0 from step 2 on: the beam is what agent 1 has to cross
    assert helpgraph_ref.search(text, 6, changes={"sources": [{"laser_id": 1, "enabled": False}]}).length == 3
    gems = helpgraph_ref.search(text, 6, collect_gems=True)
    assert (res.length, gems.length) == (3, 5) and (1, 3) in world.gem_pos and (1, 3) in cells[0]  # the gem lies under a beam, off the way


def test_three_beam_cell_has_three_beams_and_two_owners():
    """Three sources of three colours shine through (2, 2).  `World.lasers` -- the oracle's, the reference's and the package's -- lists
    the outer two layers of a cell and no more, so NO cell ever carries three laser ids there: the first source parsed, L1S, owns no
    tile at the crossing, and a cell word with three bits would be wrong.  The recorded plan has agent 1 on the crossing, helped along
    both listed beams; one beam lies over a start and an exit, two over the gem."""
    text = MAPS["three-beam-cell"]
    world = helpgraph_ref.oracle_world(text)
    step = {0: (-1, 0), 1: (0, 1), 2: (1, 0), 3: (0, -1)}  # Direction: N, E, S, W
    through = {}
    for l, (i, j, direction, colour, _enabled, length) in enumerate(world.sources()):
        for k in range(1, length + 1):
            through.setdefault((i + k * step[direction][0], j + k * step[direction][1]), []).append((l, colour))
    assert sorted(through[(2, 2)]) == [(0, 1), (1, 0), (2, 2)] and max(len(v) for v in through.values()) == 3
    listed = {}
    for i, j, laser_id, *_ in world.lasers():
        listed.setdefault((i, j), []).append(laser_id)
    assert listed[(2, 2)] == [2, 1] and max(len(v) for v in listed.values()) == 2  # outermost first; the two-layer rule
    assert {c for c, v in listed.items() if 0 in v} == {(1, 2), (3, 2), (4, 2)} and (1, 2) == tuple(world.start_pos[1]) and (4, 2) in world.exit_pos
    assert listed[(2, 3)] == [2, 1] and (2, 3) in world.gem_pos
    res = helpgraph_ref.search(text, 5)
    assert res.length == 4 and res.edges == {(0, 1), (0, 2), (2, 0), (2, 1)}
    world.reset()
    for joint in res.plan[:2]:
        world.step(joint)
    assert world.positions() == [(2, 1), (2, 2), (2, 3)]  # three agents on the two beams through the crossing, agent 1 on it
    assert edges_by_source(text, res.plan) == {1: {(0, 1), (0, 2)}, 2: {(2, 1), (2, 0)}}
    # with L2W disabled agent 1 stands on the crossing with agent 2 below it on L1S's beam -- and helps nobody from there
    off2 = {"sources": [{"laser_id": 2, "enabled": False, "colour": None}]}
    world = helpgraph_ref.oracle_world(text, off2)
    world.reset()
    for joint in ([1, 4, 1], [1, 4, 1], [4, 4, 1], [4, 1, 3]):
        world.step(joint)
    assert world.positions() == [(2, 1), (2, 2), (3, 2)] and all(world.alive())
    from tests import coop_ref
    assert coop_ref.detect(world) == {(0, 1)}


def test_six_agent_maps_use_both_help_words():
    for name, edges in (("six-mutual", {(3, 5), (5, 3)}), ("six-converge", {(3, 4), (3, 5), (5, 3), (5, 4)})):
        res = helpgraph_ref.search(MAPS[name], 3)
        bits = {8 * h + b for h, b in res.edges}
        assert res.edges == edges and min(bits) < 32 <= max(bits)
    assert {s["mode"] for s in CASES["searches"] if s["map"] == "six-mutual" and s["length"] is None} == {"no-mutual"}
    assert {(s["mode"], s["param"]) for s in CASES["searches"] if s["map"] == "six-converge" and s["length"] is None} == {("no-mutual", 2), ("no-convergence", 2), ("no-divergence", 2)}
    assert {(s["mode"], s["param"]) for s in CASES["searches"] if s["map"] == "six-converge" and s["length"] == 3} == {("standard", 2), ("no-divergence", 3), ("no-fully-coupled", 2)}


def test_a_map_in_the_far_corner_is_the_same_world():
    """`embed` puts a layout in the bottom-right corner of a map of walls: the restatement gives the small layout's recorded counters,
    so what tests/test_gpu_helpgraph_maps.py finds on the device with such a map is the device's."""
    s = recorded("two-agent-mutual-compact")
    for height, width in ((20, 20), (6, 255)):
        big = helpgraph_ref.embed(MAPS[s["map"]], height, width)
        world = helpgraph_ref.oracle_world(big)
        assert (world.height, world.width) == (height, width) and min(i * width + j for i, j, *_ in world.lasers()) > 255
        res = helpgraph_ref.search(big, s["t_max"])
        assert (res.length, res.frontier, res.expanded) == (s["length"], s["frontier"], s["expanded"])


def test_check_plan_refuses_what_a_mode_rejects():
    text = MAPS["two-agent-mutual-compact"]
    plan = helpgraph_ref.search(text, 6).plan
    assert helpgraph_ref.check_plan(text, plan, "no-asymmetric") == {(0, 1), (1, 0)}
    with pytest.raises(AssertionError):
        helpgraph_ref.check_plan(text, plan, "no-mutual")
    with pytest.raises(AssertionError):
        helpgraph_ref.check_plan(text, plan[:-1])
    single = MAPS["single-laser-asymmetric"]
    with pytest.raises(AssertionError):
        helpgraph_ref.check_plan(single, helpgraph_ref.search(single, 6).plan, "no-asymmetric")


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_logic_under_sanitizers(tmp_path):
    """tests/hostsim/helpgraph_logic.cpp: its own main over helpgraph_logic.hpp, built with g++ -fsanitize=address,undefined and run as a
    child process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "helpgraph_logic")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "helpgraph_logic.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        # every matrix of 2, 3 and 4 agents, 10 000 each of 5 and 6; 6 modes x the parameters 2 .. A + 1
        assert res.stdout.startswith("OK ") and int(out["matrices"]) == 4 + 64 + 4096 + 20000
        assert int(out["mode_checks"]) == 6 * (4 * 2 + 64 * 3 + 4096 * 4 + 10000 * 5 + 10000 * 6)
        assert int(out["states"]) == 4000 and int(out["with_edges"]) > 1000 and int(out["stored"]) > 100 and int(out["duplicates"]) > 1000
