"""The help-graph search on the MI355X where tests/test_gpu_helpgraph.py does not reach: cells at the far end of the cell table and of
the position bytes, worlds changed before the solver is constructed (a source disabled or recoloured, an exit moved under a beam), two
sources of one colour, a cell under three beams, and six-agent modes whose edges lie in both help words.  The same for the plain
search's byte-per-cell table of foreign beams (liblle_search.so, liblle_forest.so).

Every comparison is exact and is `assert_recorded` of tests/test_gpu_helpgraph.py: length, per-depth counters and stored records
against tests/golden/kat_helpgraph.json, which tests/test_helpgraph_cpu.py holds the restatement (tests/helpgraph_ref.py) to; every plan
replayed on the oracle under its mode and the entry's `changes`; the goal's help words equal to the replay's edges.

The recorded searches of the new maps and of the changed worlds that have fewer than six agents are in `LISTED` of
tests/test_gpu_helpgraph.py, whose test_counters_and_plans runs each with the default sizes and with chunk=64, max_states=16384
(test_the_new_searches_are_listed_there pins that); the six-agent ones run here, with the default sizes and with chunk=4096."""
import os
import re

import pytest

from tests import helpgraph_ref, search_ref
from tests.test_gpu_helpgraph import LISTED, MAPS, SEARCHES, assert_recorded, hg, mode_text, run, search_id  # noqa: F401  (hg: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_MAPS = ("shared-colour", "three-beam-cell", "six-mutual", "six-converge")
NEW = [s for s in SEARCHES if s["map"] in NEW_MAPS or "changes" in s]
SIX = [s for s in NEW if helpgraph_ref.n_agents_of(MAPS[s["map"]]) == 6]
COUNTERS = ("length", "frontier", "expanded", "n_states")


def of_map(name, changes=None):
    """The recorded searches of a map (without collect_gems) under `changes`."""
    return [s for s in SEARCHES if s["map"] == name and s.get("changes") == changes and not s["collect_gems"]]


def counters(stats):
    return {k: stats[k] for k in COUNTERS}


# ---------------------------------------------------------------------------------------------------------------- recorded searches
def test_the_new_searches_are_listed_there():
    assert len(NEW) == 31 and len(SIX) == 8 and {s["map"] for s in SIX} == {"six-mutual", "six-converge"}
    listed = [search_id(s) for s in LISTED]
    assert all(search_id(s) in listed for s in NEW if s not in SIX) and not any(search_id(s) in listed for s in SIX)
    assert {s["map"] for s in NEW if "changes" in s} == {"single-laser-asymmetric", "two-agent-mutual-compact", "three-beam-cell", "paper-fully-coupled"}


@pytest.mark.parametrize("config", ["defaults", "chunk4096"])
@pytest.mark.parametrize("s", SIX, ids=[search_id(s) for s in SIX])
def test_six_agents_with_edges_in_both_help_words(hg, s, config):
    """six-mutual: (3, 5) is bit 29 of the low help word, (5, 3) bit 11 of the high one; six-converge: helpers 3 and 5 of agent 4 lie in
    different words.  A mode judged on one word returns the 3-step plan where the recorded answer is None."""
    _plan, stats = assert_recorded(hg, s, **({} if config == "defaults" else dict(chunk=4096)))
    if s["length"] is not None:
        bits = {8 * h + b for h, b in stats["help_edges"]}
        assert min(bits) < 32 <= max(bits)


# ---------------------------------------------------------------------------------------------------------------- far corner
SIZES = [(20, 20), (64, 64), (65, 66), (6, 255), (255, 6)]
LDS_THREADS = 256  # HG_THREADS: cells staged per pass of the loop in hg_insert<true>


def test_the_sizes_are_the_ones_the_table_turns_at():
    source = open(os.path.join(ROOT, "lle_amd", "helpgraph", "helpgraph.hip")).read()
    lds_max = int(re.search(r"LDS_TABLE_MAX_BYTES = (\d+);", source).group(1))
    assert int(re.search(r"HG_THREADS = (\d+);", source).group(1)) == LDS_THREADS and "table_bytes <= lle::LDS_TABLE_MAX_BYTES" in source
    assert 20 * 20 == LDS_THREADS + 144, "two passes of the staging loop, the second partial"
    assert 64 * 64 * 4 == lds_max == 16384, "the largest table that goes to LDS"
    assert 65 * 66 * 4 > lds_max and 65 * 66 - 1 == 4289, "global memory"
    assert 6 * 255 * 4 <= lds_max and max(max(s) for s in SIZES) == 255 and "#define LLE_MAX_DIM 255" in open(os.path.join(ROOT, "include", "lle_hip.h")).read()


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("name", ["two-agent-mutual-compact", "paper-fully-coupled"])
def test_a_layout_in_the_far_corner(hg, name, size):
    """The layout in the bottom-right corner of a map of walls: every cell the search reads lies behind the first 256 of the table (at
    6 x 255 and 255 x 6 the coordinate bytes of agents on beams reach 253 and 254); counters, lengths and plans are the small layout's
    in every recorded mode."""
    height, width = size
    big = helpgraph_ref.embed(MAPS[name], height, width)
    if (name, size) == ("two-agent-mutual-compact", (20, 20)):  # the embedding itself, on the oracle, before any of it runs on the device
        s = next(s for s in of_map(name) if s["mode"] == "standard")
        ref = helpgraph_ref.search(big, s["t_max"])
        assert (ref.length, ref.frontier, ref.expanded) == (s["length"], s["frontier"], s["expanded"])
    from lle_amd import Map
    tiles = Map(big).laser_tiles()
    assert tiles and min(t.i * width + t.j for t in tiles) >= LDS_THREADS and max(t.i for t in tiles) >= height - 2 and max(t.j for t in tiles) >= width - 2
    recorded = of_map(name)
    assert len(recorded) == (3 if name == "two-agent-mutual-compact" else 6)
    for s in recorded:
        assert_recorded(hg, s, text=big, chunk=256, max_states=s["states"] + 1)
    assert ("hg_insert<true>" if height * width * 4 <= 16384 else "hg_insert<false>") in hg.launched_kernels()


# ---------------------------------------------------------------------------------------------------------------- build_rule
ALL_OFF = {"sources": [{"laser_id": l, "enabled": False, "colour": None} for l in range(3)]}
OFF0 = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}]}


def test_with_every_source_disabled_every_mode_is_the_plain_search(hg):
    """paper-fully-coupled with its three sources disabled: nobody can help anybody, so all six modes walk what Solver.find_shortest()
    walks on the same changed world, which is what the restatement recorded."""
    from lle_amd import Solver, World
    (recorded,) = of_map("paper-fully-coupled", ALL_OFF)
    text = MAPS["paper-fully-coupled"]
    plain = Solver(helpgraph_ref.apply_changes(World(text), ALL_OFF), recorded["t_max"])
    try:
        assert len(plain.find_shortest()) == recorded["length"] == 7
        want = counters(plain.last_stats)
    finally:
        plain.free()
    assert want == dict(length=recorded["length"], frontier=recorded["frontier"], expanded=recorded["expanded"], n_states=recorded["states"])
    for mode in helpgraph_ref.MODES:
        plan, stats = run(hg, text, recorded["t_max"], mode, 2, False, ALL_OFF)
        print(mode, stats)
        assert counters(stats) == want and stats["help_edges"] == set()
        assert helpgraph_ref.check_plan(text, plan, mode, length=7, changes=ALL_OFF) == set()


def test_the_sources_are_frozen_at_construction(hg):
    """A source disabled on the World after HelpGraphSolver(world, t) was constructed does not reach that solver (its handle is made by the
    first search, later still); a solver constructed afterwards answers for the changed world."""
    from lle_amd import World
    text = MAPS["single-laser-asymmetric"]
    before, after = of_map("single-laser-asymmetric")[0], of_map("single-laser-asymmetric", OFF0)[0]
    assert (before["mode"], before["states"], after["mode"], after["states"]) == ("standard", 14, "standard", 17)
    world = World(text)
    first = hg.HelpGraphSolver(world, 6)
    helpgraph_ref.apply_changes(world, OFF0)
    second = hg.HelpGraphSolver(world, 6)
    try:
        for solver, s, edges in ((first, before, {(0, 1)}), (second, after, set())):
            assert len(solver.find_shortest("standard")) == s["length"]
            assert counters(solver.last_stats) == dict(length=s["length"], frontier=s["frontier"], expanded=s["expanded"], n_states=s["states"])
            assert solver.last_stats["help_edges"] == edges
        assert first.find_shortest("no-asymmetric") is None and len(second.find_shortest("no-asymmetric")) == 2
    finally:
        first.free()
        second.free()


@pytest.mark.parametrize("name", ["two-agent-mutual-compact", "paper-fully-coupled"])
def test_parameters_beyond_the_agents(hg, name):
    """No agent has A distinct helpers or beneficiaries: no-convergence-k and no-divergence-k with k = A, A + 1 and 255 reject nothing and
    their counters are `standard`'s."""
    standard = next(s for s in of_map(name) if s["mode"] == "standard")
    A = helpgraph_ref.n_agents_of(MAPS[name])
    assert A == (2 if name == "two-agent-mutual-compact" else 3)
    for mode in ("no-convergence", "no-divergence"):
        for k in (A, A + 1, 255):
            assert_recorded(hg, dict(standard, mode=mode, param=k))


# ---------------------------------------------------------------------------------------------------------------- the plain search
@pytest.mark.parametrize("size", [(20, 20), (255, 6)], ids=["20x20", "255x6"])
def test_plain_search_with_a_foreign_beam_in_the_far_corner(size):
    """one-way-detour (tests/golden/kat_solver.json: cooperative up to 9 steps, independent from 10 on) in the bottom-right corner of a
    map of walls: the beam agent 1 must not stand on lies behind the first 256 bytes of the foreign-beam table, which search_insert<true>
    stages in LDS with a loop of stride 256 and the forest reads from global memory.  Counters, per mode, are those of
    tests/search_ref.py on the small layout."""
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import Map, Solver
    from lle_amd.forest import ForestSolver
    case = next(c for c in search_ref.load_cases()["catalogue"] if c["name"] == "one-way-detour")
    small, t_max = case["map"], 11
    assert case["expect"]["9"]["cooperative"] is True and case["expect"]["10"]["independent"] is True
    height, width = size
    big = helpgraph_ref.embed(small, height, width)
    tiles = Map(big).laser_tiles()
    assert tiles and min(t.i * width + t.j for t in tiles) >= 256
    for mode, length in (("standard", 6), ("no-cooperation", 10)):
        ref = search_ref.search(small, t_max, mode)
        assert ref.length == length
        s, f = Solver(big, t_max, chunk=256, max_states=ref.n_states + 1), ForestSolver([big], t_max, max_states_per_map=1024)
        try:
            plan = s.find_shortest(mode)
            stats, res = s.last_stats, f.run(mode)
        finally:
            s.free()
            f.free()
        print(size, mode, stats, res.frontier[0], res.expanded[0])
        assert counters(stats) == dict(length=ref.length, frontier=ref.frontier, expanded=ref.expanded, n_states=ref.n_states)
        search_ref.check_plan(big, [[a.value for a in row] for row in plan], mode, length=ref.length)
        assert (int(res.status[0]), int(res.length[0]), res.frontier[0], res.expanded[0], int(res.n_states[0])) == (0, ref.length, ref.frontier, ref.expanded, ref.n_states)
        search_ref.check_plan(big, [[a.value for a in row] for row in res.plans[0]], mode, length=ref.length)
