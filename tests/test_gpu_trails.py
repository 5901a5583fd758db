"""The trail search on the MI355X (liblle_trails.so, lle_amd.trails) against the reference's stated `sequential` values
(tests/golden/kat_trails.json: `catalogue`) and against the restatement of the search over the oracle (tests/trails_ref.py), whose
per-depth counters for every listed search are recorded in the same file (`searches`; tests/test_trails_cpu.py holds the restatement to
every one of them, so no test here walks a search in Python).  The counters pin the identity of a record -- the trail word included --
the walk over one state's arcs, the enumeration of joint actions and the piece boundaries; every plan is replayed on the oracle and its
longest trail measured by the package's host-side graph.

Every search runs in pieces of 65 536 and of 64 work items, and the two give equal counters: in pieces of 64, candidates with equal key
words meet as tags inside a piece and as pool records across pieces.

The shapes at which the kernels can go wrong, by the map that holds them (tests/golden/make_kat_trails.py draws them):
  chain-in-one-state        two arcs of one state chain: 0 -> 1 and 1 -> 2 at the same t, a trail of 2 from one layer
  three-beam-cell           a same-state mutual pair and a cycle inside one layer: 0 <-> 2, 0 -> 1, 2 -> 1, a trail of 3 at once
  two-agent-mutual-compact  a mutual pair held over a STAY: the trails grow by 2 per step while the flattened relation stands still
  decreasing-times          1 -> 2 at t, 0 -> 1 later: length 1, a plan under no-sequence-2
  chain-at-reset            a reset state that already has edges (N = 3), and one the mode rejects (N = 2: length -1, one record)
  decreasing-times, two-agent-mutual-compact, six-mutual
                            two candidates of one piece reach one world state: stored twice under different trail words, once under
                            equal ones from different parents (tests/test_trails_cpu.py counts both in the restatement)
  six-mutual, six-converge  six agents: an edge into agent 5's field, bits 20-23
  N = 2 everywhere; N = 4 | 5 on two-agent-mutual-compact and N = 7 | 8 on three-beam-cell: the largest N the horizon can reach, and
                            the first that rejects nothing (equal to N = 16)
  gem-detour                collect_gems=True
  long-trails and every entry with `changes`
                            trail fields up to 15, a frontier that runs empty, worlds changed before the construction: what they are
                            for and what else is asked of them is in tests/test_gpu_trails_edges.py; their counters and plans run here too

Catalogue layouts LEFT OUT of the comparison on the device, by name:
  level-6                                 at t_max 21 the default pool of 4 194 304 records overflows, as the plain search's does at depth 11
  eight-agent-interdependent-8            more than six agents (and the reference states no `sequential` for it)
  eight-agent-interdependent-8-perimeter  more than six agents (likewise)
Every other layout that states `sequential` is held to its stated values at its own t_max below, the four that are beyond the
restatement's reach in test time included.
"""
import ctypes as C

import pytest

from tests import trails_ref

pytestmark = pytest.mark.gpu

CASES = trails_ref.load_cases()
CATALOGUE = {c["name"]: c for c in CASES["catalogue"]}
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"] if "map" in c}, **CASES["maps"])
SEARCHES = CASES["searches"]
CONFIGS = {"chunk65536": dict(chunk=65536), "chunk64": dict(chunk=64, max_states=16384)}
LEFT_OUT = {"level-6": "the default pool of 4 194 304 records overflows at t_max 21"}
ON_THE_DEVICE = ["one-way-detour", "single-laser-asymmetric", "sequence-4-with-mutual", "sequence-3-without-cycle", "paper-sequence-2",
                 "paper-sequence-2-not-interdependent-3", "paper-convergent-2", "two-agent-mutual-with-detours", "temporal-flattening-counterexample",
                 "three-agent-temporal-cycle", "three-agent-with-two-agent-cycle", "paper-interdependent-3", "four-agent-interdependent-4-sequence-6"]


def search_id(s):
    return f"{s['map']}{trails_ref.changes_label(s.get('changes'))}-t{s['t_max']}-n{s['n']}" + ("-gems" if s["collect_gems"] else "")


def recorded(map_name, n, collect_gems=False, changes=None):
    """The first recorded search of the map under `changes` (None: the unchanged world) with this N."""
    return next(s for s in SEARCHES if (s["map"], s["n"], s["collect_gems"], s.get("changes")) == (map_name, n, collect_gems, changes))


@pytest.fixture(scope="module")
def tr():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import trails
    return trails


def values(plan):
    return None if plan is None else [[a.value for a in row] for row in plan]


def world_of(text, changes=None):
    """What the solver is constructed over: the map text, or an lle_amd.World with `changes` applied before the construction."""
    if changes is None:
        return text
    from lle_amd import World
    return trails_ref.apply_changes(World(text), changes)


def run(tr, text, t_max, n, collect_gems=False, changes=None, **options):
    """(plan as rows of action values or None, last_stats) of one fresh TrailSolver over the world under `changes`."""
    s = tr.TrailSolver(world_of(text, changes), t_max, **options)
    try:
        plan = values(s.find_shortest(f"no-sequence-{n}", collect_gems=collect_gems))
        return plan, s.last_stats
    finally:
        s.free()


def assert_recorded(tr, s, text=None, **options):
    """One search of the golden file: length, counters and state count equal the restatement's; the plan replays on the oracle (under
    the entry's `changes`) with a longest trail below N, and the goal's trail word is the L of that replay."""
    text = MAPS[s["map"]] if text is None else text
    plan, stats = run(tr, text, s["t_max"], s["n"], s["collect_gems"], s.get("changes"), **options)
    print(f"{search_id(s)} {options}: length {stats['length']} (ref {s['length']}), states {stats['n_states']} (ref {s['states']}), frontier {stats['frontier']}, "
          f"expanded {stats['expanded']}, trails {stats['trail_lengths']}")
    assert stats["length"] == s["length"] and (plan is None) == (s["length"] is None)
    assert stats["frontier"] == s["frontier"] and stats["expanded"] == s["expanded"] and stats["n_states"] == s["states"]
    if plan is None:
        assert stats["trail_lengths"] is None and stats["longest_trail"] is None
    else:
        L = trails_ref.check_plan(text, plan, s["n"], s["collect_gems"], length=s["length"], changes=s.get("changes"))
        assert tuple(stats["trail_lengths"]) == L and stats["longest_trail"] == max(L) < s["n"], "the goal's trail word is the L of the plan's replay"
    return plan, stats


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("s", SEARCHES, ids=[search_id(s) for s in SEARCHES])
def test_counters_and_plans(tr, s, config):
    assert_recorded(tr, s, **CONFIGS[config])


def test_the_shapes_are_listed():
    """Every shape the module's docstring names has its searches in the golden file, with the outcome that shows it."""
    rows = [("chain-in-one-state", 2, None), ("chain-in-one-state", 3, 5), ("chain-at-reset", 2, None), ("chain-at-reset", 3, 3), ("decreasing-times", 2, 6),
            ("two-agent-mutual-compact", 2, None), ("two-agent-mutual-compact", 3, 5), ("two-agent-mutual-compact", 4, 5), ("two-agent-mutual-compact", 5, 5),
            ("two-agent-mutual-compact", 16, 5), ("three-beam-cell", 2, None), ("three-beam-cell", 3, None), ("three-beam-cell", 4, 4), ("three-beam-cell", 7, 4),
            ("three-beam-cell", 8, 4), ("three-beam-cell", 16, 4), ("six-mutual", 2, None), ("six-mutual", 3, 3), ("six-converge", 3, 3)]
    assert set(rows) <= {(s["map"], s["n"], s["length"]) for s in SEARCHES if not s["collect_gems"]}
    assert {(s["n"], s["length"]) for s in SEARCHES if s["collect_gems"]} == {(2, None), (3, 7)} and {s["map"] for s in SEARCHES if s["collect_gems"]} == {"gem-detour"}
    assert (recorded("chain-at-reset", 2)["states"], recorded("chain-at-reset", 2)["frontier"], recorded("chain-at-reset", 2)["expanded"]) == (1, [1], [])
    # the mutual pair held over a STAY: no-sequence-3 changes answer and record count against no-sequence-2, and the largest N counts
    compact = [recorded("two-agent-mutual-compact", n)["states"] for n in (2, 3, 4, 5, 16)]
    assert compact == [100, 119, 125, 126, 126] and recorded("three-beam-cell", 7)["states"] + 1 == recorded("three-beam-cell", 8)["states"] == recorded("three-beam-cell", 16)["states"]
    assert set(LEFT_OUT) | set(ON_THE_DEVICE) == set(CATALOGUE) and not set(LEFT_OUT) & set(ON_THE_DEVICE)


# ---------------------------------------------------------------------------------------------------------------- characterizer
@pytest.mark.parametrize("name", ON_THE_DEVICE)
def test_characterizer(tr, name):
    """TrailCharacterizer.is_sequential gives what python/tests/world_layouts.py states for the layout at every stated t_max; every
    no-sequence-N plan it finds on the way has a longest trail below N on the oracle."""
    from lle_amd import World
    case = CATALOGUE[name]
    for t, expect in sorted(case["expect"].items(), key=lambda kv: int(kv[0])):
        c = tr.TrailCharacterizer(World(case["map"]), int(t))
        try:
            got = {n: c.is_sequential(int(n)) for n in expect["sequential"]}
            print(name, t, got, c._solver.last_stats and c._solver.last_stats["n_states"])
            assert got == expect["sequential"]
            assert c.is_solvable()
            for n in expect["sequential"]:
                plan = values(c.compute_shortest_path_without_sequence(int(n)))
                assert (plan is None) == expect["sequential"][n]  # solvable: sequential exactly when no plan avoids the trail
                if plan is not None:
                    assert max(trails_ref.check_plan(case["map"], plan, int(n))) < int(n)
        finally:
            c._solver.free()


def test_the_flattening_counterexample_differs_from_the_flattened_relation(tr):
    """decreasing-times: the flattened relation of every plan chains 0 -> 1 -> 2, the times never do.  is_sequential(2) is False although
    the shortest plan's flattened relation holds a path of two arcs."""
    from lle_amd import World
    text = MAPS["decreasing-times"]
    c = tr.TrailCharacterizer(World(text), 8)
    try:
        assert c.is_sequential(2) is False and c.is_solvable() and c.is_cooperative()
        plan = values(c.shortest_path)
        _L, edges, _w = trails_ref.replay_trails(text, plan)
        assert {(0, 1), (1, 2)} <= {(h, b) for h, b, _t in edges}
    finally:
        c._solver.free()


def test_generator_atoms(tr):
    """Constraint(t, Sequential(N)).is_satisfied_by(w, characterizer=TrailCharacterizer), alone and combined; the default characterizer
    still raises."""
    from lle_amd import Constraint, Cooperative, Sequential, World
    w = World(MAPS["sequence-3-without-cycle"])
    assert Constraint(6, Sequential(3)).is_satisfied_by(w, characterizer=tr.TrailCharacterizer) is True
    assert Constraint(6, Sequential(4)).is_satisfied_by(w, characterizer=tr.TrailCharacterizer, chunk=4096) is False
    assert Constraint(6, Cooperative() & ~Sequential(4)).is_satisfied_by(w, characterizer=tr.TrailCharacterizer) is True
    assert Constraint(6, Cooperative() & ~Sequential(3)).is_satisfied_by(World(MAPS["two-agent-mutual-with-detours"]), characterizer=tr.TrailCharacterizer) is True
    with pytest.raises(NotImplementedError):
        Constraint(6, Sequential(3)).is_satisfied_by(w)


# ---------------------------------------------------------------------------------------------------------------- shapes
def test_cell_table_in_global_memory(tr):
    """chain-in-one-state in the top-left corner of a 65 x 66 map of walls: 4 290 cells are more than 16 KB of table, so the insert kernel
    reads it from global memory; the counters are the small layout's."""
    rows = [line.split() for line in MAPS["chain-in-one-state"].strip().splitlines()]
    big = "\n".join(" ".join((rows[i][j] if i < len(rows) and j < len(rows[0]) else "@") for j in range(66)) for i in range(65))
    for n in (2, 3):
        assert_recorded(tr, recorded("chain-in-one-state", n), text=big, chunk=256, max_states=1024)
    assert "tr_insert<false>" in tr.launched_kernels()


def test_collect_gems_changes_the_length(tr):
    without, with_gems = recorded("gem-detour", 3), recorded("gem-detour", 3, True)
    s = tr.TrailSolver(MAPS["gem-detour"], 8)  # one handle, both searches: the gem word joins the identity per run
    try:
        assert len(s.find_shortest("no-sequence-3")) == 5 and s.last_stats["frontier"] == without["frontier"]
        plan = values(s.find_shortest("no-sequence-3", collect_gems=True))
        assert len(plan) == 7 and s.last_stats["frontier"] == with_gems["frontier"] and s.last_stats["expanded"] == with_gems["expanded"]
        trails_ref.check_plan(MAPS["gem-detour"], plan, 3, collect_gems=True)
        assert len(s.find_shortest("no-sequence-3")) == 5 and s.last_stats["n_states"] == without["states"]  # (cached per mode and collect_gems)
    finally:
        s.free()


def test_interface_on_the_device(tr):
    """STAY padding, solve(path_length), the delegated modes beside the native one, and the cache."""
    from lle_amd import Action, HelpGraphSolver
    text = MAPS["two-agent-mutual-compact"]
    s, hg = tr.TrailSolver(text, 8), HelpGraphSolver(text, 8)
    try:
        plan = s.find_shortest("no-sequence-3", t_min=7)
        assert len(plan) == 7 and plan[5:] == [(Action.STAY, Action.STAY)] * 2 and s.last_stats["trail_lengths"] == [2, 1] and s.last_stats["longest_trail"] == 2
        assert len(s.solve(8, mode="no-sequence-3")) == 8 and s.solve(4, mode="no-sequence-3") is None
        assert s.find_shortest("no-sequence") is None and s.find_shortest("no-sequence-2") is None and s.last_stats["length"] is None
        assert s.last_stats["trail_lengths"] is None and s.last_stats["longest_trail"] is None
        assert s.find_shortest("no-mutual") is None and hg.find_shortest("no-mutual") is None and s.last_stats == hg.last_stats
        assert len(s.find_shortest("no-asymmetric")) == len(hg.find_shortest("no-asymmetric")) == 5 and s.last_stats == hg.last_stats
        assert values(s.find_shortest("no-cooperation")) == values(hg.find_shortest("no-cooperation"))
        with pytest.raises(NotImplementedError, match="no-interdependence-3"):
            s.find_shortest("no-interdependence-3")
    finally:
        s.free()
        hg.free()


def test_capacity(tr):
    """A pool of 16 records overflows on paper-sequence-2: SolverCapacityError, no partial plan, and the solver object still answers."""
    from lle_amd import SolverCapacityError
    s = tr.TrailSolver(MAPS["paper-sequence-2"], 10, max_states=16)
    try:
        for mode in ("no-sequence-2", "no-sequence-3"):
            with pytest.raises(SolverCapacityError, match="max_states = 16"):
                s.find_shortest(mode)
        assert s._cache == {}
    finally:
        s.free()


def test_run_refusals_and_results_on_a_handle(tr):
    """Wrong struct_bytes, N out of range, negative t_max on a live handle; the result's trail word; lle_trails_plan after a run without a
    plan; a reset state the mode rejects."""
    from lle_amd import Map
    L = tr.lib()
    map_ = Map(MAPS["chain-at-reset"])  # (kept: the handle of a temporary would be freed before the call)
    h = L.lle_trails_create(map_.h, None)
    assert h, L.lle_trails_last_error()
    try:
        A, R = tr.TrailArgs, tr.TrailResult
        res = R(C.sizeof(R))
        for args, result, word in ((A(4, 2, 0, 5), res, b"lle_trails_args.struct_bytes"), (A(C.sizeof(A), 2, 0, 5), R(8), b"lle_trails_result.struct_bytes"),
                                   (A(C.sizeof(A), 1, 0, 5), res, b"length_n"), (A(C.sizeof(A), 17, 0, 5), res, b"length_n"), (A(C.sizeof(A), 2, 0, -1), res, b"t_max")):
            assert L.lle_trails_run(h, C.byref(args), C.byref(result)) == -2 and word in L.lle_trails_last_error()
        assert L.lle_trails_run(h, None, C.byref(res)) == -1 and L.lle_trails_run(h, C.byref(A(C.sizeof(A), 2, 0, 5)), None) == -1
        assert L.lle_trails_run(h, C.byref(A(C.sizeof(A), 3, 0, 6)), C.byref(res)) == 0
        assert (res.length, res.n_states, res.depth_reached, res.trail, res.step_errors) == (3, 19, 3, 0x210, 0)  # L = (0, 1, 2)
        buf = (C.c_uint8 * 9)()
        assert L.lle_trails_plan(h, buf, 8) == -2 and L.lle_trails_plan(h, None, 9) == -2 and L.lle_trails_plan(h, buf, 9) == 3
        frontier, expanded = (C.c_int64 * 8)(), (C.c_int64 * 8)()
        assert L.lle_trails_stats(h, frontier, expanded, 8) == 4 and list(frontier[:4]) == [1, 9, 6, 3] and list(expanded[:3]) == [16, 77, 28]
        assert L.lle_trails_run(h, C.byref(A(C.sizeof(A), 16, 0, 6)), C.byref(res)) == 0 and (res.length, res.n_states, res.trail) == (3, 19, 0x210)
        assert L.lle_trails_run(h, C.byref(A(C.sizeof(A), 3, 0, 2)), C.byref(res)) == 0 and (res.length, res.n_states, res.depth_reached, res.trail) == (-1, 16, 2, 0)
        # the reset state holds 0 -> 1 -> 2: no-sequence-2 rejects it -- no plan, one record, no level
        assert L.lle_trails_run(h, C.byref(A(C.sizeof(A), 2, 0, 6)), C.byref(res)) == 0
        assert (res.length, res.n_states, res.depth_reached, res.trail) == (-1, 1, 0, 0)
        assert L.lle_trails_plan(h, buf, 9) == -2 and b"no plan" in L.lle_trails_last_error()
        assert L.lle_trails_stats(h, frontier, expanded, 8) == 1 and frontier[0] == 1 and L.lle_trails_stats(h, None, None, 0) == 1
    finally:
        L.lle_trails_free(h)


def test_every_kernel_was_launched(tr):
    """At the end of this file: the searches above have gone through every kernel the library holds."""
    assert sorted(tr.launched_kernels()) == sorted(tr.compiled_kernels()) == ["tr_commit", "tr_expand", "tr_insert<false>", "tr_insert<true>"]
