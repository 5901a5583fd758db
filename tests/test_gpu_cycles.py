"""The closed-trail search on the MI355X (liblle_cycles.so, lle_amd.cycles) against the reference's stated `interdependent` values for
orders >= 3 (tests/golden/kat_cycles.json: `catalogue`) and against the restatement of the search over the oracle
(tests/cycles_ref.py), whose per-depth counters for every listed search are recorded in the same file (`searches`;
tests/test_cycles_cpu.py holds the restatement to every one of them, so no test here walks a search in Python).  The counters pin the
identity of a record -- the packed triples and their pruning rule included -- the walk over one state's arcs, the enumeration of joint
actions and the piece boundaries; every plan is replayed on the oracle and its closed trails found by the package's host-side graph.

Every search runs in pieces of 65 536 and of 64 work items, and the two give equal counters: in pieces of 64, candidates with equal key
words meet as tags inside a piece (their 3 or 21 value words are worked out again by the comparing lane) and as pool records across
pieces.

The shapes at which the kernels can go wrong, by the map that holds them (tests/golden/make_kat_cycles.py draws them):
  closes-in-one-state         an order-3 trail that closes only if two arcs of ONE state chain (0 -> 1 -> 2 at the reset, 2 -> 0 later); the
                              reset state already has edges and is stored
  three-agent-temporal-cycle  a closure across time
  cycle-against-time          the flattened relation is a 3-cycle, the times decrease along it: a plan under N = 3
  revisited-anchor            0 -> 1 -> 0 -> 2 -> 0: order 3 only through the closed triple (0, 0, {0, 1})
  ring-of-four                an order-4 ring without an order-3 trail: a plan under N = 3, none under N = 4
  two-agent-mutual-compact    a mutual pair held over a STAY under native order 2
  mutual-at-reset             a reset state the mode rejects: no plan, one record
  six-mutual, six-converge    six agents at N = 2 and 3: agent 5's bits, the 21-word class
  gem-detour                  collect_gems=True
  closes-in-one-state under `changes`: its last source off, its last source recoloured
  twins and merges            at chunk 64 on nearly every entry (tests/test_cycles_cpu.py counts both in the restatement)

Catalogue layouts LEFT OUT, by name: level-6 (the pool overflows as the plain search's does), fully-coupled-4agents (no plan through
World.step), eight-agent-interdependent-8 and eight-agent-interdependent-8-perimeter (more than six agents).
"""
import pytest

from tests import cycles_ref

pytestmark = pytest.mark.gpu

CASES = cycles_ref.load_cases()
CATALOGUE = {c["name"]: c for c in CASES["catalogue"]}
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"]}, **CASES["maps"])
SEARCHES = CASES["searches"]
CONFIGS = {"chunk65536": dict(chunk=65536), "chunk64": dict(chunk=64, max_states=32768)}


def search_id(s):
    return f"{s['map']}{cycles_ref.changes_label(s.get('changes'))}-t{s['t_max']}-n{s['n']}" + ("-gems" if s["collect_gems"] else "")


def recorded(map_name, n, collect_gems=False, changes=None):
    return next(s for s in SEARCHES if (s["map"], s["n"], s["collect_gems"], s.get("changes")) == (map_name, n, collect_gems, changes))


@pytest.fixture(scope="module")
def cy():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import cycles
    return cycles


def values(plan):
    return None if plan is None else [[a.value for a in row] for row in plan]


def world_of(text, changes=None):
    if changes is None:
        return text
    from lle_amd import World
    return cycles_ref.apply_changes(World(text), changes)


def assert_recorded(cy, s, text=None, **options):
    """One search of the golden file: length, counters and state count equal the restatement's; the plan replays on the oracle (under
    the entry's `changes`) without a closed trail of order N, with exactly the closed orders below N and the triples the device reports."""
    text = MAPS[s["map"]] if text is None else text
    solver = cy.CycleSolver(world_of(text, s.get("changes")), s["t_max"], **options)
    try:
        plan = values(solver.shortest_without_closed_trail(s["n"], collect_gems=s["collect_gems"]))
        stats = solver.last_stats
    finally:
        solver.free()
    print(f"{search_id(s)} {options}: length {stats['length']} (ref {s['length']}), states {stats['n_states']} (ref {s['states']}), frontier {stats['frontier']}, "
          f"expanded {stats['expanded']}, closed orders {stats['closed_orders']}")
    assert stats["length"] == s["length"] and (plan is None) == (s["length"] is None)
    assert stats["frontier"] == s["frontier"] and stats["expanded"] == s["expanded"] and stats["n_states"] == s["states"]
    if plan is None:
        assert stats["triples"] is None and stats["closed_orders"] is None
    else:
        cycles_ref.check_plan(text, plan, s["n"], s["collect_gems"], length=s["length"], changes=s.get("changes"), triples=stats["triples"],
                              closed_orders=stats["closed_orders"])
    return plan, stats


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("s", SEARCHES, ids=[search_id(s) for s in SEARCHES])
def test_counters_and_plans(cy, s, config):
    assert_recorded(cy, s, **CONFIGS[config])


def test_the_shapes_are_listed():
    """Every shape the module's docstring names has its searches in the golden file, with the outcome that shows it."""
    got = {(s["map"], s["n"], s["collect_gems"], cycles_ref.changes_label(s.get("changes"))): s for s in SEARCHES}
    rows = [("closes-in-one-state", 3, None), ("closes-in-one-state", 2, 5), ("three-agent-temporal-cycle", 3, None), ("cycle-against-time", 3, 5),
            ("revisited-anchor", 3, None), ("revisited-anchor", 2, None), ("ring-of-four", 3, 6), ("ring-of-four", 4, None), ("two-agent-mutual-compact", 2, None),
            ("mutual-at-reset", 2, None), ("six-mutual", 2, None), ("six-mutual", 3, 3), ("six-converge", 2, None), ("six-converge", 3, 3)]
    for name, n, length in rows:
        assert got[(name, n, False, "")]["length"] == length, (name, n)
    assert got[("closes-in-one-state", 3, False, "")]["states"] > 1, "the reset state with its two chained arcs is stored and expanded"
    rejected = got[("mutual-at-reset", 2, False, "")]
    assert (rejected["states"], rejected["frontier"], rejected["expanded"]) == (1, [1], [])
    assert got[("gem-detour", 2, True, "")]["states"] != got[("gem-detour", 2, False, "")]["states"]
    changed = [s for s in SEARCHES if "changes" in s]
    assert [(s["map"], s["n"], s["length"]) for s in changed] == [("closes-in-one-state", 3, 4), ("closes-in-one-state", 3, 6)]
    assert changed[0]["changes"]["sources"][0]["enabled"] is False and changed[1]["changes"]["sources"][0]["colour"] == 1
    stated = {(name, int(t), int(n)) for name, c in CATALOGUE.items() for t, e in c["expect"].items() for n in e["interdependent"]}
    assert len(stated) == 25 and all(n >= 3 for _name, _t, n in stated)


def test_the_ring_of_four_closes_no_order_three(cy):
    """ring-of-four: the plan under N = 3 holds the ring 0 -> 1 -> 2 -> 3 -> 0 and no closed trail over two or three agents."""
    plan, stats = assert_recorded(cy, recorded("ring-of-four", 3))
    assert stats["closed_orders"] == [] and 3 not in stats["closed_orders"]
    _R, edges, _w = cycles_ref.replay_triples(MAPS["ring-of-four"], plan)
    assert {(h, b) for h, b, _t in edges} == {(0, 1), (1, 2), (2, 3), (3, 0)}
    full = cycles_ref.replay_triples(MAPS["ring-of-four"], plan)[0]
    assert cycles_ref.closes(full, 4) and not cycles_ref.closes(full, 3) and not cycles_ref.closes(full, 2)


def test_the_flattened_view_would_be_wrong(cy):
    """cycle-against-time: every plan's flattened relation is the 3-cycle 0 -> 1 -> 2 -> 0; no closed trail exists, is_interdependent(3)
    is False."""
    from lle_amd import World
    text = MAPS["cycle-against-time"]
    c = cy.CycleCharacterizer(World(text), 7)
    try:
        assert c.is_interdependent(3) is False and c.is_solvable() and c.is_cooperative()
        _R, edges, _w = cycles_ref.replay_triples(text, values(c.shortest_path))
        assert {(h, b) for h, b, _t in edges} == {(0, 1), (1, 2), (2, 0)}
        assert c._solver.h is None, "the shortest plan's profile said no: no native search was needed"
        assert values(c.compute_shortest_non_interdependent_path(3)) is not None and c._solver.h is not None
    finally:
        c._solver.free()


# ---------------------------------------------------------------------------------------------------------------- characterizer
@pytest.mark.parametrize("name", sorted(CATALOGUE))
def test_characterizer(cy, name):
    """CycleCharacterizer.is_interdependent gives what python/tests/world_layouts.py states for the layout at every stated t_max and
    every stated order >= 3, orders above the map's agents included."""
    from lle_amd import World
    case = CATALOGUE[name]
    for t, expect in sorted(case["expect"].items(), key=lambda kv: int(kv[0])):
        c = cy.CycleCharacterizer(World(case["map"]), int(t))
        try:
            got = {n: c.is_interdependent(int(n)) for n in expect["interdependent"]}
            print(name, t, got)
            assert got == expect["interdependent"]
            for n in expect["interdependent"]:
                plan = values(c.compute_shortest_non_interdependent_path(int(n)))
                assert (plan is None) == expect["interdependent"][n]  # (every layout here is solvable at its t_max)
                if plan is not None and int(n) <= c.world.n_agents:
                    cycles_ref.check_plan(case["map"], plan, int(n))
        finally:
            c._solver.free()


def test_generator_atom(cy):
    from lle_amd import Constraint, Interdependent, World
    w = World(MAPS["paper-interdependent-3"])
    assert Constraint(10, Interdependent(3)).is_satisfied_by(w, characterizer=cy.CycleCharacterizer) is True
    assert Constraint(7, ~Interdependent(3)).is_satisfied_by(World(MAPS["cycle-against-time"]), characterizer=cy.CycleCharacterizer) is True


# ---------------------------------------------------------------------------------------------------------------- shapes
def test_cell_table_in_global_memory(cy):
    """closes-in-one-state (3 words) in the far corner of a 65 x 66 map of walls -- 4 290 cells are more than 16 KB of table -- and
    six-mutual (21 words, staged up to 8 KB) in that of a 46 x 46 one -- 2 116 cells, more than 8 KB; a larger six-agent map does not fit
    the step kernel's own tables --: the insert kernel reads the table from global memory; the counters are the small layout's."""
    from tests import helpgraph_ref
    for name, n, size in (("closes-in-one-state", 3, (65, 66)), ("six-mutual", 3, (46, 46))):
        assert_recorded(cy, recorded(name, n), text=helpgraph_ref.embed(MAPS[name], *size), chunk=4096, max_states=8192)
    assert {"cy_insert<false, 3>", "cy_insert<false, 21>"} <= set(cy.launched_kernels())


def test_exact_fit_pool(cy):
    """A pool of exactly the records the search stores succeeds; one record fewer raises SolverCapacityError."""
    from lle_amd import SolverCapacityError
    s = recorded("cycle-against-time", 3)
    assert_recorded(cy, s, chunk=64, max_states=s["states"])
    solver = cy.CycleSolver(MAPS[s["map"]], s["t_max"], chunk=64, max_states=s["states"] - 1)
    try:
        with pytest.raises(SolverCapacityError, match=f"max_states = {s['states'] - 1}"):
            solver.find_shortest("no-interdependence-3")
        assert solver._cache == {}
    finally:
        solver.free()


def test_solver_reuse(cy):
    """One solver, one handle: N = 2 and 3, collect_gems on and off, each with its own counters; the modes route as the class says."""
    from lle_amd import TrailSolver
    s = cy.CycleSolver(MAPS["gem-detour"], 8)
    try:
        for n, gems in ((2, True), (2, False), (2, True)):
            assert s.shortest_without_closed_trail(n, collect_gems=gems) is None
            want = recorded("gem-detour", n, gems)
            assert (s.last_stats["frontier"], s.last_stats["expanded"], s.last_stats["n_states"]) == (want["frontier"], want["expanded"], want["states"])
        handle = s.h
        assert handle is not None and s._inner is None
        plan = s.find_shortest("no-interdependence-3")  # above the two agents: the standard answer, no native search
        assert len(plan) == 5 and type(s._inner) is TrailSolver and "triples" not in s.last_stats and s.h == handle
        s.find_shortest("no-mutual")
        assert "triples" not in s.last_stats and "help_edges" in s.last_stats  # order 2 as a mode stays the flattened relation's
        assert len(s.find_shortest("no-sequence-3")) == 5
    finally:
        s.free()
    s = cy.CycleSolver(MAPS["six-mutual"], 3)
    try:
        assert s.find_shortest("no-interdependence-3") is not None and s.last_stats["n_states"] == recorded("six-mutual", 3)["states"]
        assert s.last_stats["closed_orders"] == [2] and any(a == c and agents == frozenset({3, 5}) for a, c, agents in s.last_stats["triples"])
        assert s.shortest_without_closed_trail(2) is None and s.last_stats["n_states"] == recorded("six-mutual", 2)["states"]
    finally:
        s.free()


def test_every_kernel_was_launched(cy):
    """At the end of this file: the searches above have gone through every kernel the library holds."""
    assert sorted(cy.launched_kernels()) == sorted(cy.compiled_kernels()) and len(cy.compiled_kernels()) == 7
