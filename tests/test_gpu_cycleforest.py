"""The cycle forest on the MI355X (liblle_cycleforest.so, lle_amd.cycleforest, lle_amd.generator) against the restatement of the
closed-trail search over the oracle (tests/cycles_ref.py), whose per-map figures for every (set, order) of tests/cycleforest_ref.py are
recorded in tests/golden/kat_cycleforest.json (tests/test_cycleforest_cpu.py holds the restatement to it), so no test here walks a
search in Python: per map length, per-depth counters and stored records; every plan replayed on the oracle -- no closed trail of order
N, the closed orders below N, the goal's triples equal to the replay's.

Sets F and M carry per-map `changes`: they are applied to the worlds the forest is constructed over and to the oracle worlds the plans
are replayed on."""
import numpy as np
import pytest

from tests import cycleforest_ref, helpgraph_ref
from tests.cycleforest_ref import SET_F, SET_M, SET_T, SET_X, SETS
from tests.test_gpu_helpforest import expected_pieces

pytestmark = pytest.mark.gpu

GOLDEN = cycleforest_ref.load_golden()
KERNELS = ["cf_commit<21>", "cf_commit<3>", "cf_expand", "cf_insert<21>", "cf_insert<3>", "cf_plans<21>", "cf_plans<3>", "cf_roots", "cf_seed<21>", "cf_seed<3>"]
LLE_CAPACITY, LLE_DENSE = -20, -21


@pytest.fixture(scope="module")
def cf():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import cycleforest
    return cycleforest


def golden(s, order):
    return GOLDEN[s.name][str(order)]


def run(cf, worlds, t_max, order, only=None, **options):
    f = cf.CycleForestSolver(worlds, t_max, **options)
    try:
        res = f.run_closed_trail(order, only=only)
        if only is None:
            assert f.run_closed_trail(order) is res, "results are cached"
        return res
    finally:
        f.free()


def assert_equals_golden(cf, s, order, indices=None, **options):
    """The maps `indices` of the set (default: all, in order) as one forest under `order`, every one against its recorded entry."""
    indices = list(range(len(s.maps))) if indices is None else list(indices)
    worlds = s.worlds
    refs = [golden(s, order)[i] for i in indices]
    res = run(cf, [worlds[i] for i in indices], s.t_max, order, **options)
    print(f"set {s.name} order {order} {options}: lengths {res.length.tolist()}, records {res.n_states.tolist()}, pieces {res.pieces}, "
          f"occupancy {res.valid_items}/{res.launched_lanes}")
    for m, i in enumerate(indices):
        cycleforest_ref.assert_map_equals_golden(s, i, refs[m], res, m, order)
    E, n_joint = options.get("envs_per_map", 256), 5 ** helpgraph_ref.n_agents_of(s.maps[0])
    assert res.launched_lanes == res.pieces * len(indices) * E
    assert res.valid_items == n_joint * sum(sum(r["frontier"][:len(r["expanded"])]) for r in refs) <= res.launched_lanes
    assert res.pieces == expected_pieces(refs, n_joint, E)
    return res


# ---------------------------------------------------------------------------------------------------------------- the sets
GRID = [(name, order) for name in "TFM" for order in SETS[name].orders]


@pytest.mark.parametrize("E", [256, 64])
@pytest.mark.parametrize("name, order", GRID, ids=[f"{n}-{o}" for n, o in GRID])
def test_sets_equal_the_golden_file(cf, name, order, E):
    """Every map's counters and length are the restatement's whatever E is, every plan replays without a closed trail of the order, the
    goal's triples are the replay's, status 0.  E = 256: a workgroup per map; 64: four maps per workgroup."""
    res = assert_equals_golden(cf, SETS[name], order, envs_per_map=E)
    assert not res.status.any()


@pytest.mark.parametrize("order", SET_T.orders)
def test_workgroups_that_straddle_maps(cf, order):
    """E = 7 (125 joint actions: many pieces per state, workgroups that span 36 maps' worth of lanes and straddle their borders: a
    lane's slab is its number inside the workgroup, not inside its map)."""
    assert_equals_golden(cf, SET_T, order, envs_per_map=7)


@pytest.mark.parametrize("order", SET_T.orders)
def test_one_environment_per_map(cf, order):
    """E = 1, the whole set T: a piece serves one work item of every map; every tag is 0.  A piece per work item of the largest
    frontier: half a million pieces under order 2, 1.2 million under order 3 (paper-fully-coupled-legacy: 11 812 records of 125 joint
    actions) -- the one case of this module that takes tens of seconds, at four launches of seven lanes per piece."""
    assert_equals_golden(cf, SET_T, order, envs_per_map=1)


@pytest.mark.parametrize("E", [4096, 256])
@pytest.mark.parametrize("order", SET_X.orders)
def test_six_agents_carry_twenty_one_words(cf, order, E):
    res = assert_equals_golden(cf, SET_X, order, envs_per_map=E)
    if order == 3:
        assert all(2 in orders for orders in res.closed_orders), "a closed pair below N: a closed field, in words of its own"


# ---------------------------------------------------------------------------------------------------------------- one map, the same map, another order
@pytest.mark.parametrize("name, i, order", [("T", 1, 3), ("T", 2, 2), ("F", 0, 3), ("M", 1, 2)])
def test_a_forest_of_one_map_equals_the_single_solvers(cf, name, i, order):
    from lle_amd import cycles
    s = SETS[name]
    single = cycles.CycleSolver(s.worlds[i], s.t_max)
    try:
        plan = single.shortest_without_closed_trail(order)
        stats = single.last_stats
    finally:
        single.free()
    res = run(cf, [s.worlds[i]], s.t_max, order)
    assert (None if res.length[0] < 0 else int(res.length[0])) == stats["length"] and (plan is None) == (res.plans[0] is None)
    assert res.frontier[0] == stats["frontier"] and res.expanded[0] == stats["expanded"] and int(res.n_states[0]) == stats["n_states"]
    cycleforest_ref.assert_map_equals_golden(s, i, golden(s, order)[i], res, 0, order)
    if plan is not None:  # (which shortest plan comes back is free: the triples may differ, neither closes the order)
        assert order not in res.closed_orders[0] and order not in stats["closed_orders"]


def test_the_same_map_twice_and_another_order(cf):
    order_of_maps = [3, 0, 1, 0, 2, 1]
    for order in SET_T.orders:
        res = assert_equals_golden(cf, SET_T, order, indices=order_of_maps, envs_per_map=64)
        for a, b in ((1, 3), (2, 5)):
            assert res.length[a] == res.length[b] and res.frontier[a] == res.frontier[b] and res.expanded[a] == res.expanded[b] and res.n_states[a] == res.n_states[b]


def test_a_horizon_of_no_steps_and_a_reset_state_that_closes(cf):
    res = run(cf, SET_T.worlds[:3], 0, 3)
    assert res.length.tolist() == [-1, -1, -1] and res.frontier == [[1]] * 3 and res.expanded == [[]] * 3 and res.n_states.tolist() == [1, 1, 1]
    assert res.pieces == 0 and res.occupancy == 0.0 and res.plans == [None] * 3 and res.triples == [None] * 3
    at_reset = SET_M.names.index("mutual-at-reset")
    res = run(cf, SET_M.worlds, SET_M.t_max, 2)
    assert res.length[at_reset] == -1 and res.n_states[at_reset] == 1 and res.depth_reached[at_reset] == 0 and res.status[at_reset] == 0
    assert res.frontier[at_reset] == [1] and res.expanded[at_reset] == []


def test_routing_on_the_device(cf):
    """Order 2 through `run` is the flattened no-mutual of the inner help forest; an order above the agents is its standard answer."""
    from lle_amd import helpforest
    f = cf.CycleForestSolver(SET_M.worlds, SET_M.t_max, envs_per_map=64)
    h = helpforest.HelpForestSolver(SET_M.worlds, SET_M.t_max, envs_per_map=64)
    try:
        for asked, inner in (("no-interdependence-2", "no-mutual"), ("no-interdependence-3", "standard"), ("no-sequence-3", "no-sequence-3")):
            got, want = f.run(asked), h.run(inner)
            assert isinstance(got, cf.CycleForestResult) and got.length.tolist() == want.length.tolist() and got.n_states.tolist() == want.n_states.tolist()
            assert got.frontier == want.frontier and got.triples == [None] * len(SET_M.maps)
        assert f.h is None, "no native search was asked for"
    finally:
        f.free()
        h.free()


# ---------------------------------------------------------------------------------------------------------------- capacity and the mask
def test_capacity_isolation(cf):
    """Set T under order 3 with 256 records per map: exactly the maps whose search stores more than 256 records (by the golden file,
    not by the run) have no answer; every other map's counters and plan are what they are without a neighbour in trouble."""
    from lle_amd import solver
    refs = golden(SET_T, 3)
    over = [m for m, r in enumerate(refs) if r["states"] > 256]
    assert over and [SET_T.names[m] for m in range(len(refs)) if m not in over] == ["closes-in-one-state", "paper-interdependent-3"]
    for E in (256, 7):
        res = run(cf, SET_T.worlds, SET_T.t_max, 3, max_states_per_map=256, envs_per_map=E)
        assert [m for m in range(len(refs)) if res.status[m] != 0] == over and all(res.status[m] == LLE_CAPACITY == solver.LLE_SEARCH_CAPACITY for m in over)
        for m in range(len(refs)):
            if m in over:
                assert res.length[m] == -1 and res.plans[m] is None and res.n_states[m] == 256 and res.frontier[m] == [1] and res.expanded[m] == []
                assert res.triples[m] is None
            else:
                cycleforest_ref.assert_map_equals_golden(SET_T, m, refs[m], res, m, 3)
    with pytest.raises(solver.SolverCapacityError, match=rf"map {over[0]}\b.*max_states_per_map = 256"):
        cf.solve_many(SET_T.worlds, SET_T.t_max, mode="no-interdependence-3", max_states_per_map=256)


def test_masked_runs(cf):
    """run_closed_trail(only=...): a skipped map reports length -1, n_states 0, depth_reached 0, status 0 and costs no lane; a searched
    map is what it is in a full run."""
    for s, order in ((SET_T, 3), (SET_F, 4)):
        refs = golden(s, order)
        only = np.array([m % 3 != 1 for m in range(len(s.maps))])
        f = cf.CycleForestSolver(s.worlds, s.t_max, envs_per_map=64)
        try:
            res = f.run_closed_trail(order, only=only)
            assert f.run_closed_trail(order, only=list(only)) is not res, "a masked run is not cached"
            nothing = f.run(f"no-interdependence-{order}", only=np.zeros(len(s.maps), dtype=bool))
        finally:
            f.free()
        n_joint = 5 ** helpgraph_ref.n_agents_of(s.maps[0])
        for m in range(len(s.maps)):
            if only[m]:
                cycleforest_ref.assert_map_equals_golden(s, m, refs[m], res, m, order)
            else:
                assert (res.length[m], res.n_states[m], res.depth_reached[m], res.status[m]) == (-1, 0, 0, 0)
                assert res.plans[m] is None and res.triples[m] is None and res.closed_orders[m] is None and res.frontier[m] == [] and res.expanded[m] == []
        searched = [r for m, r in enumerate(refs) if only[m]]
        assert res.pieces == expected_pieces(searched, n_joint, 64) and res.valid_items == n_joint * sum(sum(r["frontier"][:len(r["expanded"])]) for r in searched)
        assert nothing.pieces == 0 and nothing.length.tolist() == [-1] * len(s.maps) and nothing.n_states.tolist() == [0] * len(s.maps)


# ---------------------------------------------------------------------------------------------------------------- characterisations
@pytest.mark.parametrize("name, t_max", [("T", 10), ("F", 6)])
def test_characterize_many_equals_a_characterizer_per_world(cf, name, t_max):
    """is_interdependent(3) and (4) are what one CycleCharacterizer per world answers, and what the reference states for the layout at
    this horizon where it states anything; only the open maps are searched."""
    from lle_amd import cycles
    s = SETS[name]
    worlds = s.worlds
    stated_somewhere = 0
    with cf.characterize_many(worlds, t_max, envs_per_map=64) as many:
        assert isinstance(many, cf.ManyCycleCharacterization)
        answers = {n: many.is_interdependent(n) for n in (2, 3, 4)}
        assert all(a.dtype == bool and a.shape == (len(worlds),) for a in answers.values())
        for mode, res in many.runs:
            if mode.startswith("no-interdependence-") and mode[-1] in "34":  # only the maps whose answer was open were searched
                assert (res.n_states > 0).sum() <= int(many.cooperative.sum())
        for i, world in enumerate(worlds):
            c = cycles.CycleCharacterizer(world, t_max)
            try:
                for n in (2, 3, 4):
                    assert bool(answers[n][i]) == c.is_interdependent(n), (s.names[i], n)
                    assert many.entry(i).is_interdependent(n) == bool(answers[n][i])
            finally:
                c._solver.free()
            if s.changes[i] is None:
                for n, value in cycleforest_ref.stated_interdependent(s.base[i], t_max).items():
                    if n in answers:
                        stated_somewhere += 1
                        assert bool(answers[n][i]) is value, (s.names[i], n)
    if name == "T":
        assert stated_somewhere >= 3, "paper-interdependent-3 and both fully coupled layouts are stated at t_max 10"
        assert answers[3][s.names.index("paper-interdependent-3")] and not answers[4].any()


def test_satisfied_by_many_over_mixed_shapes(cf):
    from lle_amd import Constraint, Cooperative, CycleCharacterizer, Interdependent, Sequential
    worlds = [w for pair in zip(SET_T.worlds[:3], SET_M.worlds[:3], SET_F.worlds) for w in pair]  # three shapes, interleaved
    for predicate in (Interdependent(3), Cooperative() & ~Interdependent(3), Interdependent(2) | Interdependent(4) | Sequential(3)):
        c = Constraint(10 if predicate == Interdependent(3) else 6, predicate)
        got = c.satisfied_by_many(worlds, characterizer=CycleCharacterizer, envs_per_map=64)
        want = [c.is_satisfied_by(w, characterizer=CycleCharacterizer) for w in worlds]
        assert got.dtype == bool and got.tolist() == want, predicate
    assert Constraint(10, Interdependent(3)).satisfied_by_many(worlds, characterizer=CycleCharacterizer).any()
    # a key of the single solver keeps the loop of one CycleCharacterizer per world
    c = Constraint(6, Interdependent(3))
    assert c.satisfied_by_many(worlds[:3], characterizer=CycleCharacterizer, chunk=4096).tolist() == [c.is_satisfied_by(w, characterizer=CycleCharacterizer) for w in worlds[:3]]


@pytest.mark.parametrize("batch", [4, 16])
def test_generate_n_over_candidates_that_reach_the_closed_trail_search(cf, batch, monkeypatch):
    """Random candidates are settled by the cheap no (the test below); here the candidates are the layouts of set T in turn, fed through
    a stubbed `mapgen.generate`, so that the batches hold maps whose answer is open and `generate_n` runs the native search."""
    from lle_amd import Constraint, CycleCharacterizer, Interdependent, World, generate_n, mapgen
    monkeypatch.setattr(mapgen, "generate", lambda *args, seed=0, **kwargs: SET_T.maps[seed % len(SET_T.maps)])
    native = []
    run_native = cf.CycleForestSolver._native
    monkeypatch.setattr(cf.CycleForestSolver, "_native", lambda self, order, collect_gems, mask: native.append(order) or run_native(self, order, collect_gems, mask))
    shape = dict(height=6, width=7, n_agents=3, n_lasers=3, seed=0)
    constraint = Constraint(10, Interdependent(3))
    worlds = list(generate_n(4, constraint, batch=batch, max_attempts=21, characterizer=CycleCharacterizer, envs_per_map=64, **shape))
    assert native and set(native) == {3}, "some batch held a map whose answer was open"
    other = list(generate_n(4, constraint, batch=20 - batch, max_attempts=21, characterizer=CycleCharacterizer, **shape))
    assert [w.world_string for w in worlds] == [w.world_string for w in other], "the worlds do not depend on the batch"
    # (paper-interdependent-3 and both fully coupled layouts are stated at t_max 10: at least three of every seven candidates pass)
    assert len(worlds) == 4 and all(isinstance(w, World) for w in worlds)
    for w in worlds:
        c = CycleCharacterizer(w, 10)
        try:
            assert c.is_interdependent(3)
        finally:
            c._solver.free()


@pytest.mark.parametrize("batch", [4, 16])
def test_generate_n(cf, batch):
    from lle_amd import Constraint, CycleCharacterizer, Interdependent, World, generate_n
    shape = dict(height=4, width=5, n_agents=3, n_lasers=3, n_gems=0, n_exits=3, wall_fraction=0.05, n_voids=0, seed=0)
    constraint = Constraint(8, ~Interdependent(3))
    worlds = list(generate_n(3, constraint, batch=batch, max_attempts=32, characterizer=CycleCharacterizer, envs_per_map=64, **shape))
    other = list(generate_n(3, constraint, batch=20 - batch, max_attempts=32, characterizer=CycleCharacterizer, **shape))
    assert len(worlds) == 3 and all(isinstance(w, World) for w in worlds)
    assert [w.world_string for w in worlds] == [w.world_string for w in other], "the worlds do not depend on the batch"
    for w in worlds:
        c = CycleCharacterizer(w, 8)
        try:
            assert not c.is_interdependent(3)
        finally:
            c._solver.free()


def test_every_kernel_was_launched(cf):
    """(last in the module: the tests above launch both agent classes.)"""
    assert sorted(cf.compiled_kernels()) == KERNELS
    assert set(cf.launched_kernels()) == set(cf.compiled_kernels())
