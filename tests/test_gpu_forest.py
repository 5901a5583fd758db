"""The forest search on the MI355X (liblle_forest.so, lle_amd.forest, lle_amd.generator) against the restatement of the search over the
oracle (tests/search_ref.py), per map: length, per-depth counters, stored states, and every plan replayed on the oracle.  The fixed
input sets are those of tests/forest_ref.py."""
import numpy as np
import pytest

from tests import forest_ref, search_ref
from tests.forest_ref import MODES, SET_A, SET_B, SET_C, SETS

pytestmark = pytest.mark.gpu

KERNELS = ["forest_commit", "forest_expand", "forest_insert<false>", "forest_insert<true>", "forest_plans", "forest_roots", "forest_seed"]


@pytest.fixture(scope="module")
def forest_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import forest
    return forest


def run(forest_mod, maps, t_max, mode="standard", collect_gems=False, **options):
    f = forest_mod.ForestSolver(maps, t_max, **options)
    res = f.run(mode, collect_gems)
    assert f.run(mode, collect_gems) is res, "results are cached"
    f.free()
    return res


def assert_equals_oracle(forest_mod, maps, t_max, mode="standard", collect_gems=False, **options):
    refs = forest_ref.oracle(maps, t_max, mode, collect_gems)
    res = run(forest_mod, maps, t_max, mode, collect_gems, **options)
    print(f"{mode} collect_gems={collect_gems} {options}: lengths {res.length.tolist()}, states {res.n_states.tolist()}, pieces {res.pieces}, "
          f"occupancy {res.valid_items}/{res.launched_lanes}")
    for m, (text, ref) in enumerate(zip(maps, refs)):
        forest_ref.assert_map_equals_oracle(text, ref, res, m, mode, collect_gems)
    E = options.get("envs_per_map", 256)
    assert res.launched_lanes == res.pieces * len(maps) * E
    assert res.valid_items == 5 ** _agents(maps[0]) * sum(sum(r.frontier[:len(r.expanded)]) for r in refs if r.expanded) and 0 < res.valid_items <= res.launched_lanes
    # pieces: per level the most any map needs, over the levels some map still walks
    depths = max(len(r.expanded) for r in refs)
    want = sum(max(-(-r.frontier[d] * 5 ** _agents(maps[0]) // E) for r in refs if d < len(r.expanded)) for d in range(depths))
    assert res.pieces == want
    return res


def _agents(text):
    from lle_amd import Map
    return Map(text).n_agents


# ---------------------------------------------------------------------------------------------------------------- the sets
@pytest.mark.parametrize("E", [256, 64, 7])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(SETS))
def test_sets_equal_the_oracle(forest_mod, name, mode, E):
    """Every map's counters and length are the oracle's whatever E is (so they do not depend on E), every plan replays, status 0.
    E = 256: a workgroup per map; 64: four maps per workgroup; 7: workgroups that straddle maps, many pieces per level."""
    s = SETS[name]
    res = assert_equals_oracle(forest_mod, s.maps, s.t_max, mode, envs_per_map=E)
    assert not res.status.any()
    if name == "A" and mode == "standard":
        assert [None if v < 0 else int(v) for v in res.length] == forest_ref.A_STANDARD_LENGTHS
        assert res.depth_reached[8] == 10 and res.depth_reached[13] == 9 and res.frontier[8][-1] == 0 == res.frontier[13][-1]  # ran empty
    if name == "A" and mode == "no-cooperation":
        assert [s_ for s_ in range(16) if res.length[s_] < 0 and forest_ref.A_STANDARD_LENGTHS[s_] is not None] == forest_ref.A_COOPERATIVE_SEEDS
    if name == "B" and mode == "standard":
        for seed in forest_ref.B_HORIZON_SEEDS:  # stopped at the horizon with a live frontier
            assert res.length[seed] < 0 and res.depth_reached[seed] == SET_B.t_max and res.frontier[seed][-1] > 0


@pytest.mark.parametrize("mode", MODES)
def test_one_environment_per_map(forest_mod, mode):
    """E = 1: a piece serves one work item of every map; four launches per item of the widest frontier."""
    assert_equals_oracle(forest_mod, SET_A.maps[:4], SET_A.t_max, mode, envs_per_map=1)


def test_collect_gems(forest_mod):
    res = assert_equals_oracle(forest_mod, SET_A.maps, SET_A.t_max, collect_gems=True)
    assert [None if v < 0 else int(v) for v in res.length[:8]] == forest_ref.A_GEM_LENGTHS_FIRST_8
    assert_equals_oracle(forest_mod, SET_A.maps[:8], SET_A.t_max, "no-cooperation", collect_gems=True, envs_per_map=64)


def test_a_forest_of_one_map_equals_the_solver(forest_mod):
    from lle_amd import solver
    for seed in (7, 8, 0):  # cooperative, runs empty, plain
        text = SET_A.maps[seed]
        for mode in MODES:
            s = solver.Solver(text, SET_A.t_max)
            plan = s.find_shortest(mode)
            stats = s.last_stats
            s.free()
            res = run(forest_mod, [text], SET_A.t_max, mode)
            assert (None if res.length[0] < 0 else int(res.length[0])) == stats["length"] and (plan is None) == (res.plans[0] is None)
            assert res.frontier[0] == stats["frontier"] and res.expanded[0] == stats["expanded"] and int(res.n_states[0]) == stats["n_states"]
            if plan is not None:
                assert len(plan) == len(res.plans[0])
                search_ref.check_plan(text, [[a.value for a in row] for row in res.plans[0]], mode, length=len(plan))


def test_the_same_map_twice(forest_mod):
    for mode in MODES:
        res = assert_equals_oracle(forest_mod, [SET_A.maps[3], SET_A.maps[7], SET_A.maps[3]], SET_A.t_max, mode, envs_per_map=64)
        assert res.length[0] == res.length[2] and res.frontier[0] == res.frontier[2] and res.expanded[0] == res.expanded[2] and res.n_states[0] == res.n_states[2]


def test_a_horizon_of_no_steps_and_a_start_on_the_exit(forest_mod):
    res = run(forest_mod, SET_A.maps[:3], 0)
    assert res.length.tolist() == [-1, -1, -1] and res.frontier == [[1]] * 3 and res.expanded == [[]] * 3 and res.n_states.tolist() == [1, 1, 1]
    assert res.pieces == 0 and res.occupancy == 0.0 and res.plans == [None] * 3
    res = run(forest_mod, ["S0 X", "S0 X"], 3)
    assert res.length.tolist() == [1, 1] and [len(p) for p in res.plans] == [1, 1]


# ---------------------------------------------------------------------------------------------------------------- capacity
def test_capacity_isolation(forest_mod):
    """max_states_per_map = 128: exactly the maps whose search stores more than 128 states have no answer; every other map's counters and
    plan are what they are without a neighbour in trouble."""
    from lle_amd import solver
    refs = forest_ref.oracle(SET_A.maps, SET_A.t_max)
    over = [s for s in range(16) if refs[s].n_states > 128]
    assert over == forest_ref.A_OVER_128_STATES
    for E in (256, 7):
        res = run(forest_mod, SET_A.maps, SET_A.t_max, max_states_per_map=128, envs_per_map=E)
        assert [s for s in range(16) if res.status[s] != 0] == over and all(res.status[s] == solver.LLE_SEARCH_CAPACITY for s in over)
        for s in range(16):
            if s in over:
                assert res.length[s] == -1 and res.plans[s] is None and res.n_states[s] == 128 and res.frontier[s] == [1] and res.expanded[s] == []
            else:
                forest_ref.assert_map_equals_oracle(SET_A.maps[s], refs[s], res, s)
    with pytest.raises(solver.SolverCapacityError, match=r"map 2\b.*max_states_per_map = 128"):
        forest_mod.solve_many(SET_A.maps, SET_A.t_max, max_states_per_map=128)
    with pytest.raises(solver.SolverCapacityError, match=r"map 2\b"):
        forest_mod.characterize_many(SET_A.maps, SET_A.t_max, max_states_per_map=128)
    exact = run(forest_mod, [SET_A.maps[15]], SET_A.t_max, max_states_per_map=130)  # exactly full is no overflow
    assert exact.status[0] == 0 and exact.n_states[0] == 130 == refs[15].n_states and exact.length[0] == refs[15].length


def test_a_batch_stepped_beside_a_forest_is_undisturbed(forest_mod):
    """tests/test_gpu_solver.py::test_capacity_and_neighbours with a forest for a neighbour."""
    import torch

    from lle_amd import BatchedWorld
    text = SET_A.maps[7]
    bw = BatchedWorld(text, 64, device="cuda:0")
    bw.step(sample=True, seed=5, t=0)
    small = forest_mod.ForestSolver(SET_A.maps, SET_A.t_max, max_states_per_map=128, envs_per_map=64)
    second = forest_mod.ForestSolver(SET_A.maps[:8], SET_A.t_max, envs_per_map=100)  # a second handle beside the first
    first = small.run()
    other = second.run("no-cooperation")
    bw.step(sample=True, seed=5, t=1)
    after = bw.host_buffers()
    again = second.run("standard")
    twin = BatchedWorld(text, 64, device="cuda:0")
    twin.step(sample=True, seed=5, t=0)
    twin.step(sample=True, seed=5, t=1)
    want = twin.host_buffers()
    for key in ("pos", "bits", "gems", "beams", "avail"):
        assert torch.equal(torch.as_tensor(after[key]), torch.as_tensor(want[key])), key
    refs = forest_ref.oracle(SET_A.maps, SET_A.t_max)
    alone = forest_ref.oracle(SET_A.maps, SET_A.t_max, "no-cooperation")
    assert [s for s in range(16) if first.status[s] != 0] == forest_ref.A_OVER_128_STATES
    for m in range(8):
        forest_ref.assert_map_equals_oracle(SET_A.maps[m], alone[m], other, m, "no-cooperation")
        forest_ref.assert_map_equals_oracle(SET_A.maps[m], refs[m], again, m)
    small.free()
    second.free()


# ---------------------------------------------------------------------------------------------------------------- many worlds of any shape
MIXED = [("A", 0), ("B", 3), ("C", 4), ("A", 1), ("B", 5), ("A", 8), ("C", 1), ("B", 7), ("A", 10), ("C", 0)]


def test_solve_many_and_characterize_many_over_mixed_shapes(forest_mod):
    """One t_max for the whole list, three shapes in it: grouped by shape, answered in input order, equal to one Solver /
    WorldCharacterizer per map (plans: equally long and valid -- which shortest plan comes back is free)."""
    from lle_amd import World, WorldCharacterizer, solver
    texts = [SETS[name].maps[seed] for name, seed in MIXED]
    t_max = 8
    for mode in MODES:
        many = forest_mod.solve_many([World(t) for t in texts], t_max, mode=mode, envs_per_map=64)
        assert isinstance(many, list) and len(many) == len(texts)
        for text, got in zip(texts, many):
            s = solver.Solver(text, t_max)
            want = s.find_shortest(mode)
            s.free()
            assert (got is None) == (want is None) and (got is None or len(got) == len(want)), (text, got, want)
            assert (None if got is None else len(got)) == search_ref.search(text, t_max, mode).length
            if got is not None:
                assert all(isinstance(row, tuple) and len(row) == len(want[0]) for row in got)
                search_ref.check_plan(text, [[a.value for a in row] for row in got], mode, length=len(want))
    many = forest_mod.characterize_many(texts, t_max)
    assert many.solvable.dtype == bool and many.cooperative.dtype == bool and many.independent.dtype == bool and len(many) == len(texts)
    for i, text in enumerate(texts):
        c = WorldCharacterizer(World(text), t_max)
        assert (bool(many.solvable[i]), bool(many.cooperative[i]), bool(many.independent[i])) == (c.is_solvable(), c.is_cooperative(), c.is_independent())
        for got, want, length, mode in ((many.shortest_paths[i], c.shortest_path, many.shortest_length[i], "standard"),
                                        (many.shortest_independent_paths[i], c.shortest_independent_path, many.shortest_independent_length[i], "no-cooperation")):
            assert (got is None) == (want is None) and length == (-1 if want is None else len(want))
            if got is not None:
                search_ref.check_plan(text, [[a.value for a in row] for row in got], mode, length=len(want))
        c._solver.free()
    assert many.cooperative.any() and many.independent.any() and not many.solvable.all()


# ---------------------------------------------------------------------------------------------------------------- filters and the generator
def test_constraints_over_set_a(forest_mod):
    from lle_amd import Constraint, Cooperative, Independent, Solvable, World
    worlds = [World(t) for t in SET_A.maps]
    solvable = [s for s in range(16) if forest_ref.A_STANDARD_LENGTHS[s] is not None]
    got = Constraint(10, Cooperative()).satisfied_by_many(worlds)
    assert got.dtype == bool and got.shape == (16,) and np.flatnonzero(got).tolist() == forest_ref.A_COOPERATIVE_SEEDS
    others = [s for s in solvable if s not in forest_ref.A_COOPERATIVE_SEEDS]
    assert np.flatnonzero(Constraint(10, ~Cooperative() & Solvable()).satisfied_by_many(SET_A.maps)).tolist() == others
    assert np.flatnonzero(Constraint(10, Independent()).satisfied_by_many(worlds, envs_per_map=64)).tolist() == others
    assert np.flatnonzero(Constraint(10).satisfied_by_many(worlds)).tolist() == solvable
    longer = [s for s in solvable if forest_ref.A_STANDARD_LENGTHS[s] >= 6]
    assert np.flatnonzero(Constraint(10, min_solution_length=6).satisfied_by_many(worlds)).tolist() == longer == [1, 3, 5, 7, 10]
    assert np.flatnonzero(Constraint(10, Cooperative(), min_solution_length=7).satisfied_by_many(worlds)).tolist() == [7]
    for s in (1, 4):  # ... and the one-world way gives the same
        assert Constraint(10, Cooperative()).is_satisfied_by(worlds[s]) is bool(got[s])


@pytest.mark.parametrize("batch", [4, 16])
def test_generate_n(forest_mod, batch):
    from lle_amd import Constraint, Cooperative, World, generate_n
    shape = dict(height=4, width=5, n_agents=2, n_lasers=1, n_gems=1, n_exits=2, wall_fraction=0.12, n_voids=1, seed=0)
    worlds = list(generate_n(3, Constraint(10, Cooperative()), batch=batch, **shape))
    assert all(isinstance(w, World) for w in worlds)
    assert [w.world_string for w in worlds] == [World(SET_A.maps[s]).world_string for s in forest_ref.A_COOPERATIVE_SEEDS]
    assert len(list(generate_n(3, Constraint(10, Cooperative()), batch=batch, max_attempts=8, **shape))) == 2  # seeds 1 and 7 of the first eight
    assert len(list(generate_n(1, Constraint(10, Cooperative()), batch=batch, **shape))) == 1


def test_every_kernel_was_launched(forest_mod):
    """(last in the module: the tests above launch both insert kernels.)"""
    assert sorted(forest_mod.compiled_kernels()) == KERNELS
    assert set(forest_mod.launched_kernels()) == set(forest_mod.compiled_kernels())
