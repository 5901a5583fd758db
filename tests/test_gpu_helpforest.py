"""The help forest on the MI355X (liblle_helpforest.so, lle_amd.helpforest, lle_amd.generator) against the restatements of the two
searches over the oracle (tests/helpgraph_ref.py, tests/trails_ref.py), whose per-map figures for every (set, mode) of
tests/helpforest_ref.py are recorded in tests/golden/kat_helpforest.json (tests/test_helpforest_cpu.py holds the restatements to it), so
no test here walks a search in Python: per map length, per-depth counters and stored records; every plan replayed on the oracle under
its mode; the goal's help edges or trail equal to the replay's.

Set X (six agents: 15 625 joint actions per state, frontiers of several hundred records) takes tens of thousands of pieces at
envs_per_map = 256 and 64 -- a few seconds -- and runs at 4096 as well, where a piece holds candidates of several records.

Sets L and C (long trails, one layout under four edge rules) carry per-map `changes`: `assert_equals_golden` applies them to the worlds
the forest is constructed over and to the oracle worlds the plans are replayed on.  What else is asked of them is in
tests/test_gpu_helpforest_edges.py."""
import numpy as np
import pytest

from tests import helpforest_ref, helpgraph_ref
from tests.helpforest_ref import SET_G, SET_P, SET_R, SET_S, SET_X, SETS, golden_key, mode_text

pytestmark = pytest.mark.gpu

GOLDEN = helpforest_ref.load_golden()
KERNELS = ["hf_commit<help>", "hf_commit<trail>", "hf_expand", "hf_insert<help>", "hf_insert<trail>", "hf_plans", "hf_roots", "hf_seed<help>", "hf_seed<trail>"]
LLE_CAPACITY, LLE_DENSE = -20, -21


@pytest.fixture(scope="module")
def hf():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import helpforest
    return helpforest


def run(hf, maps, t_max, mode, param=2, collect_gems=False, only=None, **options):
    f = hf.HelpForestSolver(maps, t_max, **options)
    try:
        res = f.run(mode_text(mode, param), collect_gems, only=only)
        if only is None:
            assert f.run(mode_text(mode, param), collect_gems) is res, "results are cached"
        return res
    finally:
        f.free()


def expected_pieces(refs, n_joint, E):
    """Per level the most any map needs, over the levels some map still walks (the formula of tests/test_gpu_forest.py)."""
    depths = max([len(r["expanded"]) for r in refs] + [0])
    return sum(max(-(-r["frontier"][d] * n_joint // E) for r in refs if d < len(r["expanded"])) for d in range(depths))


def assert_equals_golden(hf, maps, refs, t_max, mode, param=2, collect_gems=False, changes=None, **options):
    """`maps`: map texts; `changes`: per map the changes of tests/helpgraph_ref.py applied to its world before the forest is constructed
    (and to the oracle world every plan is replayed on), None: no map is changed."""
    changes = [None] * len(maps) if changes is None else list(changes)
    assert len(changes) == len(maps) == len(refs)
    res = run(hf, [helpforest_ref.world_of(text, c) for text, c in zip(maps, changes)], t_max, mode, param, collect_gems, **options)
    print(f"{mode}-{param} collect_gems={collect_gems} {options}: lengths {res.length.tolist()}, records {res.n_states.tolist()}, pieces {res.pieces}, "
          f"occupancy {res.valid_items}/{res.launched_lanes}")
    for m, (text, ref) in enumerate(zip(maps, refs)):
        helpforest_ref.assert_map_equals_golden(text, ref, res, m, mode, param, collect_gems, changes=changes[m])
    E, n_joint = options.get("envs_per_map", 256), 5 ** helpgraph_ref.n_agents_of(maps[0])
    assert res.launched_lanes == res.pieces * len(maps) * E
    assert res.valid_items == n_joint * sum(sum(r["frontier"][:len(r["expanded"])]) for r in refs) <= res.launched_lanes
    assert res.pieces == expected_pieces(refs, n_joint, E)
    return res


def golden(s, mode, param):
    return GOLDEN[s.name][golden_key(mode, param)]


# ---------------------------------------------------------------------------------------------------------------- the sets
GRID = [(name, mode, param) for name in sorted(SETS) for mode, param in SETS[name].modes]


@pytest.mark.parametrize("E", [256, 64])
@pytest.mark.parametrize("name, mode, param", GRID, ids=[f"{n}-{mode_text(m, p)}" for n, m, p in GRID])
def test_sets_equal_the_golden_file(hf, name, mode, param, E):
    """Every map's counters and length are the restatement's whatever E is, every plan replays under its mode, the goal's extra words
    are the replay's, status 0.  E = 256: a workgroup per map; 64: four maps per workgroup."""
    s = SETS[name]
    res = assert_equals_golden(hf, s.maps, golden(s, mode, param), s.t_max, mode, param, s.collect_gems, changes=s.changes, envs_per_map=E)
    assert not res.status.any()


@pytest.mark.parametrize("mode, param", SET_P.modes, ids=[mode_text(m, p) for m, p in SET_P.modes])
def test_workgroups_that_straddle_maps(hf, mode, param):
    """E = 7 (25 joint actions: many pieces per state, workgroups that span 36 maps' worth of lanes and straddle their borders)."""
    assert_equals_golden(hf, SET_P.maps, golden(SET_P, mode, param), SET_P.t_max, mode, param, envs_per_map=7)


@pytest.mark.parametrize("mode, param", SET_P.modes, ids=[mode_text(m, p) for m, p in SET_P.modes])
def test_one_environment_per_map(hf, mode, param):
    """E = 1: a piece serves one work item of every map; every tag is 0."""
    assert_equals_golden(hf, SET_P.maps[:4], golden(SET_P, mode, param)[:4], SET_P.t_max, mode, param, envs_per_map=1)


@pytest.mark.parametrize("mode, param", SET_X.modes, ids=[mode_text(m, p) for m, p in SET_X.modes])
def test_six_agents_reach_the_second_help_word(hf, mode, param):
    res = assert_equals_golden(hf, SET_X.maps, golden(SET_X, mode, param), SET_X.t_max, mode, param, envs_per_map=4096)
    if mode == "standard":
        assert any(h >= 4 for edges in res.help_edges if edges for h, _b in edges), "an edge whose helper's row lies in the second help word"


def test_collect_gems(hf):
    """Set G with and without the gem in the identity: one handle, both searches."""
    f = hf.HelpForestSolver(SET_G.maps, SET_G.t_max, envs_per_map=64)
    try:
        for mode, param in SET_G.modes:
            with_gems, without = f.run(mode_text(mode, param), True), f.run(mode_text(mode, param), False)
            for m, text in enumerate(SET_G.maps):
                helpforest_ref.assert_map_equals_golden(text, golden(SET_G, mode, param)[m], with_gems, m, mode, param, True)
                if without.plans[m] is not None:
                    helpforest_ref.check_plan(text, [[a.value for a in row] for row in without.plans[m]], mode, param, False)
                    assert with_gems.plans[m] is None or len(with_gems.plans[m]) >= len(without.plans[m])
        assert any(r["length"] is not None for r in golden(SET_G, "standard", 2))
    finally:
        f.free()


# ---------------------------------------------------------------------------------------------------------------- one map, the same map, another order
@pytest.mark.parametrize("name, m", [("P", 1), ("S", 1)])
def test_a_forest_of_one_map_equals_the_single_solvers(hf, name, m):
    from lle_amd import trails
    s = SETS[name]
    for mode, param in s.modes[:3] if name == "S" else s.modes[1:]:
        single = trails.TrailSolver(s.maps[m], s.t_max)
        try:
            plan = single.find_shortest(mode_text(mode, param))
            stats = single.last_stats
        finally:
            single.free()
        res = run(hf, [s.maps[m]], s.t_max, mode, param)
        assert (None if res.length[0] < 0 else int(res.length[0])) == stats["length"] and (plan is None) == (res.plans[0] is None)
        assert res.frontier[0] == stats["frontier"] and res.expanded[0] == stats["expanded"] and int(res.n_states[0]) == stats["n_states"]
        helpforest_ref.assert_map_equals_golden(s.maps[m], golden(s, mode, param)[m], res, 0, mode, param)
        if plan is not None and mode == "no-sequence":  # (which shortest plan comes back is free: the two trails may differ, both stay below N)
            assert max(res.trail[0]) < param and stats["longest_trail"] < param
        if plan is not None and mode != "no-sequence":
            assert helpgraph_ref.accepts(res.help_edges[0], mode) and helpgraph_ref.accepts(stats["help_edges"], mode)


def test_the_same_map_twice_and_another_order(hf):
    for s, mode, param in ((SET_S, "no-asymmetric", 2), (SET_S, "no-divergence", 2), (SET_P, "no-sequence", 3), (SET_P, "no-mutual", 2)):
        order = [3, 0, 1, 0, 7, 1]
        refs = golden(s, mode, param)
        res = assert_equals_golden(hf, [s.maps[i] for i in order], [refs[i] for i in order], s.t_max, mode, param, envs_per_map=64)
        for a, b in ((1, 3), (2, 5)):
            assert res.length[a] == res.length[b] and res.frontier[a] == res.frontier[b] and res.expanded[a] == res.expanded[b] and res.n_states[a] == res.n_states[b]


def test_a_horizon_of_no_steps_and_a_reset_state_the_mode_rejects(hf):
    res = run(hf, SET_P.maps[:3], 0, "no-mutual")
    assert res.length.tolist() == [-1, -1, -1] and res.frontier == [[1]] * 3 and res.expanded == [[]] * 3 and res.n_states.tolist() == [1, 1, 1]
    assert res.pieces == 0 and res.occupancy == 0.0 and res.plans == [None] * 3
    at_reset = SET_R.names.index("chain-at-reset")
    res = run(hf, SET_R.maps, SET_R.t_max, "no-sequence", 2)
    assert res.length[at_reset] == -1 and res.n_states[at_reset] == 1 and res.depth_reached[at_reset] == 0 and res.status[at_reset] == 0
    assert res.frontier[at_reset] == [1] and res.expanded[at_reset] == []


# ---------------------------------------------------------------------------------------------------------------- capacity and the mask
def test_capacity_isolation(hf):
    """Set S under no-asymmetric with 256 records per map: exactly the maps whose search stores more than 256 records (by the golden
    file, not by the run) have no answer; every other map's counters and plan are what they are without a neighbour in trouble."""
    from lle_amd import solver
    refs = golden(SET_S, "no-asymmetric", 2)
    over = [m for m, r in enumerate(refs) if r["states"] > 256]
    assert over and len(over) < len(refs)
    for E in (256, 7):
        res = run(hf, SET_S.maps, SET_S.t_max, "no-asymmetric", max_states_per_map=256, envs_per_map=E)
        assert [m for m in range(len(refs)) if res.status[m] != 0] == over and all(res.status[m] == LLE_CAPACITY == solver.LLE_SEARCH_CAPACITY for m in over)
        for m, text in enumerate(SET_S.maps):
            if m in over:
                assert res.length[m] == -1 and res.plans[m] is None and res.n_states[m] == 256 and res.frontier[m] == [1] and res.expanded[m] == []
                assert res.help_edges[m] is None
            else:
                helpforest_ref.assert_map_equals_golden(text, refs[m], res, m, "no-asymmetric", 2)
    with pytest.raises(solver.SolverCapacityError, match=rf"map {over[0]}\b.*max_states_per_map = 256"):
        hf.solve_many(SET_S.maps, SET_S.t_max, mode="no-asymmetric", max_states_per_map=256)
    with hf.characterize_many(SET_S.maps, SET_S.t_max, max_states_per_map=256) as many:
        with pytest.raises(solver.SolverCapacityError, match=r"map \d+\b"):
            many.is_asymmetric()


def test_masked_runs(hf):
    """run(only=...): a skipped map reports length -1, n_states 0, depth_reached 0, status 0 and costs no lane; a searched map is what
    it is in a full run."""
    for s, mode, param in ((SET_P, "no-sequence", 3), (SET_S, "no-divergence", 2)):
        refs = golden(s, mode, param)
        only = np.array([m % 3 != 1 for m in range(len(s.maps))])
        f = hf.HelpForestSolver(s.maps, s.t_max, envs_per_map=64)
        try:
            res = f.run(mode_text(mode, param), only=only)
            assert f.run(mode_text(mode, param), only=list(only)) is not res, "a masked run is not cached"
            full = f.run(mode_text(mode, param))
            nothing = f.run(mode_text(mode, param), only=np.zeros(len(s.maps), dtype=bool))
            independent = f.run("no-cooperation", only=only)
        finally:
            f.free()
        n_joint = 5 ** helpgraph_ref.n_agents_of(s.maps[0])
        for m, text in enumerate(s.maps):
            if only[m]:
                helpforest_ref.assert_map_equals_golden(text, refs[m], res, m, mode, param)
            else:
                assert (res.length[m], res.n_states[m], res.depth_reached[m], res.status[m]) == (-1, 0, 0, 0)
                assert res.plans[m] is None and res.help_edges[m] is None and res.trail[m] is None and res.frontier[m] == [] and res.expanded[m] == []
                assert (independent.length[m], independent.n_states[m], independent.plans[m]) == (-1, 0, None)
            helpforest_ref.assert_map_equals_golden(text, refs[m], full, m, mode, param)
        searched = [r for m, r in enumerate(refs) if only[m]]
        assert res.pieces == expected_pieces(searched, n_joint, 64) and res.valid_items == n_joint * sum(sum(r["frontier"][:len(r["expanded"])]) for r in searched)
        assert nothing.pieces == 0 and nothing.length.tolist() == [-1] * len(s.maps) and nothing.n_states.tolist() == [0] * len(s.maps)


# ---------------------------------------------------------------------------------------------------------------- characterisations
QUESTIONS = [("is_solvable", "solvable", ()), ("is_cooperative", "cooperative", ()), ("is_independent", "independent", ()), ("is_asymmetric", None, ()),
             ("is_fully_coupled", None, ()), ("is_mutual", None, ()), ("is_interdependent", None, (2,)), ("is_convergent", None, (2,)), ("is_convergent", None, (3,)),
             ("is_divergent", None, (2,)), ("is_divergent", None, (3,)), ("is_sequential", None, (2,)), ("is_sequential", None, (3,))]


@pytest.mark.parametrize("name", ["S", "P", "R"])
def test_characterize_many_equals_a_characterizer_per_world(hf, name):
    from lle_amd import World, trails
    s = SETS[name]
    with hf.characterize_many(s.maps, s.t_max, envs_per_map=64) as many:
        answers = {(q, args): (getattr(many, attr) if attr else getattr(many, q)(*args)) for q, attr, args in QUESTIONS}
        assert all(a.dtype == bool and a.shape == (len(s.maps),) for a in answers.values())
        for i, text in enumerate(s.maps):
            c = trails.TrailCharacterizer(World(text), s.t_max)
            try:
                for q, _attr, args in QUESTIONS:
                    assert bool(answers[(q, args)][i]) == getattr(c, q)(*args), (s.names[i], q, args)
                    assert getattr(many.entry(i), q)(*args) == bool(answers[(q, args)][i])
            finally:
                c._solver.free()
            want = helpforest_ref.stated(s.names[i], s.t_max)  # the reference's own values, where it states any at this horizon
            for key, q in (("asymmetric", "is_asymmetric"), ("fully_coupled", "is_fully_coupled")):
                if key in want:
                    assert bool(answers[(q, ())][i]) is want[key], (s.names[i], key)
            for key, q in (("convergent", "is_convergent"), ("divergent", "is_divergent"), ("interdependent", "is_interdependent"), ("sequential", "is_sequential")):
                for k, value in want.get(key, {}).items():
                    if (q, (int(k),)) in answers:
                        assert bool(answers[(q, (int(k),))][i]) is value, (s.names[i], key, k)
    stated_somewhere = [n for n in s.names if helpforest_ref.stated(n, s.t_max)]
    assert stated_somewhere, "every one of these sets holds a layout the reference states values for"


def test_satisfied_by_many_over_mixed_shapes(hf):
    from lle_amd import Asymmetric, Constraint, Cooperative, Divergent, Interdependent, Sequential, TrailCharacterizer, World
    texts = [t for pair in zip(SET_S.maps[:4], SET_P.maps[:4], SET_R.maps[:4]) for t in pair]  # three shapes, interleaved
    worlds = [World(t) for t in texts]
    t_max = 6
    for predicate in (Asymmetric(), Cooperative() & ~Sequential(3), Divergent(2) | Interdependent(2)):
        c = Constraint(t_max, predicate)
        got = c.satisfied_by_many(worlds, characterizer=TrailCharacterizer, envs_per_map=64)
        want = [c.is_satisfied_by(w, characterizer=TrailCharacterizer) for w in worlds]
        assert got.dtype == bool and got.tolist() == want, predicate
    c = Constraint(t_max, Asymmetric() & ~Sequential(3), min_solution_length=2)
    assert c.satisfied_by_many(texts, characterizer=TrailCharacterizer).tolist() == [c.is_satisfied_by(t, characterizer=TrailCharacterizer) for t in texts]
    assert Constraint(t_max, Asymmetric()).satisfied_by_many(worlds, characterizer=TrailCharacterizer).any()
    with pytest.raises(NotImplementedError):  # today's path keeps raising
        Constraint(t_max, Asymmetric()).satisfied_by_many(worlds)


@pytest.mark.parametrize("batch", [4, 16])
def test_generate_n(hf, batch):
    from lle_amd import Asymmetric, Constraint, TrailCharacterizer, World, generate_n
    shape = dict(height=4, width=5, n_agents=2, n_lasers=1, n_gems=1, n_exits=2, wall_fraction=0.12, n_voids=1, seed=0)
    worlds = list(generate_n(3, Constraint(10, Asymmetric()), batch=batch, max_attempts=32, characterizer=TrailCharacterizer, envs_per_map=64, **shape))
    other = list(generate_n(3, Constraint(10, Asymmetric()), batch=20 - batch, max_attempts=32, characterizer=TrailCharacterizer, **shape))
    assert len(worlds) == 3 and all(isinstance(w, World) for w in worlds)
    assert [w.world_string for w in worlds] == [w.world_string for w in other], "the worlds do not depend on the batch"
    for w in worlds:
        c = TrailCharacterizer(w, 10)
        try:
            assert c.is_asymmetric()
        finally:
            c._solver.free()


def test_every_kernel_was_launched(hf):
    """(last in the module: the tests above launch both kinds.)"""
    assert sorted(hf.compiled_kernels()) == KERNELS
    assert set(hf.launched_kernels()) == set(hf.compiled_kernels())
