"""The help forest on the MI355X where tests/test_gpu_helpforest.py does not reach: trail fields up to 15 and a map whose frontier runs
empty while its neighbour is long solved, ONE layout several times under different edge rules, a pool that fits one map exactly, cell
tables of more than 256 cells per map, and six agents under an N that stores trails of two edges.

Every comparison is exact and is `assert_equals_golden` of tests/test_gpu_helpforest.py: per map length, per-depth frontier and expanded
counters, stored records and depth_reached against tests/golden/kat_helpforest.json, which tests/test_helpforest_cpu.py holds the
restatements (tests/helpgraph_ref.py, tests/trails_ref.py) to; every plan replayed on the oracle under its mode and the map's `changes`;
the goal's help edges or trail equal to the replay's; the piece count what `expected_pieces` says.  No test here walks a search in Python.

The smallest shapes at which these can go wrong (tests/helpforest_ref.py draws the sets):
  set L (4 x 6, 2 agents, t_max 24)   long-trails | long-trails with source 1 disabled | two-agent-mutual-compact.  Under no-sequence-N
        the first map stores 100 + 76 (N - 2) records with fields up to N - 1 <= 15 and walks N + 5 levels until its frontier is empty;
        the third is solved at depth 5 and idles for 16 levels; the second has the first's cell table and another rule.
  set C (4 x 4, 2 agents, t_max 8)    two-agent-mutual-compact four times: unchanged, source 1 disabled, source 0 disabled, source 1
        recoloured to 0.  Equal texts, equal cell tables up to the owner bits, four different (length, records) in every mode: only
        `rules[map]` tells them apart.
  max_states_per_map = 1088 on set L  fits the first map under no-sequence-15 exactly and is 76 records short under no-sequence-16.
  20 x 20, 65 x 66, 6 x 255, 255 x 6  around sets L and R (20 x 20 and 255 x 6): 400 to 4 290 cells per map, so map m's table starts
        m * H * W words in; a map laid out in the OTHER corner stands at index 0, so a wrong offset reads other tiles.
  set X (4 x 8, 6 agents, t_max 3)    under no-sequence-3: trails of two edges stored, the sixth field (bits 20-23) non-zero."""
import pytest

from tests import helpforest_ref, helpgraph_ref
from tests.helpforest_ref import MAPS, SET_C, SET_L, SET_X, embed_top_left, mode_text
from tests.test_gpu_helpforest import LLE_CAPACITY, QUESTIONS, assert_equals_golden, expected_pieces, golden, hf, run  # noqa: F401  (hf: the fixture)

pytestmark = pytest.mark.gpu

def answers(refs):
    return [(r["length"], r["states"]) for r in refs]


# ---------------------------------------------------------------------------------------------------------------- set L: long trails
L_RUNS = [(mode, param, E) for mode, param in SET_L.modes for E in (256, 64)] + [("no-sequence", 16, 7)]


@pytest.mark.parametrize("mode, param, E", L_RUNS, ids=[f"{mode_text(m, p)}-E{E}" for m, p, E in L_RUNS])
def test_long_trails_beside_a_map_that_is_long_solved(hf, mode, param, E):
    """Set L: the first map walks N + 5 levels (9 under `standard`) until its frontier is empty, the second 8, the third is solved at
    depth 5; the pieces of a level are what the map that still walks needs."""
    refs = golden(SET_L, mode, param)
    res = assert_equals_golden(hf, SET_L.maps, refs, SET_L.t_max, mode, param, changes=SET_L.changes, envs_per_map=E)
    assert not res.status.any() and res.length.tolist() == [-1, -1, 5]
    if mode == "no-sequence":
        assert res.depth_reached.tolist() == [param + 5, 8, 5] and res.n_states.tolist() == [100 + 76 * (param - 2), 198, 126]
        assert res.frontier[0][-1] == 0 and len(res.frontier[0]) == param + 6 and 2 <= max(res.trail[2]) < param
        assert res.trail[0] is None and res.trail[1] is None
    else:
        assert res.depth_reached.tolist() == [9, 8, 5] and res.n_states.tolist() == [203, 198, 123]
    assert res.pieces == expected_pieces(refs, 25, E) and res.launched_lanes == res.pieces * 3 * E


# ---------------------------------------------------------------------------------------------------------------- set C: one layout, four rules
@pytest.mark.parametrize("E", [256, 64, 7])
@pytest.mark.parametrize("mode, param", SET_C.modes, ids=[mode_text(m, p) for m, p in SET_C.modes])
def test_one_layout_under_four_edge_rules(hf, mode, param, E):
    """Set C: every map gives its own answer -- and the same four worlds in the order [3, 0, 2, 1, 0]: the answers follow the worlds."""
    refs = golden(SET_C, mode, param)
    assert len(set(answers(refs))) == 4, "four worlds, four answers"
    res = assert_equals_golden(hf, SET_C.maps, refs, SET_C.t_max, mode, param, changes=SET_C.changes, envs_per_map=E)
    assert not res.status.any() and [(None if n < 0 else n, s) for n, s in zip(res.length.tolist(), res.n_states.tolist())] == answers(refs)
    order = [3, 0, 2, 1, 0]
    res = assert_equals_golden(hf, [SET_C.maps[i] for i in order], [refs[i] for i in order], SET_C.t_max, mode, param, changes=[SET_C.changes[i] for i in order],
                               envs_per_map=E)
    assert [(None if n < 0 else n, s) for n, s in zip(res.length.tolist(), res.n_states.tolist())] == [answers(refs)[i] for i in order]
    assert res.frontier[1] == res.frontier[4] and res.expanded[1] == res.expanded[4]


# ---------------------------------------------------------------------------------------------------------------- capacity
@pytest.mark.parametrize("E", [256, 64])
def test_a_pool_that_fits_one_map_exactly(hf, E):
    """Set L with 1088 records per map: no-sequence-15 answers every map -- the first stores exactly 1088 -- and no-sequence-16 leaves
    exactly the first without an answer; the other two keep their recorded counters."""
    assert golden(SET_L, "no-sequence", 15)[0]["states"] == 1088 < golden(SET_L, "no-sequence", 16)[0]["states"] == 1164
    res = assert_equals_golden(hf, SET_L.maps, golden(SET_L, "no-sequence", 15), SET_L.t_max, "no-sequence", 15, changes=SET_L.changes, envs_per_map=E,
                               max_states_per_map=1088)
    assert not res.status.any() and res.n_states[0] == 1088
    refs = golden(SET_L, "no-sequence", 16)
    res = run(hf, SET_L.worlds, SET_L.t_max, "no-sequence", 16, envs_per_map=E, max_states_per_map=1088)
    print(res.status.tolist(), res.n_states.tolist(), res.depth_reached.tolist())
    assert res.status.tolist() == [LLE_CAPACITY, 0, 0]
    assert res.length[0] == -1 and res.plans[0] is None and res.n_states[0] == 1088 and res.frontier[0] == [1] and res.expanded[0] == [] and res.trail[0] is None
    for m in (1, 2):
        helpforest_ref.assert_map_equals_golden(SET_L.maps[m], refs[m], res, m, "no-sequence", 16, changes=SET_L.changes[m])


# ---------------------------------------------------------------------------------------------------------------- far corner
FAR = [("L", size) for size in ((20, 20), (65, 66), (6, 255), (255, 6))] + [("R", size) for size in ((20, 20), (255, 6))]
FAR_MODES = {"L": (("no-sequence", 16), ("standard", 2)), "R": (("no-convergence", 2), ("no-sequence", 3))}
FIRST = {"L": 2, "R": 3}  # the map of the set that also stands at index 0, in the other corner: two-agent-mutual-compact, chain-at-reset


@pytest.mark.parametrize("name, size", FAR, ids=[f"{n}-{h}x{w}" for n, (h, w) in FAR])
def test_the_sets_in_the_far_corner(hf, name, size):
    """The maps of the set, each in the bottom-right corner of a map of walls (every laser tile behind the first 256 cells of its
    map's table, coordinate bytes up to 254; long-trails keeps two columns of walls and exits to its right, so its beams end at column
    W - 3), behind a map laid out in the top-left corner: map m's table starts m * H * W words in,
    and what lies one table earlier has its tiles elsewhere.  Counters are the small sets'."""
    from lle_amd import Map
    s = helpforest_ref.SETS[name]
    height, width = size
    first = embed_top_left(MAPS[s.names[FIRST[name]]], height, width)
    maps = [first] + [helpgraph_ref.embed(text, height, width) for text in s.maps]
    changes = [None] + list(s.changes)
    near = {t.i * width + t.j for t in Map(first).laser_tiles()}
    assert near and max(near) < 5 * width, "the first map's beams lie at the start of its table"
    for text in maps[1:]:
        tiles = Map(text).laser_tiles()
        far = {t.i * width + t.j for t in tiles}
        assert tiles and min(far) >= 256 and not far & near and max(t.i for t in tiles) >= height - 3 and max(t.j for t in tiles) >= width - 3
    for mode, param in FAR_MODES[name]:
        refs = golden(s, mode, param)
        res = assert_equals_golden(hf, maps, [refs[FIRST[name]]] + refs, s.t_max, mode, param, changes=changes, envs_per_map=64, max_states_per_map=2048)
        assert not res.status.any()


# ---------------------------------------------------------------------------------------------------------------- six agents
@pytest.mark.parametrize("E", [4096, 256])
def test_six_agents_store_trails_of_two_edges(hf, E):
    """Set X under no-sequence-3 (1 856 and 4 540 records): the mutual pair of six-mutual is 3 <-> 5, so every plan ends a trail at
    agent 5 -- the sixth field, bits 20-23 -- and some trail of the set has two edges."""
    res = assert_equals_golden(hf, SET_X.maps, golden(SET_X, "no-sequence", 3), SET_X.t_max, "no-sequence", 3, envs_per_map=E)
    assert not res.status.any() and res.length.tolist() == [3, 3]
    assert res.trail[0][5] > 0 and max(max(t) for t in res.trail) == 2 and all(max(t) < 3 for t in res.trail)


# ---------------------------------------------------------------------------------------------------------------- characterisations
EDGE_QUESTIONS = QUESTIONS + [("is_sequential", None, (16,))]


@pytest.mark.parametrize("name", ["C", "L"])
def test_characterize_many_equals_a_characterizer_per_changed_world(hf, name):
    from lle_amd import World, trails
    s = helpforest_ref.SETS[name]
    assert [q for q in EDGE_QUESTIONS if q[0] == "is_sequential"] == [("is_sequential", None, (2,)), ("is_sequential", None, (3,)), ("is_sequential", None, (16,))]
    with hf.characterize_many(s.worlds, s.t_max, envs_per_map=64) as many:
        got = {(q, args): (getattr(many, attr) if attr else getattr(many, q)(*args)) for q, attr, args in EDGE_QUESTIONS}
        assert all(a.dtype == bool and a.shape == (len(s.maps),) for a in got.values())
        for i, (text, changes) in enumerate(zip(s.maps, s.changes)):
            c = trails.TrailCharacterizer(helpgraph_ref.apply_changes(World(text), changes), s.t_max)
            try:
                for q, _attr, args in EDGE_QUESTIONS:
                    assert bool(got[(q, args)][i]) == getattr(c, q)(*args), (s.names[i], q, args)
                    assert getattr(many.entry(i), q)(*args) == bool(got[(q, args)][i])
            finally:
                c._solver.free()
    print(name, {k: v.tolist() for k, v in got.items()})
    if name == "C":  # what the golden file says of the four worlds
        assert got[("is_solvable", ())].tolist() == [True, True, True, False]
        assert got[("is_sequential", (2,))].tolist() == [True, False, False, False] and not got[("is_sequential", (3,))].any()
    else:
        assert got[("is_solvable", ())].tolist() == [False, False, True] and got[("is_sequential", (2,))].tolist() == [False, False, True]
        assert not got[("is_sequential", (16,))].any()


def test_every_kernel_was_launched(hf):
    """(last in the module: the tests above launch both kinds.)"""
    from tests.test_gpu_helpforest import KERNELS
    assert sorted(hf.compiled_kernels()) == KERNELS
    assert set(hf.launched_kernels()) == set(hf.compiled_kernels())
