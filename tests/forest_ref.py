"""The fixed input sets of the forest tests (tests/test_forest_cpu.py, tests/test_gpu_forest.py) and their oracle: per map
`tests/search_ref.search`, whose results are cached per (map, t_max, mode, collect_gems) and shared by every test of the process.

Set A: sixteen 4x5 maps of two agents, one laser, one gem, a void; t_max = 10.  One forest holds maps solved at depths 1 to 9, two
       that run empty (depths 10 and 9: seeds 8 and 13) and three that need cooperation (seeds 1, 7, 10).
Set B: sixteen 5x5 maps of two agents, two lasers, one gem; t_max = 12.  Seeds 5 and 8 stop at the horizon with a live frontier,
       seeds 3 and 7 need cooperation.
Set C: six 4x4 maps of three agents (pitch 4, 125 joint actions per state), one laser; t_max = 8.
"""
from dataclasses import dataclass

from lle_amd import mapgen
from tests import search_ref

MODES = ("standard", "no-cooperation")


@dataclass(frozen=True)
class InputSet:
    name: str
    maps: tuple
    t_max: int


SET_A = InputSet("A", tuple(mapgen.generate(4, 5, 2, 1, 1, n_exits=2, wall_fraction=0.12, n_voids=1, seed=s) for s in range(16)), 10)
SET_B = InputSet("B", tuple(mapgen.generate(5, 5, 2, 2, 1, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s) for s in range(16)), 12)
SET_C = InputSet("C", tuple(mapgen.generate(4, 4, 3, 1, 0, n_exits=3, wall_fraction=0.12, n_voids=0, seed=s) for s in range(6)), 8)
SETS = {s.name: s for s in (SET_A, SET_B, SET_C)}

# what the oracle gives for the sets (checked by tests/test_forest_cpu.py)
A_STANDARD_LENGTHS = [4, 6, 5, 6, 3, 7, 5, 9, None, 1, 6, 5, 2, None, 3, 5]
A_COOPERATIVE_SEEDS = [1, 7, 10]
A_GEM_LENGTHS_FIRST_8 = [7, 6, 5, 6, 8, None, 7, 9]
A_OVER_128_STATES = [2, 3, 7, 15]
B_HORIZON_SEEDS = [5, 8]
B_COOPERATIVE_SEEDS = [3, 7]


def oracle(maps, t_max, mode="standard", collect_gems=False):
    """[search_ref.Result] per map."""
    return [search_ref.search(text, t_max, mode, collect_gems) for text in maps]


def assert_map_equals_oracle(text, ref, res, m, mode="standard", collect_gems=False):
    """Map m of the ForestResult `res` against the oracle's Result `ref`: length, counters, stored states, and the plan replayed."""
    length = None if res.length[m] < 0 else int(res.length[m])
    assert res.status[m] == 0, (m, res.status[m])
    assert length == ref.length, (m, length, ref.length)
    assert res.frontier[m] == ref.frontier and res.expanded[m] == ref.expanded, (m, res.frontier[m], ref.frontier, res.expanded[m], ref.expanded)
    assert int(res.n_states[m]) == ref.n_states and int(res.depth_reached[m]) == len(ref.expanded), (m, res.n_states[m], ref.n_states)
    assert (res.plans[m] is None) == (ref.length is None)
    if res.plans[m] is not None:
        search_ref.check_plan(text, [[a.value for a in row] for row in res.plans[m]], mode, collect_gems, length=ref.length)
