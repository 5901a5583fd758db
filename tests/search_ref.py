"""The shortest-plan search of liblle_search.so restated over `oracle.OracleWorld`, without a GPU.

The oracle has no clone, so a state is kept as the list of joint actions that leads to it and is reached by replaying that prefix
from a reset.  Identity of a state: positions, arrived flags and every source's beam bits, plus the collected gems with collect_gems.
Mode "no-cooperation" forbids every state, the start state included, in which an agent stands on a laser tile (OracleWorld.lasers():
the tiles World.lasers lists, beam on or off) of a source of another colour.  A level is always finished before the search stops on a
goal, so `frontier` and `expanded` by depth are reproducible: frontier[d] = states first reached at depth d (frontier[0] = 1),
expanded[d] = available joint actions over the states of depth d.

Results are cached per (map, t_max, mode, collect_gems): the CPU and the GPU tests share one computation.
"""
import itertools
import json
import os
from dataclasses import dataclass, field

from oracle import oracle
from oracle.levels import LEVELS

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    with open(os.path.join(HERE, "golden", "kat_solver.json")) as f:
        return json.load(f)


def map_text(case):
    return LEVELS[case["level"]] if "level" in case else case["map"]


@dataclass
class Result:
    length: object                 # int, or None: no plan within t_max
    plan: object                   # list of joint actions (lists of action values), or None
    frontier: list = field(default_factory=list)
    expanded: list = field(default_factory=list)

    @property
    def n_states(self):
        return sum(self.frontier)


def foreign_colours(world):
    """{(i, j): colours of the sources that own a laser tile there}."""
    cells = {}
    for (i, j, _laser_id, agent_id, _on, _enabled) in world.lasers():
        cells.setdefault((i, j), set()).add(agent_id)
    return cells


def on_foreign_beam(world, cells):
    return any(cells.get(tuple(p), set()) - {a} for a, p in enumerate(world.positions()))


def replay(world, prefix):
    world.reset()
    for joint in prefix:
        world.step(list(joint))


def identity(world, collect_gems):
    key = (tuple(map(tuple, world.positions())), tuple(world.arrived()), tuple(tuple(world.beam_bits(l)) for l in range(world.n_sources)))
    return key + (tuple(world.gems_collected()),) if collect_gems else key


def is_goal(world, collect_gems):
    return all(world.arrived()) and (not collect_gems or all(world.gems_collected()))


_CACHE = {}


def search(text, t_max, mode="standard", collect_gems=False):
    key = (text, int(t_max), mode, bool(collect_gems))
    if key not in _CACHE:
        _CACHE[key] = _search(text, int(t_max), mode, bool(collect_gems))
    return _CACHE[key]


def _search(text, t_max, mode, collect_gems):
    assert mode in ("standard", "no-cooperation")
    world = oracle.OracleWorld(text)
    cells = foreign_colours(world) if mode == "no-cooperation" else None
    world.reset()
    res = Result(None, None, [1], [])
    if not all(world.alive()) or (cells is not None and on_foreign_beam(world, cells)):
        return res
    if is_goal(world, collect_gems):
        res.length, res.plan = 0, []
        return res
    seen = {identity(world, collect_gems)}
    frontier, depth = [()], 0
    while depth < t_max and frontier:
        new, expanded, goal = [], 0, None
        for prefix in frontier:
            replay(world, prefix)
            for joint in itertools.product(*world.available_actions()):
                expanded += 1
                replay(world, prefix)
                world.step(list(joint))  # (an available joint action is never refused: OracleError would fail the caller)
                if not all(world.alive()) or (cells is not None and on_foreign_beam(world, cells)):
                    continue
                k = identity(world, collect_gems)
                if k in seen:
                    continue
                seen.add(k)
                new.append(prefix + (joint,))
                if goal is None and is_goal(world, collect_gems):
                    goal = prefix + (joint,)
        depth += 1
        res.expanded.append(expanded)
        res.frontier.append(len(new))
        if goal is not None:
            res.length, res.plan = depth, [list(j) for j in goal]
            return res
        frontier = new
    return res


def check_plan(text, plan, mode="standard", collect_gems=False, length=None):
    """Replay `plan` (rows of action values) on a fresh oracle world and assert that it is a plan in the sense of the search."""
    world = oracle.OracleWorld(text)
    cells = foreign_colours(world)
    world.reset()
    if length is not None:
        assert len(plan) == length, (len(plan), length)
    assert all(world.alive())
    if mode == "no-cooperation":
        assert not on_foreign_beam(world, cells), "the start state has an agent on a foreign beam"
    for t, joint in enumerate(plan):
        assert len(joint) == world.n_agents
        world.step([int(a) for a in joint])  # raises OracleError when the joint action is refused
        assert all(world.alive()), f"an agent died at step {t}"
        if mode == "no-cooperation":
            assert not on_foreign_beam(world, cells), f"an agent stands on a foreign beam after step {t}"
    assert all(world.arrived()), "not every agent has arrived"
    if collect_gems:
        assert all(world.gems_collected())
