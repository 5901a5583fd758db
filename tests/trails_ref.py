"""The trail search of liblle_trails.so restated over `oracle.OracleWorld`, without a GPU -- TEST INFRASTRUCTURE for
tests/test_trails_cpu.py and tests/test_gpu_trails.py.

A breadth-first search in the style of tests/helpgraph_ref.py (a state is the list of joint actions that leads to it, reached by replay
from a reset) whose states remember how long the trails of help edges are that END at each agent: the identity of a state is
`search_ref.identity` plus a tuple L, L[a] = the number of edges of the longest trail that ends at agent a -- chained, times
non-decreasing, no temporal edge twice (lle_amd.characterization.TemporalCooperationGraph says the same in its own words).  The arcs
of one state, `coop_ref.detect`, lengthen it by `layer_update`: memoised recursion over (current agent, arcs of this state already
used), written from the definition; nothing here knows bit words, nibbles, cursors or budgets.  L is never saturated here: under
no-sequence-N a trajectory is dropped as soon as max(L) >= N, so every stored L is below N on both sides.

A level is always finished before the search stops on a goal, so `frontier` and `expanded` by depth are reproducible.  Results are
cached per (map, changes, t_max, N, collect_gems): the CPU and the GPU tests share one computation.

`changes` (optional everywhere; None: the map as its text gives it) has the meaning and the plain-data form of tests/helpgraph_ref.py:
sources disabled or recoloured and exits moved on the fresh OracleWorld before its reset (`helpgraph_ref.oracle_world`), and on an
lle_amd.World before a solver is constructed over it (`helpgraph_ref.apply_changes`).
"""
import itertools
import json
import os
from dataclasses import dataclass, field
from functools import lru_cache

from tests import coop_ref, search_ref
from tests.helpgraph_ref import apply_changes, changes_key, changes_label, oracle_world  # noqa: F401  (re-exported: one meaning of `changes`)

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    """tests/golden/kat_trails.json (tests/golden/make_kat_trails.py says what the keys mean)."""
    with open(os.path.join(HERE, "golden", "kat_trails.json")) as f:
        return json.load(f)


@dataclass
class Result:
    length: object                 # int, or None: no plan within t_max
    plan: object                   # list of joint actions (lists of action values), or None
    frontier: list = field(default_factory=list)
    expanded: list = field(default_factory=list)
    trails: object = None          # L of the plan's last state, a tuple; None without a plan
    peak: int = 0                  # the greatest max(L) over the records stored
    twins: int = 0                 # records stored whose world state was stored in the same level with another L
    merges: int = 0                # successors dropped as duplicates of a record stored in the same level under another parent

    @property
    def n_states(self):
        return sum(self.frontier)


def layer_update(L, arcs):
    """L after one more state whose help arcs are `arcs` (pairs (helper, beneficiary)): a trail that ends at x may go on along any
    sequence of distinct arcs of the state, each starting where the one before ends."""
    arcs = frozenset(arcs)
    if not arcs:
        return tuple(L)

    @lru_cache(maxsize=None)
    def reach(current, used):
        """{agent: the most arcs of a walk from `current` to it over arcs not in `used`} (current itself: 0)."""
        out = {current: 0}
        for arc in arcs:
            if arc[0] != current or arc in used:
                continue
            for agent, n in reach(arc[1], used | {arc}).items():
                out[agent] = max(out.get(agent, 0), n + 1)
        return out

    new = list(L)
    for x in range(len(L)):
        for y, n in reach(x, frozenset()).items():
            if n > 0:
                new[y] = max(new[y], L[x] + n)
    return tuple(new)


_CACHE = {}


def search(text, t_max, n, collect_gems=False, changes=None):
    key = (text, changes_key(changes), int(t_max), int(n), bool(collect_gems))
    if key not in _CACHE:
        _CACHE[key] = _search(text, int(t_max), int(n), bool(collect_gems), changes)
    return _CACHE[key]


def _search(text, t_max, n, collect_gems, changes=None):
    assert n >= 2
    world = oracle_world(text, changes)
    A = world.n_agents
    world.reset()
    res = Result(None, None, [1], [])
    root = layer_update((0,) * A, coop_ref.detect(world))
    if not all(world.alive()) or max(root) >= n:
        return res
    res.peak = max(root)
    if search_ref.is_goal(world, collect_gems):
        res.length, res.plan, res.trails = 0, [], root
        return res
    seen = {(search_ref.identity(world, collect_gems), root)}
    frontier, depth = [((), root)], 0
    while depth < t_max and frontier:
        new, expanded, goal = [], 0, None
        level = {}  # record -> index of the parent that stored it; world state -> the Ls stored in this level
        states = {}
        for parent, (prefix, L) in enumerate(frontier):
            search_ref.replay(world, prefix)
            for joint in itertools.product(*world.available_actions()):
                expanded += 1
                search_ref.replay(world, prefix)
                world.step(list(joint))
                if not all(world.alive()):
                    continue
                mine = layer_update(L, coop_ref.detect(world))
                if max(mine) >= n:
                    continue
                ident = search_ref.identity(world, collect_gems)
                k = (ident, mine)
                if k in seen:
                    res.merges += k in level and level[k] != parent
                    continue
                seen.add(k)
                level[k] = parent
                states.setdefault(ident, set()).add(mine)
                res.peak = max(res.peak, max(mine))
                new.append((prefix + (joint,), mine))
                if goal is None and search_ref.is_goal(world, collect_gems):
                    goal = (prefix + (joint,), mine)
        depth += 1
        res.twins += sum(len(v) for v in states.values() if len(v) > 1)
        res.expanded.append(expanded)
        res.frontier.append(len(new))
        if goal is not None:
            res.length, res.plan, res.trails = depth, [list(j) for j in goal[0]], goal[1]
            return res
        frontier = new
    return res


def replay_trails(text, plan, changes=None):
    """(L after the last state of `plan` by `layer_update`, the temporal edges (helper, beneficiary, t), the world) on a fresh oracle
    world with `changes` applied; asserts that nobody dies."""
    world = oracle_world(text, changes)
    world.reset()
    assert all(world.alive())
    arcs = coop_ref.detect(world)
    L = layer_update((0,) * world.n_agents, arcs)
    edges = [(h, b, 0) for h, b in arcs]
    for t, joint in enumerate(plan, start=1):
        assert len(joint) == world.n_agents
        world.step([int(a) for a in joint])  # raises OracleError when the joint action is refused
        assert all(world.alive()), f"an agent died at step {t - 1}"
        arcs = coop_ref.detect(world)
        L = layer_update(L, arcs)
        edges += [(h, b, t) for h, b in arcs]
    return L, edges, world


def check_plan(text, plan, n, collect_gems=False, length=None, changes=None):
    """Replay `plan` (rows of action values) on a fresh oracle world (under `changes`): nobody dies, everybody arrives, and the longest trail of the
    replay's temporal edges -- by the package's host-side graph, lle_amd.characterization.TemporalCooperationGraph, which shares no
    code with `layer_update` -- is shorter than `n`.  Returns L of the last state (whose maximum is that longest trail)."""
    from lle_amd.characterization import DependencyEdge, TemporalCooperationGraph
    if length is not None:
        assert len(plan) == length, (len(plan), length)
    L, edges, world = replay_trails(text, plan, changes)
    assert all(world.arrived()), "not every agent has arrived"
    if collect_gems:
        assert all(world.gems_collected())
    longest = TemporalCooperationGraph([DependencyEdge(h, b, t) for h, b, t in edges]).longest_trail_length()
    assert longest < n, (n, longest, sorted(edges, key=lambda e: e[2]))
    assert longest == max(L), (longest, L)
    return L


# ---------------------------------------------------------------------------------------------- the reference's predicate
def is_sequential(text, t_max, length, changes=None):
    """The reference's WorldCharacterizer.is_sequential (world_characterization.py) answered with this search: solvable within t_max
    and no plan within t_max avoids every trail of `length` edges.  (The reference asks the shortest plan's profile first: a plan that
    holds such a trail is implied by "no plan avoids it", so the answers are the same.)"""
    from tests import helpgraph_ref
    if helpgraph_ref.search(text, t_max, changes=changes).length is None:
        return False
    return search(text, t_max, length, changes=changes).length is None
