"""The closed-trail search of liblle_cycles.so restated over `oracle.OracleWorld`, without a GPU -- TEST INFRASTRUCTURE for
tests/test_cycles_cpu.py and tests/test_gpu_cycles.py.

A breadth-first search in the style of tests/trails_ref.py (a state is the list of joint actions that leads to it, reached by replay
from a reset) whose states remember which trails of help edges the trajectory holds: the identity of a state is
`search_ref.identity` plus a frozenset R of triples (anchor, current, support) -- some trail (chained, times non-decreasing, no
temporal edge twice) leads from `anchor` to `current` and visits exactly the agents of the frozenset `support`.  The arcs of one
state, `coop_ref.detect`, extend it by `layer_update`, written from the definition: every non-empty trail inside the state (a
sequence of distinct arcs, each starting where the one before ends) is enumerated by recursion and appended to every triple of R
that stands at its first agent, and to the empty trail (x, x, {x}).  Nothing here knows bit words, subsets as masks, stacks or budgets.

THE PRUNING RULE (the words of lle_amd/cycles/cycles_logic.hpp and include/lle_cycles.h).  Under no-interdependence-N:
  a triple with |S| > N is never stored, because supports only grow;
  a trajectory is dropped the moment some (a, a, S) with |S| = N appears;
  kept are (a, c, S) with a != c and |S| <= N, and (a, a, S) with |S| < N.
`layer_update(R, arcs)` without an order prunes nothing; `closes(R, n)` says whether some (a, a, S) has |S| = n.

A level is always finished before the search stops on a goal, so `frontier` and `expanded` by depth are reproducible.  Results are
cached per (map, changes, t_max, N, collect_gems): the CPU and the GPU tests share one computation.  `changes` as in
tests/helpgraph_ref.py.
"""
import itertools
import json
import os
from dataclasses import dataclass, field

from tests import coop_ref, search_ref
from tests.helpgraph_ref import apply_changes, changes_key, changes_label, oracle_world  # noqa: F401  (re-exported: one meaning of `changes`)

HERE = os.path.dirname(os.path.abspath(__file__))


def load_cases():
    """tests/golden/kat_cycles.json (tests/golden/make_kat_cycles.py says what the keys mean)."""
    with open(os.path.join(HERE, "golden", "kat_cycles.json")) as f:
        return json.load(f)


@dataclass
class Result:
    length: object                 # int, or None: no plan within t_max
    plan: object                   # list of joint actions (lists of action values), or None
    frontier: list = field(default_factory=list)
    expanded: list = field(default_factory=list)
    triples: object = None         # R of the plan's last state, a frozenset; None without a plan
    twins: int = 0                 # records stored whose world state was stored in the same level with another R
    merges: int = 0                # successors dropped as duplicates of a record stored in the same level under another parent

    @property
    def n_states(self):
        return sum(self.frontier)

    @property
    def closed_orders(self):
        return None if self.triples is None else sorted({len(s) for a, c, s in self.triples if a == c})


def trails_inside(arcs):
    """Every non-empty trail inside one state as (first agent, last agent, frozenset of the agents it touches): sequences of distinct
    arcs (helper, beneficiary), each starting where the one before ends."""
    arcs = frozenset(arcs)
    found = set()

    def walk(first, current, used, touched):
        for arc in arcs:
            if arc[0] != current or arc in used:
                continue
            seen = touched | {arc[1]}
            found.add((first, arc[1], seen))
            walk(first, arc[1], used | {arc}, seen)

    for x in {h for h, _b in arcs}:
        walk(x, x, frozenset(), frozenset({x}))
    return found


def layer_update(R, arcs, n=None):
    """R after one more state whose help arcs are `arcs`; with `n`, triples of more than n agents are not stored.  (A closed triple of
    exactly n agents is stored here: `closes` finds it, and the search drops the trajectory.)"""
    new = set(R)
    for x, y, touched in trails_inside(arcs):
        for a, c, support in set(R) | {(x, x, frozenset({x}))}:
            if c == x and (n is None or len(support | touched) <= n):
                new.add((a, y, support | touched))
    return frozenset(new)


def closes(R, n):
    return any(a == c and len(s) == n for a, c, s in R)


_CACHE = {}


def search(text, t_max, n, collect_gems=False, changes=None):
    key = (text, changes_key(changes), int(t_max), int(n), bool(collect_gems))
    if key not in _CACHE:
        _CACHE[key] = _search(text, int(t_max), int(n), bool(collect_gems), changes)
    return _CACHE[key]


def _search(text, t_max, n, collect_gems, changes=None):
    assert n >= 2
    world = oracle_world(text, changes)
    world.reset()
    res = Result(None, None, [1], [])
    root = layer_update(frozenset(), coop_ref.detect(world), n)
    if not all(world.alive()) or closes(root, n):
        return res
    if search_ref.is_goal(world, collect_gems):
        res.length, res.plan, res.triples = 0, [], root
        return res
    seen = {(search_ref.identity(world, collect_gems), root)}
    frontier, depth = [((), root)], 0
    updates = {}  # (R, arcs) -> R': many successors share both
    while depth < t_max and frontier:
        new, expanded, goal = [], 0, None
        level = {}  # record -> index of the parent that stored it; world state -> the Rs stored in this level
        states = {}
        for parent, (prefix, R) in enumerate(frontier):
            search_ref.replay(world, prefix)
            for joint in itertools.product(*world.available_actions()):
                expanded += 1
                search_ref.replay(world, prefix)
                world.step(list(joint))
                if not all(world.alive()):
                    continue
                arcs = frozenset(coop_ref.detect(world))
                if (R, arcs) not in updates:
                    updates[(R, arcs)] = layer_update(R, arcs, n)
                mine = updates[(R, arcs)]
                if closes(mine, n):
                    continue
                ident = search_ref.identity(world, collect_gems)
                k = (ident, mine)
                if k in seen:
                    res.merges += k in level and level[k] != parent
                    continue
                seen.add(k)
                level[k] = parent
                states.setdefault(ident, set()).add(mine)
                new.append((prefix + (joint,), mine))
                if goal is None and search_ref.is_goal(world, collect_gems):
                    goal = (prefix + (joint,), mine)
        depth += 1
        res.twins += sum(len(v) for v in states.values() if len(v) > 1)
        res.expanded.append(expanded)
        res.frontier.append(len(new))
        if goal is not None:
            res.length, res.plan, res.triples = depth, [list(j) for j in goal[0]], goal[1]
            return res
        frontier = new
    return res


def replay_triples(text, plan, n=None, changes=None):
    """(R after the last state of `plan` by `layer_update` -- pruned to n when given --, the temporal edges (helper, beneficiary, t),
    the world) on a fresh oracle world with `changes` applied; asserts that nobody dies."""
    world = oracle_world(text, changes)
    world.reset()
    assert all(world.alive())
    arcs = coop_ref.detect(world)
    R = layer_update(frozenset(), arcs, n)
    edges = [(h, b, 0) for h, b in arcs]
    for t, joint in enumerate(plan, start=1):
        assert len(joint) == world.n_agents
        world.step([int(a) for a in joint])  # raises OracleError when the joint action is refused
        assert all(world.alive()), f"an agent died at step {t - 1}"
        arcs = coop_ref.detect(world)
        R = layer_update(R, arcs, n)
        edges += [(h, b, t) for h, b in arcs]
    return R, edges, world


def check_plan(text, plan, n, collect_gems=False, length=None, changes=None, triples=None, closed_orders=None):
    """Replay `plan` (rows of action values) on a fresh oracle world (under `changes`): nobody dies, everybody arrives, and by the
    package's host-side graph, lle_amd.characterization.TemporalCooperationGraph, which shares no code with `layer_update`: there is
    no closed trail of order `n`, and for every k < n `has_closed_trail_of_order(k)` equals `k in closed_orders` (the replay's own when
    None is given).  `triples` (when given) equals the replay's R.  Returns that R."""
    from lle_amd.characterization import DependencyEdge, TemporalCooperationGraph
    if length is not None:
        assert len(plan) == length, (len(plan), length)
    R, edges, world = replay_triples(text, plan, n, changes)
    assert all(world.arrived()), "not every agent has arrived"
    if collect_gems:
        assert all(world.gems_collected())
    graph = TemporalCooperationGraph([DependencyEdge(h, b, t) for h, b, t in edges])
    assert not graph.has_closed_trail_of_order(n), (n, sorted(edges, key=lambda e: e[2]))
    assert not closes(R, n)
    orders = sorted({len(s) for a, c, s in R if a == c}) if closed_orders is None else list(closed_orders)
    for k in range(2, n):
        assert graph.has_closed_trail_of_order(k) == (k in orders), (k, orders, sorted(edges, key=lambda e: e[2]))
    assert all(2 <= k < n for k in orders), orders
    if triples is not None:
        assert set(triples) == set(R), (sorted(map(str, set(triples) ^ set(R))))
    return R


# ---------------------------------------------------------------------------------------------- the reference's predicate
def is_interdependent(text, t_max, order, changes=None):
    """The reference's WorldCharacterizer.is_interdependent (world_characterization.py) answered with this search: solvable within
    t_max and no plan within t_max avoids every closed trail over exactly `order` agents.  (The reference asks the shortest plan's
    profile first: a plan that holds such a trail is implied by "no plan avoids it", so the answers are the same.)"""
    from tests import helpgraph_ref
    if helpgraph_ref.search(text, t_max, changes=changes).length is None:
        return False
    return search(text, t_max, order, changes=changes).length is None
