"""The help-graph search of liblle_helpgraph.so restated over `oracle.OracleWorld`, without a GPU -- TEST INFRASTRUCTURE for
tests/test_helpgraph_cpu.py and tests/test_gpu_helpgraph.py.

A breadth-first search in the style of tests/search_ref.py (a state is the list of joint actions that leads to it, reached by replay
from a reset) whose states remember who has helped whom: the identity of a state is `search_ref.identity` plus the FLATTENED help
relation of its trajectory, a frozenset of (helper, beneficiary) pairs that grows by `coop_ref.detect` of every state, the reset state
included.  Nothing here knows bit words, cell tables or colour masks.

The modes, as the reference's predicates define them on a flattened relation E (python/lle/characterization/plan/graph.py, profile.py):
  standard           no restriction
  no-convergence k   a trajectory is dropped as soon as some beneficiary has >= k distinct helpers
  no-divergence k    ... as soon as some helper has >= k distinct beneficiaries
  no-mutual          ... as soon as E holds (a, b) and (b, a)
  no-fully-coupled   ... as soon as E holds all A (A - 1) ordered pairs, A >= 2
  no-asymmetric      judged at the goal only: a goal state counts when no edge of E has a helper that is nobody's beneficiary; goal
                     states that do not count are stored like any other (they are absorbing)
A level is always finished before the search stops on a goal, so `frontier` and `expanded` by depth are reproducible.

Results are cached per (map, changes, t_max, mode, param, collect_gems): the CPU and the GPU tests share one computation.

`changes` (optional everywhere; None: the map as its text gives it) is plain data, as tests/golden/kat_helpgraph.json stores it:
  {"sources": [{"laser_id": 0, "enabled": false, "colour": null}, ...], "exits": [[i, j], ...]}
Either key may be missing; `enabled` / `colour` null or missing: left as the text has it.  It is applied to the fresh OracleWorld with
set_source / set_exits before the reset (`oracle_world`), and to an lle_amd.World through LaserSource.disable() / enable() /
set_colour() and the exit_pos setter (`apply_changes`) before a solver is constructed over it.
"""
import itertools
import json
import os
from dataclasses import dataclass, field

from oracle import oracle
from tests import coop_ref, search_ref

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("standard", "no-asymmetric", "no-mutual", "no-fully-coupled", "no-convergence", "no-divergence")


def load_cases():
    """tests/golden/kat_helpgraph.json (tests/golden/make_kat_helpgraph.py says what the keys mean)."""
    with open(os.path.join(HERE, "golden", "kat_helpgraph.json")) as f:
        return json.load(f)


@dataclass
class Result:
    length: object                 # int, or None: no plan within t_max
    plan: object                   # list of joint actions (lists of action values), or None
    frontier: list = field(default_factory=list)
    expanded: list = field(default_factory=list)
    edges: object = None           # the flattened help relation of the plan, a set of pairs; None without a plan

    @property
    def n_states(self):
        return sum(self.frontier)


def violates(edges, mode, param, n_agents):
    """Whether the flattened relation `edges` is one the monotone mode `mode` rejects."""
    helpers, beneficiaries = {}, {}
    for h, b in edges:
        helpers.setdefault(b, set()).add(h)
        beneficiaries.setdefault(h, set()).add(b)
    if mode == "no-convergence":
        return any(len(v) >= param for v in helpers.values())
    if mode == "no-divergence":
        return any(len(v) >= param for v in beneficiaries.values())
    if mode == "no-mutual":
        return any((b, h) in edges for h, b in edges)
    if mode == "no-fully-coupled":
        return n_agents >= 2 and len(edges) == n_agents * (n_agents - 1)
    return False


def accepts(edges, mode):
    """Whether a goal state whose trajectory has the flattened relation `edges` counts under `mode`."""
    if mode != "no-asymmetric":
        return True
    helped = {b for _h, b in edges}
    return all(h in helped for h, _b in edges)


def changes_key(changes):
    """`changes` as a hashable value: equal data, equal key."""
    return None if changes is None else json.dumps(changes, sort_keys=True)


def oracle_world(text, changes=None):
    """A fresh OracleWorld of the map text with `changes` applied; not reset yet."""
    world = oracle.OracleWorld(text)
    if changes is not None:
        assert set(changes) <= {"sources", "exits"}, sorted(changes)
        for src in changes.get("sources", ()):
            assert set(src) <= {"laser_id", "enabled", "colour"} and 0 <= src["laser_id"] < world.n_sources, src
            world.set_source(src["laser_id"], enabled=src.get("enabled"), colour=src.get("colour"))
        if "exits" in changes:
            world.set_exits(changes["exits"])
    return world


def apply_changes(world, changes=None):
    """The same data on an lle_amd.World, through its public mutators; returns the world.  Call it before the solver is constructed: a
    solver keeps the map as it is at construction."""
    if changes is not None:
        assert set(changes) <= {"sources", "exits"}, sorted(changes)
        sources = {s.laser_id: s for s in world.laser_sources}
        for src in changes.get("sources", ()):
            handle = sources[src["laser_id"]]
            if src.get("enabled") is not None:
                handle.enable() if src["enabled"] else handle.disable()
            if src.get("colour") is not None:
                handle.set_colour(src["colour"])
        if "exits" in changes:
            world.exit_pos = [tuple(p) for p in changes["exits"]]
    return world


def changes_label(changes):
    """A short name of `changes` for test ids: "" for None, else e.g. "-source0-off", "-source0-colour1", "-exits-1.1-2.2"."""
    if changes is None:
        return ""
    parts = []
    for src in changes.get("sources", ()):
        parts += [f"source{src['laser_id']}" + ("" if src.get("enabled") is None else "-on" if src["enabled"] else "-off")
                  + ("" if src.get("colour") is None else f"-colour{src['colour']}")]
    if "exits" in changes:
        parts.append("exits-" + "-".join(f"{i}.{j}" for i, j in changes["exits"]))
    return "-" + "-".join(parts)


def n_agents_of(text):
    """The number of agents of a map text: its distinct start tokens S<k>."""
    return len({tok for tok in text.split() if tok[0] == "S" and tok[1:].isdigit()})


def embed(text, height, width):
    """The map `text` in the bottom-right corner of a height x width map that is wall everywhere else: the same world (walls on every
    side of a map change nothing), every cell it uses at the far end of the cell table and of the position bytes."""
    rows = [line.split() for line in text.strip().splitlines()]
    h, w = len(rows), len(rows[0])
    assert all(len(r) == w for r in rows) and h <= height and w <= width
    return "\n".join(" ".join(rows[i - (height - h)][j - (width - w)] if i >= height - h and j >= width - w else "@" for j in range(width))
                     for i in range(height))


_CACHE = {}


def search(text, t_max, mode="standard", param=2, collect_gems=False, changes=None):
    key = (text, changes_key(changes), int(t_max), mode, int(param), bool(collect_gems))
    if key not in _CACHE:
        _CACHE[key] = _search(text, int(t_max), mode, int(param), bool(collect_gems), changes)
    return _CACHE[key]


def _search(text, t_max, mode, param, collect_gems, changes=None):
    assert mode in MODES
    world = oracle_world(text, changes)
    A = world.n_agents
    world.reset()
    res = Result(None, None, [1], [])
    root_edges = frozenset(coop_ref.detect(world))
    if not all(world.alive()) or violates(root_edges, mode, param, A):
        return res
    if search_ref.is_goal(world, collect_gems) and accepts(root_edges, mode):
        res.length, res.plan, res.edges = 0, [], set(root_edges)
        return res
    seen = {(search_ref.identity(world, collect_gems), root_edges)}
    frontier, depth = [((), root_edges)], 0
    while depth < t_max and frontier:
        new, expanded, goal = [], 0, None
        for prefix, edges in frontier:
            search_ref.replay(world, prefix)
            for joint in itertools.product(*world.available_actions()):
                expanded += 1
                search_ref.replay(world, prefix)
                world.step(list(joint))
                if not all(world.alive()):
                    continue
                mine = edges | frozenset(coop_ref.detect(world))
                if violates(mine, mode, param, A):
                    continue
                k = (search_ref.identity(world, collect_gems), mine)
                if k in seen:
                    continue
                seen.add(k)
                new.append((prefix + (joint,), mine))
                if goal is None and search_ref.is_goal(world, collect_gems) and accepts(mine, mode):
                    goal = (prefix + (joint,), mine)
        depth += 1
        res.expanded.append(expanded)
        res.frontier.append(len(new))
        if goal is not None:
            res.length, res.plan, res.edges = depth, [list(j) for j in goal[0]], set(goal[1])
            return res
        frontier = new
    return res


def replay_edges(text, plan, changes=None):
    """The flattened help relation of `plan` on a fresh oracle world; asserts that nobody dies.  Returns (edges, world)."""
    world = oracle_world(text, changes)
    world.reset()
    assert all(world.alive())
    edges = set(coop_ref.detect(world))
    for t, joint in enumerate(plan):
        assert len(joint) == world.n_agents
        world.step([int(a) for a in joint])  # raises OracleError when the joint action is refused
        assert all(world.alive()), f"an agent died at step {t}"
        edges |= coop_ref.detect(world)
    return edges, world


def check_plan(text, plan, mode="standard", param=2, collect_gems=False, length=None, changes=None):
    """Replay `plan` (rows of action values) on a fresh oracle world: nobody dies, everybody arrives, and the flattened edges of the
    replay satisfy the mode.  Returns the edges."""
    if length is not None:
        assert len(plan) == length, (len(plan), length)
    edges, world = replay_edges(text, plan, changes)
    assert all(world.arrived()), "not every agent has arrived"
    if collect_gems:
        assert all(world.gems_collected())
    assert not violates(edges, mode, param, world.n_agents), (mode, param, sorted(edges))
    assert accepts(edges, mode), (mode, sorted(edges))
    return edges


# ---------------------------------------------------------------------------------------------- the reference's predicates
def characterize(text, t_max, changes=None):
    """The reference's WorldCharacterizer questions (world_characterization.py) answered with this search: what the golden file states."""
    n_agents = oracle.OracleWorld(text).n_agents
    standard = search(text, t_max, changes=changes)
    solvable = standard.length is not None

    def none(mode, k=2):
        return search(text, t_max, mode, k, changes=changes).length is None

    def asymmetric():
        # (is_asymmetric also asks for a laser colour and for no independent plan: a plan that avoids every edge avoids the asymmetric ones,
        # so "no plan avoids them" implies both)
        return solvable and none("no-asymmetric")

    return dict(solvable=solvable, asymmetric=asymmetric, fully_coupled=lambda: solvable and none("no-fully-coupled"),
                convergent=lambda k: solvable and none("no-convergence", k),
                divergent=lambda k: solvable and k < n_agents and none("no-divergence", k),
                interdependent=lambda n: solvable and none("no-mutual") if n == 2 else None)
