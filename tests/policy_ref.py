"""The steps-to-go table of liblle_policy.so restated over `oracle.OracleWorld`, without a GPU.

Exploration is the level-by-level walk of tests/search_ref.py (its `identity`, `is_goal` and `replay`) that does not stop at a goal:
it runs until the frontier is empty (`complete`) or `horizon` levels are expanded, and keeps the depth of every state.  Successors with
a dead agent are dropped.  The edges of every expanded state are kept explicitly -- (joint-action code, successor) for every available
joint action whose successor is a stored state -- and relaxed backwards from the goal states to the fixpoint: the shortest distance in
the explored graph.  A state's action is the smallest (steps, code) pair over its edges; `code` is the joint action in base 5, agent 0
the lowest digit.

Exactness: a value of state s is exact iff the table is complete or depth[s] + steps <= horizon (a shorter true path would lie wholly
among expanded states).  A state without a plan is DEAD_END when the table is complete; everything else that is not exact is UNKNOWN.

Results are cached per (map, horizon, collect_gems): the CPU and the GPU tests share one computation.
"""
import itertools
from dataclasses import dataclass, field

from oracle import oracle
from tests.search_ref import identity, is_goal, replay

UNKNOWN, DEAD_END = -1, -2
STAY = 4


def code_of(joint):
    return sum(int(a) * 5 ** k for k, a in enumerate(joint))


def joint_of(code, n_agents):
    return [(code // 5 ** k) % 5 for k in range(n_agents)]


@dataclass
class State:
    key: tuple          # identity
    prefix: tuple       # joint actions from the reset state
    depth: int
    positions: list     # [(i, j)] per agent
    gems: list          # collected flags
    goal: bool
    edges: list = field(default_factory=list)  # (code, successor index) of every available joint action whose successor is stored
    steps: object = None                       # shortest distance to a goal in the explored graph, None: no plan known
    code: int = 0


@dataclass
class Table:
    text: str
    horizon: int
    collect_gems: bool
    n_agents: int
    states: list
    frontier: list      # states first reached at depth d
    expanded: list      # available joint actions over the states of depth d, for the depths that were expanded
    complete: bool

    @property
    def n_states(self):
        return len(self.states)

    @property
    def depth_reached(self):
        return len(self.expanded)

    def answer(self, s):
        """(steps or UNKNOWN or DEAD_END, code) a lookup gives for state `s`; negative answers come with the all-STAY code."""
        stay = code_of([STAY] * self.n_agents)
        if s.steps is None:
            return (DEAD_END if self.complete else UNKNOWN), stay
        if self.complete or s.depth + s.steps <= self.horizon:
            return s.steps, s.code
        return UNKNOWN, stay

    @property
    def table(self):
        """{identity: (steps or UNKNOWN or DEAD_END, code, depth)}"""
        return {s.key: self.answer(s) + (s.depth,) for s in self.states}

    @property
    def root_steps(self):
        steps = self.answer(self.states[0])[0]
        return steps if steps >= 0 else None

    def kinds(self):
        """(exact, no plan known, plan known but beyond the horizon) state counts."""
        exact = sum(self.answer(s)[0] >= 0 for s in self.states)
        no_plan = sum(s.steps is None for s in self.states)
        return exact, no_plan, len(self.states) - exact - no_plan


_CACHE = {}


def build(text, horizon, collect_gems=False):
    key = (text, int(horizon), bool(collect_gems))
    if key not in _CACHE:
        _CACHE[key] = _build(text, int(horizon), bool(collect_gems))
    return _CACHE[key]


def _build(text, horizon, collect_gems):
    world = oracle.OracleWorld(text)

    def state_here(prefix, depth):
        return State(identity(world, collect_gems), prefix, depth, [tuple(p) for p in world.positions()], list(world.gems_collected()),
                     is_goal(world, collect_gems))

    world.reset()
    states = [state_here((), 0)]
    index = {states[0].key: 0}
    frontier, expanded = [1], []
    level, depth = [0], 0
    while depth < horizon and level:
        new, count = [], 0
        for si in level:
            s = states[si]
            replay(world, s.prefix)
            for joint in itertools.product(*world.available_actions()):
                count += 1
                replay(world, s.prefix)
                world.step(list(joint))  # (an available joint action is never refused: OracleError would fail the caller)
                if not all(world.alive()):
                    continue
                k = identity(world, collect_gems)
                if k not in index:
                    index[k] = len(states)
                    states.append(state_here(s.prefix + (tuple(joint),), depth + 1))
                    new.append(index[k])
                s.edges.append((code_of(joint), index[k]))
        depth += 1
        expanded.append(count)
        frontier.append(len(new))
        level = new
    # ---- backward relaxation to the fixpoint
    stay = code_of([STAY] * world.n_agents)
    for s in states:
        if s.goal:
            s.steps, s.code = 0, stay
    changed = True
    while changed:
        changed = False
        for s in reversed(states):
            for code, t in s.edges:
                if states[t].steps is None:
                    continue
                cand = (states[t].steps + 1, code)
                if s.steps is None or cand < (s.steps, s.code):
                    s.steps, s.code = cand
                    changed = True
    return Table(text, horizon, collect_gems, world.n_agents, states, frontier, expanded, complete=not level)


def rows():
    """The maps and horizons the policy tests share: (name, map text, horizon, collect_gems)."""
    from tests import search_ref, test_gpu_solver as tgs
    catalogue = {c["name"]: c for c in search_ref.load_cases()["catalogue"]}
    text = lambda name: search_ref.map_text(catalogue[name])  # noqa: E731
    return [("line", "S0 . . X", 10, False), ("single-laser-asymmetric", text("single-laser-asymmetric"), 30, False),
            ("one-way-detour", text("one-way-detour"), 40, False), ("one-way-detour-h7", text("one-way-detour"), 7, False),
            ("termination-exhausted", tgs.TERMINATION_EXHAUSTED, 30, False), ("exit-freezes", "S0 . S1 . X X", 12, False),
            ("five-lanes", tgs.FIVE_LANES, 8, False), ("long-beam", tgs.LONG_BEAM, 8, False), ("gems-collect", tgs.GEMS, 12, True),
            ("gems", tgs.GEMS, 12, False), ("open-two-agent", text("open-two-agent"), 20, False)]
