"""The reference's single-world cooperation analysis (python/lle/characterization/plan/) over `lle_amd.World`, which is one
environment on the GPU: `detect_dependencies`, `DependencyEdge`, `TemporalCooperationGraph`, `PlanProfile`, `profile_plan`.

The per-state detection is the coop kernel's (lle_amd.cooperation, liblle_coop.so): one launch and a copy of n_agents words per
call.  The graph queries are host Python over a few dozen edges, written from the definitions in the reference's docstrings:

  * a TRAIL is a sequence of help edges, each starting at the agent the one before ends at, with non-decreasing time stamps, in
    which every temporal edge (helper, beneficiary, t) is used at most once; agents may be revisited;
  * a CLOSED trail of order k ends at the agent it starts from and visits exactly k distinct agents.

`WorldCharacterizer` answers the solver-backed questions -- solvable within t_max, the shortest plan, is cooperation required -- with
the exact shortest-plan search of lle_amd.solver (liblle_search.so) in place of the reference's SAT encoding; the predicates that
need the other solve modes raise here, and `lle_amd.HelpGraphCharacterizer` (lle_amd.helpgraph) answers those over the help graph.  Many worlds at once: `lle_amd.characterize_many` (lle_amd.forest), and the generator's
filter vocabulary over it in lle_amd.generator.  For whole batches use `BatchedLLE(..., cooperation=True)`.
"""
from dataclasses import dataclass
from functools import lru_cache


@dataclass(frozen=True)
class DependencyEdge:
    """`helper` blocks its own laser at state index `t`, which keeps `beneficiary` alive on the beam."""
    helper: int
    beneficiary: int
    t: int


def _tracker(world):
    tracker = getattr(world, "_coop_tracker", None)
    if tracker is None or tracker.world is not world._batch:
        from .cooperation import CooperationTracker
        tracker = world._coop_tracker = CooperationTracker(world._batch)
    return tracker


def detect_dependencies(world):
    """The (helper, beneficiary) edges of the world's current state (analyser.py:31-60): for every enabled source of colour c whose
    beam tiles agent c occupies, c helps every other agent occupying a tile of that source."""
    tracker = _tracker(world)
    tracker.mark()
    return set(tracker.edges(0, "step"))


class TemporalCooperationGraph:
    """Help edges over time.  Self-loops are ignored, duplicates collapsed; `edges` is sorted by (t, helper, beneficiary)."""

    def __init__(self, edges):
        unique = {(int(e.t), int(e.helper), int(e.beneficiary)) for e in edges if e.helper != e.beneficiary}
        self._edges = tuple(DependencyEdge(h, b, t) for t, h, b in sorted(unique))
        self._out = {}  # helper -> indices of its edges, in time order
        for k, e in enumerate(self._edges):
            self._out.setdefault(e.helper, []).append(k)
        self.vertices = sorted({e.helper for e in self._edges} | {e.beneficiary for e in self._edges})

    @staticmethod
    def empty():
        return TemporalCooperationGraph([])

    @staticmethod
    def from_plan(plan, world, reset=True):
        """Replay `plan` (joint actions: an Action or one Action per agent) on `world`, which IS mutated, and record the edges of
        the initial state (t = 0) and of the state after each action (t = 1, 2, ...).  reset=False continues from the current state."""
        if reset:
            world.reset()
        edges = [DependencyEdge(h, b, 0) for h, b in detect_dependencies(world)]
        for t, joint_action in enumerate(plan, start=1):
            world.step(joint_action)
            edges.extend(DependencyEdge(h, b, t) for h, b in detect_dependencies(world))
        return TemporalCooperationGraph(edges)

    @property
    def edges(self):
        return self._edges

    @property
    def n_vertices(self):
        return len(self.vertices)

    @property
    def is_empty(self):
        return not self._edges

    def flattened_edges(self):
        """The (helper, beneficiary) pairs of any time step."""
        return {(e.helper, e.beneficiary) for e in self._edges}

    def max_distinct_helpers(self):
        """The greatest number of distinct helpers of one beneficiary."""
        helpers = {}
        for h, b in self.flattened_edges():
            helpers.setdefault(b, set()).add(h)
        return max((len(v) for v in helpers.values()), default=0)

    def max_distinct_beneficiaries(self):
        """The greatest number of distinct beneficiaries of one helper."""
        beneficiaries = {}
        for h, b in self.flattened_edges():
            beneficiaries.setdefault(h, set()).add(b)
        return max((len(v) for v in beneficiaries.values()), default=0)

    def asymmetric_edges(self):
        """The flattened edges whose helper is never helped by anybody."""
        flat = self.flattened_edges()
        helped = {b for _h, b in flat}
        return {(h, b) for h, b in flat if h not in helped}

    def has_asymmetric_edge(self):
        return bool(self.asymmetric_edges())

    def _next_edges(self, agent, t, used):
        """Indices of the edges that may extend a trail standing at `agent` at time `t` having used `used` (edges of time t)."""
        for k in self._out.get(agent, ()):
            e = self._edges[k]
            if e.t > t or (e.t == t and k not in used):
                yield k

    def longest_trail_length(self):
        """The number of edges of the longest trail.  Of the edges a trail has used, only those of its current time stamp can still
        be met again, so a search state is (agent, time, edges of that time already used)."""
        edges = self._edges

        @lru_cache(maxsize=None)
        def best(agent, t, used):
            longest = 0
            for k in self._next_edges(agent, t, used):
                e = edges[k]
                longest = max(longest, 1 + best(e.beneficiary, e.t, (used | {k}) if e.t == t else frozenset({k})))
            return longest

        if not edges:
            return 0
        before = edges[0].t - 1
        return max(best(a, before, frozenset()) for a in self._out)

    def has_closed_trail_of_order(self, order):
        """Whether some closed trail visits exactly `order` distinct agents."""
        if order < 2 or order > self.n_vertices:
            return False
        edges = self._edges
        before = edges[0].t - 1

        for anchor in self.vertices:
            @lru_cache(maxsize=None)
            def closes(agent, t, used, visited, anchor=anchor):
                for k in self._next_edges(agent, t, used):
                    e = edges[k]
                    seen = visited | {e.beneficiary}
                    if len(seen) > order:
                        continue
                    if e.beneficiary == anchor and len(seen) == order:
                        return True
                    if closes(e.beneficiary, e.t, (used | {k}) if e.t == t else frozenset({k}), seen):
                        return True
                return False

            if closes(anchor, before, frozenset(), frozenset({anchor})):
                return True
        return False

    def profile(self):
        return PlanProfile(self)


class PlanProfile:
    """The cooperation properties of a trajectory (profile.py:4-85)."""

    def __init__(self, graph):
        self.graph = graph

    @property
    def is_independent(self):
        return self.graph.is_empty

    @property
    def is_cooperative(self):
        return not self.graph.is_empty

    @property
    def is_asymmetric(self):
        """Some help edge's helper is never helped."""
        return self.graph.has_asymmetric_edge()

    @property
    def is_mutual(self):
        return self.is_interdependent(2)

    def is_sequential(self, length=2):
        """A trail of at least `length` help edges exists; a sequence has at least 2 edges."""
        if length < 2:
            raise ValueError("A sequence must have at least 2 edges")
        return self.graph.longest_trail_length() >= length

    def is_convergent(self, k=2):
        """One beneficiary is helped by at least k distinct agents."""
        if k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {k}.")
        if k >= self.graph.n_vertices:
            return False
        return self.graph.max_distinct_helpers() >= k

    def is_divergent(self, k=2):
        """One helper helps at least k distinct agents."""
        if k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {k}.")
        if k >= self.graph.n_vertices:
            return False
        return self.graph.max_distinct_beneficiaries() >= k

    def is_interdependent(self, n_agents=2):
        """Some closed trail visits exactly n_agents distinct agents."""
        return self.graph.has_closed_trail_of_order(n_agents)


def profile_plan(world, plan, reset=True):
    """The profile of `plan` on `world` (TemporalCooperationGraph.from_plan says what the arguments mean)."""
    return TemporalCooperationGraph.from_plan(plan, world, reset=reset).profile()


class WorldCharacterizer:
    """Lazy characterisation of a world at the horizon `t_max` (python/lle/characterization/world_characterization.py): every property
    depends on t_max -- a world can require cooperation within 10 steps and have an independent detour of 11.  `world`: an
    lle_amd.World, a Map or map text; `solver_options` (chunk, max_states, device) go to lle_amd.solver.Solver.  Results are cached."""

    def __init__(self, world, t_max, **solver_options):
        from .solver import Solver
        self._solver = Solver(world, t_max, **solver_options)
        self.world = self._solver.world
        self.t_max = self._solver.t_max
        self._results = {}

    def _cached(self, key, compute):
        if key not in self._results:
            self._results[key] = compute()
        return self._results[key]

    @property
    def n_laser_colours(self):
        """Number of distinct agent colours that own a laser source."""
        return self._cached("colours", lambda: len({source.agent_id for source in self.world.laser_sources}))

    @property
    def shortest_path(self):
        """The shortest plan within t_max, or None."""
        return self._cached("standard", lambda: self._solver.find_shortest("standard"))

    @property
    def shortest_independent_path(self):
        """The shortest plan within t_max in which nobody stands on a beam tile of another colour, or None."""
        return self._cached("no-cooperation", lambda: self._solver.find_shortest("no-cooperation"))

    def is_solvable(self):
        return self.shortest_path is not None

    def is_cooperative(self):
        if not self.is_solvable():
            return False
        return self.shortest_independent_path is None

    def is_independent(self):
        if not self.is_solvable():
            return False
        return self.shortest_independent_path is not None

    @staticmethod
    def _needs(mode):
        raise NotImplementedError(f"this predicate needs the solve mode '{mode}', which the search does not build "
                                  "(it serves 'standard' and 'no-cooperation')")

    def is_asymmetric(self):
        self._needs("no-asymmetric")

    def is_fully_coupled(self):
        self._needs("no-fully-coupled")

    def is_sequential(self, length=2):
        if length < 2:
            raise ValueError(f"Sequence length must be >= 2, got {length}.")
        self._needs(f"no-sequence-{length}")

    def is_convergent(self, k=2):
        if k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {k}.")
        self._needs(f"no-convergence-{k}")

    def is_divergent(self, k=2):
        if k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {k}.")
        self._needs(f"no-divergence-{k}")

    def is_interdependent(self, n_agents=2):
        if n_agents < 2:
            raise ValueError(f"Interdependence only makes sense for >= 2 agents. Got {n_agents}.")
        self._needs(f"no-interdependence-{n_agents}")

    def is_mutual(self):
        self._needs("no-mutual")

    def __eq__(self, other):
        return isinstance(other, WorldCharacterizer) and self.world == other.world and self.t_max == other.t_max

    def __hash__(self):
        return hash((self.world, self.t_max))


__all__ = ["profile_plan", "detect_dependencies", "DependencyEdge", "TemporalCooperationGraph", "PlanProfile", "WorldCharacterizer"]
