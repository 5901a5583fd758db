"""The filter vocabulary of the reference's generator (python/lle/generator/world_filter.py) over the forest search, and a filtered
generator on top of `lle_amd.mapgen`.

A `Predicate` is a value object describing a property of a world at a horizon: the atoms `Solvable`, `Independent`, `Cooperative`
(and the atoms of the solve modes over the help graph, which need a `characterizer`: `Asymmetric`, `Sequential`, `Convergent`,
`Divergent`, `Interdependent`), combined with `&`, `|`, `~` into `And`, `Or`, `Not`.  A `Constraint` adds the horizon `t_max` and an optional
minimum length of the shortest plan:

    keep = Constraint(10, Cooperative() & ~Sequential(3), min_solution_length=4)   # Sequential needs a TrailCharacterizer
    Constraint(10, Cooperative()).is_satisfied_by(world)           # one WorldCharacterizer: two searches of one map
    Constraint(10, Cooperative()).satisfied_by_many(worlds)        # a bool array: two forest runs per shape (lle_amd.forest)
    keep.satisfied_by_many(worlds, characterizer=TrailCharacterizer)   # the help forest (lle_amd.helpforest): a run per atom and shape
    worlds = list(generate_n(100, Constraint(12, Cooperative()), height=5, width=5, n_agents=2, n_lasers=2))

`satisfied_by_many` is new here: the reference filters its candidates one at a time.  Of the reference's generator only the filter
is restated: its placement strategies (lanes, clusters, rooms, laser spans: python/lle/generator/placements.py, candidates.py) are
out of scope, and `generate_n` draws its candidates from the plain rejection sampler `lle_amd.mapgen.generate`.
"""
from dataclasses import dataclass, field

import numpy as np

from .characterization import WorldCharacterizer


@dataclass(frozen=True)
class WorldRequirements:
    """The least a world must have for a predicate to be satisfiable at all (`Cooperative` needs two agents and a laser).  Used to
    refuse impossible requests up front; it does not replace evaluating the predicate."""
    min_lasers: int = 0
    min_agents: int = 1

    def __post_init__(self):
        if self.min_lasers < 0 or self.min_agents < 1:
            raise ValueError(f"requirements must have min_lasers >= 0 and min_agents >= 1, got {self.min_lasers} and {self.min_agents}")

    @staticmethod
    def all(requirements):
        """Of a conjunction: every child must be possible, so the largest of each."""
        rs = list(requirements)
        if not rs:
            return WorldRequirements()
        return WorldRequirements(max(r.min_lasers for r in rs), max(r.min_agents for r in rs))

    @staticmethod
    def any(requirements):
        """Of a disjunction: one child suffices, so the smallest of each."""
        rs = list(requirements)
        if not rs:
            return WorldRequirements()
        return WorldRequirements(min(r.min_lasers for r in rs), min(r.min_agents for r in rs))


class Predicate:
    """A boolean property of a world's characterisation.  `holds(c)` takes anything with WorldCharacterizer's questions."""

    def holds(self, c):
        raise NotImplementedError

    @property
    def requirements(self):
        return WorldRequirements()

    @property
    def cost(self):
        """A static estimate of what evaluating costs; And / Or ask their cheapest child first."""
        return 0

    def __and__(self, other):
        return And(self, other)

    def __or__(self, other):
        return Or(self, other)

    def __invert__(self):
        return Not(self)

    def and_(self, other):
        return self & other

    def or_(self, other):
        return self | other

    def not_(self):
        return ~self

    def and_not(self, other):
        return self & ~other


@dataclass(frozen=True)
class Solvable(Predicate):
    """Some plan of at most t_max steps exists."""

    def holds(self, c):
        return c.is_solvable()


@dataclass(frozen=True)
class Independent(Predicate):
    """Solvable with nobody ever standing in somebody else's beam."""

    def holds(self, c):
        return c.is_independent()

    @property
    def cost(self):
        return 1


@dataclass(frozen=True)
class Cooperative(Predicate):
    """Solvable, and every plan has somebody standing in somebody else's beam."""

    def holds(self, c):
        return c.is_cooperative()

    @property
    def requirements(self):
        return WorldRequirements(min_lasers=1, min_agents=2)

    @property
    def cost(self):
        return 2


@dataclass(frozen=True)
class Asymmetric(Predicate):
    """Some help edge's helper is never helped, in every plan (solve mode 'no-asymmetric': answered by lle_amd.HelpGraphCharacterizer and
    lle_amd.TrailCharacterizer; pass either as `characterizer=` to `satisfied_by_many` / `generate_n` and the help forest answers)."""

    def holds(self, c):
        return c.is_asymmetric()

    @property
    def requirements(self):
        return WorldRequirements(min_lasers=1, min_agents=2)

    @property
    def cost(self):
        return 3


@dataclass(frozen=True)
class Sequential(Predicate):
    """A chain of at least `length` help edges is required (solve mode 'no-sequence-N': answered by lle_amd.TrailCharacterizer; pass it as
    `characterizer=` to `satisfied_by_many` / `generate_n` and the help forest answers)."""
    length: int = 2

    def __post_init__(self):
        if self.length < 2:
            raise ValueError(f"Sequence length must be >= 2, got {self.length}.")

    def holds(self, c):
        return c.is_sequential(self.length)

    @property
    def requirements(self):
        return WorldRequirements(min_lasers=self.length, min_agents=2)

    @property
    def cost(self):
        return 10 + self.length


@dataclass(frozen=True)
class Convergent(Predicate):
    """One agent must be helped by `k` distinct agents (solve mode 'no-convergence-N': answered by lle_amd.HelpGraphCharacterizer and
    lle_amd.TrailCharacterizer; pass either as `characterizer=` to `satisfied_by_many` / `generate_n` and the help forest answers)."""
    k: int

    def __post_init__(self):
        if self.k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {self.k}.")

    def holds(self, c):
        return c.is_convergent(self.k)

    @property
    def requirements(self):
        return WorldRequirements(min_lasers=self.k, min_agents=self.k + 1)

    @property
    def cost(self):
        return 20 + self.k


@dataclass(frozen=True)
class Divergent(Predicate):
    """One agent must help `k` distinct agents (solve mode 'no-divergence-N': answered by lle_amd.HelpGraphCharacterizer and
    lle_amd.TrailCharacterizer; pass either as `characterizer=` to `satisfied_by_many` / `generate_n` and the help forest answers)."""
    k: int = 2

    def __post_init__(self):
        if self.k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {self.k}.")

    def holds(self, c):
        return c.is_divergent(self.k)

    @property
    def requirements(self):
        return WorldRequirements(min_lasers=1, min_agents=self.k + 1)

    @property
    def cost(self):
        return 20 + self.k


@dataclass(frozen=True)
class Interdependent(Predicate):
    """A closed chain of help over `order` agents is required (solve mode 'no-interdependence-N': order 2 is 'no-mutual', answered like
    `Asymmetric`; N >= 3 is answered by lle_amd.CycleCharacterizer: pass it as `characterizer=` to `is_satisfied_by`, or to
    `satisfied_by_many` / `generate_n`, where the cycle forest answers for many worlds at once)."""
    order: int = 2

    def __post_init__(self):
        if self.order < 2:
            raise ValueError(f"Dependency order must be >= 2, got {self.order}.")

    def holds(self, c):
        return c.is_interdependent(self.order)

    @property
    def requirements(self):
        return WorldRequirements(min_lasers=self.order, min_agents=self.order)

    @property
    def cost(self):
        return 20 + self.order


def _flatten(children, cls):
    flat = []
    for child in children:
        if not isinstance(child, Predicate):
            raise TypeError(f"Expected Predicate, got {type(child).__name__}.")
        flat.extend(child.children if isinstance(child, cls) else (child,))
    return tuple(flat)


class _Junction(Predicate):
    """Children of the same kind are flattened into one node; evaluation asks the cheapest child first (ties keep their order)."""

    def __init__(self, *children):
        object.__setattr__(self, "children", _flatten(children, type(self)))

    @property
    def cost(self):
        return sum(p.cost for p in self.children)

    def ordered(self):
        return tuple(sorted(self.children, key=lambda p: p.cost))


@dataclass(frozen=True, init=False)
class And(_Junction):
    children: tuple

    def holds(self, c):
        return all(p.holds(c) for p in self.ordered())

    @property
    def requirements(self):
        return WorldRequirements.all(p.requirements for p in self.children)


@dataclass(frozen=True, init=False)
class Or(_Junction):
    children: tuple

    def holds(self, c):
        return any(p.holds(c) for p in self.ordered())

    @property
    def requirements(self):
        return WorldRequirements.any(p.requirements for p in self.children)


@dataclass(frozen=True)
class Not(Predicate):
    inner: Predicate

    def __post_init__(self):
        if not isinstance(self.inner, Predicate):
            raise TypeError(f"Expected Predicate, got {type(self.inner).__name__}.")

    def holds(self, c):
        return not self.inner.holds(c)

    @property
    def cost(self):
        return self.inner.cost


class _Answered(WorldCharacterizer):
    """Entry i of a ManyCharacterization behind WorldCharacterizer's questions (the unbuilt ones raise as they do there)."""

    def __init__(self, many, i, world=None):  # (no Solver: the searches have run)
        self._many, self._i = many, i
        self.world, self.t_max = world, many.t_max

    @property
    def shortest_path(self):
        return self._many.shortest_paths[self._i]

    @property
    def shortest_independent_path(self):
        return self._many.shortest_independent_paths[self._i]


@dataclass(frozen=True)
class Constraint:
    """A predicate, the horizon `t_max` at which it is evaluated, and optionally the least length of the shortest plan."""
    t_max: int
    predicate: Predicate = field(default_factory=Solvable)
    min_solution_length: object = None

    def __post_init__(self):
        if not isinstance(self.predicate, Predicate):
            raise TypeError(f"Expected Predicate, got {type(self.predicate).__name__}.")
        if int(self.t_max) < 0:
            raise ValueError(f"t_max must be non-negative, got {self.t_max}.")

    @property
    def requirements(self):
        return self.predicate.requirements

    def _accepts(self, c):
        if self.min_solution_length is not None:
            path = c.shortest_path
            if path is None or len(path) < self.min_solution_length:
                return False
        return bool(self.predicate.holds(c))

    def is_satisfied_by(self, world, *, characterizer=WorldCharacterizer, **solver_options):
        """Whether `world` satisfies the constraint: one `characterizer` (`solver_options` go to its Solver).  WorldCharacterizer
        answers Solvable / Independent / Cooperative; lle_amd.HelpGraphCharacterizer also Asymmetric, Convergent, Divergent and
        Interdependent(2); lle_amd.TrailCharacterizer also Sequential(N); lle_amd.CycleCharacterizer also Interdependent(N) for N >= 3."""
        return self._accepts(characterizer(world, self.t_max, **solver_options))

    def satisfied_by_many(self, worlds, *, characterizer=None, **options):
        """A bool array, entry i == is_satisfied_by(worlds[i], characterizer=characterizer), searched together: the worlds are grouped
        by shape and every group is one forest (`options`: envs_per_map, max_states_per_map, device).  `characterizer` None: the
        plain forest (`lle_amd.forest.characterize_many`), which answers Solvable / Independent / Cooperative.
        lle_amd.HelpGraphCharacterizer or lle_amd.TrailCharacterizer: the help forest (`lle_amd.helpforest.characterize_many`),
        which also answers Asymmetric, Convergent, Divergent, Interdependent(2) and -- under TrailCharacterizer -- Sequential(N); every
        atom costs at most one forest run per shape, made when the first world needs it.  lle_amd.CycleCharacterizer: the cycle forest
        (`lle_amd.cycleforest.characterize_many`), which answers all of those and Interdependent(N) for N >= 3 -- unless `options`
        holds a key of the single solver (`chunk`, `max_states`): then, and for any other class, one such characterizer per world
        (`options` go to its Solver)."""
        worlds = list(worlds)
        if characterizer is None:
            from .forest import characterize_many
            many = characterize_many(worlds, self.t_max, **options)
            return np.array([self._accepts(_Answered(many, i)) for i in range(len(worlds))], dtype=bool)
        from .helpgraph import HelpGraphCharacterizer
        from .trails import TrailCharacterizer
        if characterizer in (HelpGraphCharacterizer, TrailCharacterizer):
            from . import helpforest
            with helpforest.characterize_many(worlds, self.t_max, sequential=characterizer is TrailCharacterizer, **options) as many:
                return np.array([self._accepts(many.entry(i)) for i in range(len(worlds))], dtype=bool)
        from .cycles import CycleCharacterizer
        if characterizer is CycleCharacterizer and not {"chunk", "max_states"} & set(options):
            from . import cycleforest
            with cycleforest.characterize_many(worlds, self.t_max, **options) as many:
                return np.array([self._accepts(many.entry(i)) for i in range(len(worlds))], dtype=bool)
        return np.array([self.is_satisfied_by(w, characterizer=characterizer, **options) for w in worlds], dtype=bool)


WorldFilter = Constraint  # the reference's earlier name


def generate_n(n, constraint, *, height, width, n_agents, n_lasers=0, n_gems=0, n_exits=None, wall_fraction=0.10, n_voids=0, seed=0, batch=256,
               max_attempts=None, **options):
    """Yield up to `n` Worlds that satisfy `constraint`, in candidate order: candidate i is
    `mapgen.generate(height, width, n_agents, n_lasers, n_gems, n_exits, wall_fraction, n_voids, seed=seed + i)` for i = 0, 1, ...;
    candidates are drawn `batch` at a time and every batch is filtered by one `constraint.satisfied_by_many` (`options` go there:
    envs_per_map, max_states_per_map, device -- and `characterizer=lle_amd.TrailCharacterizer` or `lle_amd.HelpGraphCharacterizer`
    for constraints over Asymmetric, Sequential, Convergent, Divergent or Interdependent(2), which the help forest then answers;
    `characterizer=lle_amd.CycleCharacterizer` for Interdependent(N) with N >= 3, which the cycle forest answers).  The
    worlds that come out depend on the arguments only, not on `batch`.  Stops after `n` accepted worlds or `max_attempts` candidates
    (None: no limit -- a constraint nothing satisfies then never ends).

    The candidates come from a plain rejection sampler: the reference's placement strategies (lanes, clusters, rooms, laser spans) are
    out of scope."""
    if not isinstance(constraint, Constraint):
        raise TypeError(f"Expected Constraint, got {type(constraint).__name__}.")
    n, batch = int(n), int(batch)
    if n < 0:
        raise ValueError(f"n must be non-negative, got {n}.")
    if batch < 1:
        raise ValueError(f"batch must be at least 1, got {batch}.")
    if max_attempts is not None and int(max_attempts) < 0:
        raise ValueError(f"max_attempts must be non-negative, got {max_attempts}.")
    need = constraint.requirements
    if n_agents < need.min_agents:
        raise ValueError(f"the constraint needs at least {need.min_agents} agents, got n_agents={n_agents}.")
    if n_lasers < need.min_lasers:
        raise ValueError(f"the constraint needs at least {need.min_lasers} lasers, got n_lasers={n_lasers}.")

    def candidates():
        from . import mapgen
        from .world import World
        accepted, drawn = 0, 0
        while accepted < n and (max_attempts is None or drawn < int(max_attempts)):
            count = batch if max_attempts is None else min(batch, int(max_attempts) - drawn)
            worlds = [World(mapgen.generate(height, width, n_agents, n_lasers, n_gems, n_exits=n_exits, wall_fraction=wall_fraction, n_voids=n_voids,
                                            seed=seed + drawn + k)) for k in range(count)]
            drawn += count
            for world, keep in zip(worlds, constraint.satisfied_by_many(worlds, **options)):
                if keep and accepted < n:
                    accepted += 1
                    yield world

    return candidates()


__all__ = ["Predicate", "Solvable", "Independent", "Cooperative", "Asymmetric", "Sequential", "Convergent", "Divergent", "Interdependent", "And", "Or", "Not",
           "WorldRequirements", "Constraint", "WorldFilter", "generate_n"]
