"""lle_amd -- batched, MI355X-native `World.step()` for the Laser Learning Environment.

Drop-in for the hot path of yamoling/lle: `World` (single environment, reference API) and `BatchedWorld`
(tens of thousands of lock-stepped environments per kernel launch, torch tensors over device buffers).
The compute path is hand-written HIP for gfx950 behind the C ABI of include/lle_hip.h; there is no CPU fallback.
"""
from . import exceptions, tiles, types, world  # the reference's submodule paths: lle.tiles, lle.exceptions, lle.types, lle.world
from ._capi import Map, MapParseError
from .world import (Action, Agent, Direction, EventType, Gem, InvalidActionError, InvalidLevelError, InvalidWorldStateError,
                    Laser, LaserSource, ParsingError, World, WorldEvent, WorldState)

__version__ = "0.3.0"  # (round 3 of this build; the reference exposes lle.__version__: python/tests/test_imports.py:35-39)


def __getattr__(name):
    # BatchedWorld imports torch; keep `import lle_amd` light for parse-only users
    if name == "BatchedWorld":
        from .batched import BatchedWorld
        return BatchedWorld
    if name in ("BatchedLLE", "Builder", "DeathStrategy", "level", "from_str", "from_file", "SingleObjective", "MultiObjective", "PotentialShapedLLE",
                "NoExtras", "LaserSubgoal", "MultiGenerator"):  # (lle.level(6).obs_type(...).build())
        from . import env
        return getattr(env, name)
    if name == "CooperationTracker":
        from .cooperation import CooperationTracker
        return CooperationTracker
    if name == "TemporalCooperationTracker":  # (is_sequential / is_mutual for a whole batch, liblle_cooptrails.so)
        from .cooptrails import TemporalCooperationTracker
        return TemporalCooperationTracker
    if name == "ClosedTrailCooperationTracker":  # (is_interdependent(N) for a whole batch, liblle_coopcycles.so)
        from .coopcycles import ClosedTrailCooperationTracker
        return ClosedTrailCooperationTracker
    if name in ("Solver", "solve", "SolveMode", "SolverCapacityError"):  # (lle.solver: the exact shortest-plan search, liblle_search.so)
        from . import solver
        return getattr(solver, name)
    if name in ("OptimalPolicy", "PolicyCapacityError"):  # (steps-to-go and expert actions of a whole batch, liblle_policy.so)
        from . import policy
        return getattr(policy, name)
    if name == "PolicyForest":  # (one steps-to-go table per map of a multi-map batch, one lookup launch, liblle_policyforest.so)
        from .policyforest import PolicyForest
        return PolicyForest
    if name in ("HelpGraphSolver", "HelpGraphCharacterizer"):  # (the solve modes over the help graph, liblle_helpgraph.so)
        from . import helpgraph
        return getattr(helpgraph, name)
    if name in ("TrailSolver", "TrailCharacterizer"):  # (no-sequence-N: trails of help events in time order, liblle_trails.so)
        from . import trails
        return getattr(trails, name)
    if name in ("CycleSolver", "CycleCharacterizer"):  # (no-interdependence-N: closed trails over exactly N agents, liblle_cycles.so)
        from . import cycles
        return getattr(cycles, name)
    if name in ("ForestSolver", "ForestResult", "solve_many", "characterize_many"):  # (the same search over many maps at once, liblle_forest.so)
        from . import forest
        return getattr(forest, name)
    if name in ("HelpForestSolver", "HelpForestResult", "ManyHelpCharacterization"):  # (the help-graph and trail modes over many maps, liblle_helpforest.so)
        from . import helpforest
        return getattr(helpforest, name)
    if name in ("CycleForestSolver", "CycleForestResult", "ManyCycleCharacterization"):  # (no-interdependence-N over many maps, liblle_cycleforest.so)
        from . import cycleforest
        return getattr(cycleforest, name)
    if name in ("Predicate", "Solvable", "Independent", "Cooperative", "Asymmetric", "Sequential", "Convergent", "Divergent", "Interdependent", "And", "Or",
                "Not", "WorldRequirements", "Constraint", "WorldFilter", "generate_n"):  # (lle.generator: the filter vocabulary)
        from . import generator
        return getattr(generator, name)
    if name == "WorldCharacterizer":
        from .characterization import WorldCharacterizer
        return WorldCharacterizer
    if name in ("Layered", "LayeredPadded", "ObservationType", "StateGenerator", "FlattenedLayered", "PartialGenerator",
                "AgentZeroPerspective"):
        from . import observations
        return getattr(observations, name)
    raise AttributeError(name)


__all__ = ["Action", "Agent", "AgentZeroPerspective", "BatchedLLE", "BatchedWorld", "CooperationTracker", "Direction", "EventType", "FlattenedLayered", "Gem", "InvalidActionError", "InvalidLevelError",
           "InvalidWorldStateError", "Laser", "LaserSource", "LaserSubgoal", "Layered", "LayeredPadded", "Map", "MapParseError", "MultiGenerator", "MultiObjective", "NoExtras",
           "ObservationType", "ParsingError", "PartialGenerator", "PotentialShapedLLE", "SingleObjective", "SolveMode", "Solver", "SolverCapacityError", "StateGenerator", "World", "WorldCharacterizer", "WorldEvent", "WorldState", "__version__", "exceptions", "tiles", "solve", "types", "world",
           "ForestSolver", "ForestResult", "solve_many", "characterize_many", "Constraint", "WorldFilter", "generate_n",
           "OptimalPolicy", "PolicyCapacityError", "HelpGraphSolver", "HelpGraphCharacterizer", "TrailSolver", "TrailCharacterizer",
           "HelpForestSolver", "HelpForestResult", "ManyHelpCharacterization", "TemporalCooperationTracker",
           "CycleSolver", "CycleCharacterizer", "CycleForestSolver", "CycleForestResult", "ManyCycleCharacterization",
           "ClosedTrailCooperationTracker", "PolicyForest"]
