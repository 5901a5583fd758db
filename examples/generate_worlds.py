"""Eight small worlds that cannot be solved without cooperation, generated and filtered on one MI355X.

`generate_n` draws seeded candidate layouts from `lle_amd.mapgen` in batches and keeps those a `Constraint` accepts.  A batch is
filtered by one `Constraint.satisfied_by_many`: two forest runs (lle_amd/liblle_forest.so) that walk the search trees of all its
candidates in the same launches -- any plan, and a plan in which nobody stands in somebody else's beam.
"""
from lle_amd import (Asymmetric, Constraint, Cooperative, CycleCharacterizer, Interdependent, Sequential, Solvable, TrailCharacterizer, characterize_many, generate_n,
                     mapgen, solve_many)

keep = Constraint(t_max=12, predicate=Cooperative(), min_solution_length=4)
worlds = list(generate_n(8, keep, height=5, width=5, n_agents=2, n_lasers=2, n_gems=1, n_exits=2, wall_fraction=0.12, seed=0, batch=128, max_attempts=2048))
print(f"{len(worlds)} cooperative 5x5 worlds whose shortest plan has at least 4 steps")

plans = solve_many(worlds, 12)                       # one forest: the shortest plan of every world
answers = characterize_many(worlds, 12)
for k, (world, plan) in enumerate(zip(worlds, plans)):
    print(f"--- world {k}: shortest plan {len(plan)} steps, cooperative {bool(answers.cooperative[k])}, independent {bool(answers.independent[k])}")
    print(world.world_string.rstrip())
    world.reset()                                    # the plan runs on the world it was found for
    for joint in plan:
        world.step(list(joint))
    assert all(agent.has_arrived for agent in world.agents)

# the same vocabulary composes: solvable without help, in at most 12 steps
easy = Constraint(12, Solvable() & ~Cooperative())
candidates = [mapgen.generate(5, 5, 2, 2, 1, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s) for s in range(64)]
print("of the first 64 candidates,", int(easy.satisfied_by_many(candidates).sum()), "can be solved without cooperation")

# worlds that REQUIRE a shape of cooperation: the help forest (lle_amd/liblle_helpforest.so) answers the atoms over the help graph
lopsided = Constraint(12, Asymmetric() & ~Sequential(3))
worlds = list(generate_n(4, lopsided, characterizer=TrailCharacterizer, height=5, width=5, n_agents=2, n_lasers=2, n_exits=2, wall_fraction=0.12, seed=0,
                         batch=128, max_attempts=1024))
print(f"{len(worlds)} worlds in which somebody must help without being helped, and no chain of three help events is needed")

# worlds that REQUIRE a closed chain of help over three agents: the cycle forest (lle_amd/liblle_cycleforest.so) answers Interdependent(3).
# Random candidates almost never need one -- of the first 256 candidates of the 5x5 generator call below not one does
# (profiles/r19_cycleforest.md), so this generate_n may well come back empty -- which is why the filter is also shown on a batch that holds
# two hand-made 6x6 layouts of the reference's paper among random 6x6 candidates: those two it keeps.
from characterize_world import PAPER_FULLY_COUPLED, PAPER_INTERDEPENDENT_3  # noqa: E402  (examples/characterize_world.py)

chained = Constraint(10, Interdependent(3))
batch = [mapgen.generate(6, 6, 3, 3, 0, n_exits=3, wall_fraction=0.10, n_voids=0, seed=s) for s in range(30)] + [PAPER_INTERDEPENDENT_3, PAPER_FULLY_COUPLED]
kept = chained.satisfied_by_many(batch, characterizer=CycleCharacterizer, envs_per_map=1024)
print(f"of 30 random 6x6 candidates and two hand-made layouts, {int(kept.sum())} cannot be solved within 10 steps without a closed trail of help over all "
      f"three agents: entries {[int(i) for i in kept.nonzero()[0]]}")
worlds = list(generate_n(2, chained, characterizer=CycleCharacterizer, height=5, width=5, n_agents=3, n_lasers=3, n_exits=3, wall_fraction=0.10, seed=0,
                         batch=256, max_attempts=512, envs_per_map=1024))
print(f"{len(worlds)} of 512 random 5x5 candidates need such a chain (none is the expected answer)")
for world in worlds:
    print(world.world_string.rstrip())
