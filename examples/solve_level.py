"""The shortest joint plan of level 4 on one MI355X, with and without cooperation.

`Solver.find_shortest` is an exact breadth-first search over joint states in which every successor is computed by the step kernel
(lle_amd/liblle_search.so); `WorldCharacterizer` asks it twice -- any plan, and a plan in which nobody stands in somebody else's beam.
"""
from lle_amd import Solver, World, WorldCharacterizer

world = World.level(4)
solver = Solver(world, t_max=10)
plan = solver.find_shortest()
print(f"level 4: lower bound {solver.solution_lower_bound}, shortest plan {None if plan is None else len(plan)} steps, "
      f"{solver.last_stats['n_states']} states, {sum(solver.last_stats['expanded'])} joint actions expanded")
for t, joint in enumerate(plan or []):
    print(f"  t={t}: " + "  ".join(f"agent {a}: {action.name}" for a, action in enumerate(joint)))

world.reset()                                   # the plan runs on the world it was found for
for joint in plan or []:
    world.step(list(joint))
print("all arrived:", all(agent.has_arrived for agent in world.agents))

c = WorldCharacterizer(world, t_max=10)
print(f"within 10 steps: solvable {c.is_solvable()}, cooperative {c.is_cooperative()}, independent {c.is_independent()}")
