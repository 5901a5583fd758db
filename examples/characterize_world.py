"""The full cooperation profile of one world: which shapes of cooperation EVERY plan within t_max must show.

`TrailCharacterizer` answers with exact searches on the GPU (liblle_search.so, liblle_helpgraph.so, and liblle_trails.so for
`is_sequential`): a shape is required when the world is solvable and no plan within t_max avoids it.  The world is `paper-fully-coupled` of the reference's layouts catalogue
(python/tests/world_layouts.py): three agents, three lasers, and no way out in which somebody is not helped by everybody else.

    python examples/characterize_world.py [t_max]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAPER_FULLY_COUPLED = """
 @  L0S  @ @ @ @
S0   .   . . @ @
S1   .   . . . @
S2   .   . . . @
 @  L2E  . . . @
 @   @   X X X L1W
"""

PAPER_INTERDEPENDENT_3 = """
 @   S0   @ L2S   S1 @
L0E  .    .   .   .  @
 @   .    @   X   .  @
 @   .    @   .   X L1W
 @   .    @   .   .  @
 @   .    .   X   S2 @
"""


def main():
    from lle_amd import TrailCharacterizer, World
    from lle_amd.characterization import profile_plan
    t_max = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    world = World(PAPER_FULLY_COUPLED)
    c = TrailCharacterizer(world, t_max)  # a HelpGraphCharacterizer that answers is_sequential as well
    plan = c.shortest_path
    print(f"t_max = {t_max}: shortest plan {None if plan is None else len(plan)} steps, shortest independent plan "
          f"{None if c.shortest_independent_path is None else len(c.shortest_independent_path)}")
    if plan is not None:
        graph = profile_plan(World(PAPER_FULLY_COUPLED), plan).graph
        print("help edges of the shortest plan (helper, beneficiary, t):", [(e.helper, e.beneficiary, e.t) for e in graph.edges])
    rows = [("solvable", c.is_solvable()), ("cooperative", c.is_cooperative()), ("independent", c.is_independent()), ("asymmetric", c.is_asymmetric()),
            ("mutual", c.is_mutual()), ("fully coupled", c.is_fully_coupled())]
    rows += [(f"convergent({k})", c.is_convergent(k)) for k in (2, 3)] + [(f"divergent({k})", c.is_divergent(k)) for k in (2, 3)]
    rows += [(f"sequential({n})", c.is_sequential(n)) for n in (2, 3, 4)]
    for name, value in rows:
        print(f"  {name:<16}{value}")
    for name, path in (("non-asymmetric", c.shortest_non_asymmetric_path), ("non-fully-coupled", c.shortest_non_fully_coupled_path),
                       ("without mutual help", c.compute_shortest_non_interdependent_path(2)), ("without 2-convergence", c.compute_shortest_path_without_convergence(2)),
                       ("without 2-divergence", c.compute_shortest_path_without_divergence(2)),
                       ("without a sequence of 2", c.compute_shortest_path_without_sequence(2)),
                       ("without a sequence of 3", c.compute_shortest_path_without_sequence(3))):
        print(f"  shortest plan {name:<26}{'none' if path is None else len(path)}")
    c._solver.free()
    # closed trails over exactly three agents: the reference's headline layout, under CycleCharacterizer
    from lle_amd import CycleCharacterizer
    cc = CycleCharacterizer(World(PAPER_INTERDEPENDENT_3), t_max)
    print(f"paper-interdependent-3, t_max = {t_max}: is_interdependent(2) {cc.is_interdependent(2)}, is_interdependent(3) {cc.is_interdependent(3)}, "
          f"shortest plan without a closed trail over three agents: {'none' if cc.compute_shortest_non_interdependent_path(3) is None else len(cc.compute_shortest_non_interdependent_path(3))}")
    cc._solver.free()


if __name__ == "__main__":
    main()
