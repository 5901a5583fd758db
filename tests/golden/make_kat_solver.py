"""Hand transcription of the reference's solver and characterisation expectations as data; running it rewrites kat_solver.json.

`catalogue` restates python/tests/world_layouts.py: every layout that states `solvable`, `cooperative` or `independent` (level-5 and
level-6 left out), with the map text (or the level number) and, per t_max, those three fields where the reference gives them --
`expect()` there derives `independent` from `cooperative` and the other way round (world_layouts.py:124-129), so both are written.
Every other property of a layout is left out.  `solver` restates python/tests/solver/test_solver.py: the plan lengths it asserts and
its solvable / unsolvable maps; `lower_bounds` restates src/unit_tests/test_context.rs:256-282.  Nothing here imports or executes the
reference; only inputs and expected outputs are kept.
"""
import json
import os

LAYOUTS = "python/tests/world_layouts.py"
SOLVER = "python/tests/solver/test_solver.py"
CONTEXT = "src/unit_tests/test_context.rs"


def expect_for(horizons, **fields):
    """{t_max: fields} with cooperative / independent completed from each other."""
    if "cooperative" in fields and "independent" not in fields:
        fields["independent"] = not fields["cooperative"]
    elif "independent" in fields and "cooperative" not in fields:
        fields["cooperative"] = not fields["independent"]
    return {str(t): dict(fields) for t in horizons}


def layout(name, ref, source, *expectations):
    by_t_max = {}
    for e in expectations:
        by_t_max.update(e)
    case = dict(name=name, ref=f"{LAYOUTS}:{ref}", expect=by_t_max)
    case["level" if isinstance(source, int) else "map"] = source
    return case


CATALOGUE = [
    layout("level-1", "179-183", 1, expect_for([10], solvable=True, cooperative=False)),
    layout("level-2", "185-189", 2, expect_for([10], cooperative=False)),
    layout("level-3", "191-198", 3, expect_for(range(10), solvable=False), expect_for(range(10, 20), cooperative=True)),
    layout("level-4", "200-204", 4, expect_for([10], cooperative=True)),
    layout("blocked-unsolvable", "238-242", "S0 @ X", expect_for([10], solvable=False)),
    layout("unsolvable-4agents", "244-248", "S0 S1 S2 S3 X X X X", expect_for([10], solvable=False)),
    layout("open-two-agent", "250-270", """
S0 . S1
 . . .
 X . X
""", expect_for([6], solvable=True, cooperative=False)),
    layout("open-two-agent-wide", "272-281", """
 . . . . X
S0 . . . .
S1 . . . .
 . . . . X
""", expect_for([10], solvable=True, cooperative=False)),
    layout("one-way-detour", "284-314", """
 .  . S0 S1 . .
L0E .  .  . @ .
 .  .  .  . . .
 .  .  .  . . .
 X  X  .  . . .
""", expect_for(range(6, 10), solvable=True, cooperative=True), expect_for(range(10, 12), solvable=True, cooperative=False)),
    layout("single-laser-asymmetric", "316-335", """
 @  S0 S1
L0E .  .
 @  X  X
""", expect_for([6], solvable=True, cooperative=True)),
    layout("convergent-2-tight", "347-367", """
 @  S0  @  @  @  S2
L0E  .  .  .  .  .
 @   X  @  @  @  .
L1E  .  .  .  .  .
 @  S1  @  @  @  .
 @   X  @  @  @  X
""", expect_for([5], solvable=True, cooperative=True)),
    layout("divergent-2-with-detour", "389-403", """
 @   X   X   X  @   X
L0E  .   .   .  @   .
 @  S0  S1  S2  @   .
 @   @   @   .   .  .
""", expect_for([2, 5, 6, 8], solvable=True, cooperative=True)),
    layout("sequence-4-with-mutual", "405-424", """
 @  S0 S1  @
L0E X  .   @
 @  S2 .   @
 @  .  X  L1W
 @  .  S3  @
L2E .  .   @
 @  X  X  L3W
""", expect_for([6], solvable=True)),
    layout("sequence-3-without-cycle", "426-445", """
 @  S0 S1  @
L0E X  .   @
 @  S2 .   @
 @  .  X  L1W
 @  .  S3  @
L2E X  .   @
 @  .  X   @
""", expect_for([6], solvable=True)),
    layout("paper-sequence-2", "447-465", """
 @  S0 @ S1 @
L0E .  . .  @
 @  X  @ . S2
 @ L1E . .  .
 @  @  @ X  x
""", expect_for([10], solvable=True)),
    layout("paper-sequence-2-not-interdependent-3", "467-486", """
 @  S0 @  @  L1S S1
L0E .  .  .   .  .
 @  . S2 L2W  .  X
 @  .  .  .   .  X
L0E .  @  .   .  .
 @  X  @  .   .  .
""", expect_for([10], solvable=True)),
    layout("paper-convergent-2", "488-508", """
 @   S0  .  S2  .
L0E  .   .  .   @
 @   X   @  .   .
 @  L1E  .  S1  .
 @   @   @  X   X
""", expect_for([10], solvable=True)),
    layout("paper-fully-coupled", "510-533", """
 @  L0S  @ @ @ @
S0   .   . . @ @
S1   .   . . . @
S2   .   . . . @
 @  L2E  . . . @
 @   @   X X X L1W
""", expect_for([10], solvable=True, cooperative=True, independent=False)),
    layout("paper-fully-coupled-legacy", "535-556", """
 .  S0 S1 S2 .
L0E .  .  .  .
 .  .  .  . L2W
L1E .  .  .  .
 .  X  X  X  .
""", expect_for([10], solvable=True, cooperative=True, independent=False)),
    layout("two-agent-mutual-with-detours", "587-635", """
 .  . . S0 S1  .  . . .
L0E . .  .  .  @  @ @ .
 .  . @  .  . L1W . . .
 .  . .  .  .  .  . . .
 .  . .  X  X  .  . . .
""", expect_for(range(5, 12), solvable=True, cooperative=True, independent=False),
           expect_for(range(12, 15), solvable=True, cooperative=False, independent=True)),
    layout("two-agent-mutual-reversed", "637-647", """
 .  . . S1 S0  .  . . .
L1E . .  .  .  @  @ @ .
 .  . @  .  . L0W . . .
 .  . .  .  .  .  . . .
 .  . .  X  X  .  . . .
""", expect_for([6], solvable=True, cooperative=True)),
    layout("temporal-flattening-counterexample", "649-699", """
 @  @  L1S @ L3S  @   @
 @  S0 S1  @ S3  S2   @
L0E .   .  @  .   .  L2W
 @  .   X  @  X   .   @
 @  .   .  .  .   .   @
 @ L2E  X  @  X  L0W  @
""", expect_for([20], cooperative=True)),
    layout("three-agent-temporal-cycle", "701-717", """
 @ L0S L2S L1S .
S0  .   .   .  X
S1  .   .   .  X
S2  .   .   .  X
""", expect_for([15], solvable=True)),
    layout("three-agent-with-two-agent-cycle", "719-737", """
 .  S1  S0 S2 @ @
 . L0E  .  .  @ @
 .  .  L1W .  . .
 @  .   .  @  . .
L2E .   .  .  . .
 @  @   .  X  X X
""", expect_for([16], solvable=True)),
    layout("paper-interdependent-3", "739-759", """
 @   S0   @ L2S   S1 @
L0E  .    .   .   .  @
 @   .    @   X   .  @
 @   .    @   .   X L1W
 @   .    @   .   .  @
 @   .    .   X   S2 @
""", expect_for([10], solvable=True)),
    layout("four-agent-interdependent-4-sequence-6", "761-785", """
@   S0  S1 @   @
@   .   .  L1W @
L0E .   .  L1S @
@   X   .  .   @
@   L2S .  .   S2
@   X   .  @   @
S3  .   .  .   @
@   L3E .  .   @
@   @   .  .   L1W
@   @   X  X   @
""", expect_for([14], solvable=True)),
]

LINE = "S0 . . X"
SOLVER_CASES = dict(
    lengths=[
        dict(name="solve_simple_world_returns_shortest_plan", ref=f"{SOLVER}:21-27", map=LINE, t_max=15, call="solve", path_length=3, length=3),
        dict(name="solve_fixed_length", ref=f"{SOLVER}:30-34", map=LINE, t_max=5, call="solve", path_length="auto", length=5),
        dict(name="find_shortest_uses_the_heuristic_lower_bound", ref=f"{SOLVER}:37-40", map=LINE, t_max=5, call="find_shortest", t_min=None, length=3),
        dict(name="find_shortest_honours_t_min", ref=f"{SOLVER}:43-46", map=LINE, t_max=5, call="find_shortest", t_min=4, length=4),
        dict(name="solve_default_t_max", ref=f"{SOLVER}:59-65", map="S0 .\n.  X", t_max="auto", call="solve", path_length="auto", length=2),
        dict(name="solve_plan_is_executable", ref=f"{SOLVER}:68-75", map=LINE, t_max=4, call="solve", path_length="auto", length=4),
    ],
    value_errors=[
        dict(name="find_shortest_rejects_t_min_above_t_max", ref=f"{SOLVER}:49-51", map=LINE, t_max=5, call="find_shortest", t_min=6,
             match="exceeds this solver's t_max"),
        dict(name="solver_override_t_max_cannot_exceed_construction_bound", ref=f"{SOLVER}:153-156", map=LINE, t_max=5, call="solve", path_length=6,
             match="exceeds this solver's t_max"),
    ],
    solvable=[
        dict(name="solve_path_is_executable_2agents", ref=f"{SOLVER}:78-90", t_max=10, solvable=True, map="""
@  @ L1S @ X
S0 .  .  . .
S1 .  .  . .
@  @  .  @ X
"""),
        dict(name="not_solvable", ref=f"{SOLVER}:103-114", t_max=10, solvable=False, map="""
 @ L1S  .  @
S0  .   .  X
S1  .   .  X
 @  .  L1N @"""),
        dict(name="two_same_colour_lasers_blocking_distinct_routes_is_unsat", ref=f"{SOLVER}:117-125", t_max=6, solvable=False, map="""
L0S @  L0S @ S0
 X  S1  X  @ X
"""),
        dict(name="two_same_colour_same_direction_lasers_with_clear_lanes_is_solvable", ref=f"{SOLVER}:128-134", t_max=4, solvable=True, map="""
S1 L0S L0S S0
.  .   .   .
X  X   .   .
"""),
        dict(name="two_same_colour_crossing_lasers_keep_independent_beams", ref=f"{SOLVER}:137-150", t_max=6, solvable=True, map="""
.   L0S L0S L0S X
L0E .   .   .   .
S0  .   .   .   .
S1  .   .   .   L0N
.   .   .   .   X
"""),
    ],
    collect_gems=[
        dict(name="collect_gems_is_per_solve_call", ref=f"{SOLVER}:159-163", map="S0 G X", t_max=2, solvable=True, solvable_with_gems=True),
    ],
)

LOWER_BOUNDS = [
    dict(name="lower_bound_uses_walkable_shortest_path", ref=f"{CONTEXT}:256-262", map="S0 @ X\n. . .\n. . .", bound=4),
    dict(name="lower_bound_empty_world", ref=f"{CONTEXT}:264-271", map="S0 . . . . . . . . . . X", bound=11),
    dict(name="lower_bound_with_wall", ref=f"{CONTEXT}:273-282", map="S0 @ . . . . . X\n . . . . . . . .", bound=9,
         note="the reference asserts width + 1 with width = the 8 cells of the second line"),
]


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_solver.json")
    with open(out, "w") as f:
        json.dump(dict(catalogue=CATALOGUE, solver=SOLVER_CASES, lower_bounds=LOWER_BOUNDS), f, indent=1)
        f.write("\n")
    n = sum(len(c["expect"]) for c in CATALOGUE)
    print(f"{len(CATALOGUE)} layouts with {n} horizons, {sum(len(v) for v in SOLVER_CASES.values())} solver cases, {len(LOWER_BOUNDS)} bounds -> {out}")
