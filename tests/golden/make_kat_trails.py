"""Hand transcription of the reference's `sequential` expectations as data; running it rewrites kat_trails.json.

`catalogue` restates python/tests/world_layouts.py for every layout that states `sequential={...}`: the map text (`level`: the number
of a built-in level instead) and, per t_max, the stated booleans by length.  Every other stated field is left out (they are in
kat_solver.json and kat_helpgraph.json; `interdependent[>= 3]` is not built).  Nothing here imports or executes the reference; only
inputs and expected outputs are kept.

`maps` are the maps that are not in the catalogue: five of tests/golden/kat_helpgraph.json, repeated here so that this file stands
alone (`two-agent-mutual-compact` is the reference's, `three-beam-cell`, `gem-detour`, `six-mutual` and `six-converge` this
project's), and four made for the trail search:
  long-trails         two-agent-mutual-compact without reachable exits: no plan under any N, trails up to 15 edges, a frontier that
                      runs empty at depth N + 5
  chain-in-one-state  agent 1 has to stand on the crossing of L0E and its own L1S while agent 2 crosses L1S below it: 0 -> 1 and 1 -> 2
                      in ONE state, a trail of two edges from one layer
  chain-at-reset      the same crossing with everybody standing there at the start: the reset state (t = 0) holds the trail already,
                      so no-sequence-2 rejects the reset state itself
  decreasing-times    agent 2 has to cross L1S while agent 1 still stands at its top (1 -> 2), and only afterwards can agent 1 walk down
                      through L0E behind agent 0 (0 -> 1): the flattened relation chains 0 -> 1 -> 2, the times do not, and the longest
                      trail of the shortest plan has ONE edge

`searches` are the searches the GPU tests run, one per (map, t_max, n, collect_gems): `length` (null: no plan), `states` (distinct
(world state, trail lengths) records stored), `frontier` and `expanded` per depth, all worked out with tests/trails_ref.py
(tests/test_trails_cpu.py holds it to every entry here).  A search may carry a `changes` key: what is done to the world of the map text
BEFORE the search is set up, as plain data in the form of tests/golden/kat_helpgraph.json (tests/helpgraph_ref.py: `oracle_world`,
`apply_changes`) -- {"sources": [{"laser_id": l, "enabled": false | true | null, "colour": c | null}, ...]}.

What the searches find against what the reference states -- every stated value is reproduced by tests/trails_ref.py (where it
finishes in test time) and by liblle_trails.so, with no contradiction.  Left out of the GPU comparison, by name:
  level-6   at t_max 21 the pool of 4 194 304 records overflows, as the plain search does at depth 11.
Left out of the comparison with the restatement (tests/test_trails_cpu.py: BEYOND_THE_RESTATEMENT says which and why); they are held
to their stated values on the GPU.
"""
import json
import os

LAYOUTS = "python/tests/world_layouts.py"


def expect_for(horizons, sequential):
    return {str(t): {"sequential": {str(k): v for k, v in sequential.items()}} for t in horizons}


def layout(name, ref, text, *expectations):
    by_t_max = {}
    for e in expectations:
        by_t_max.update(e)
    out = dict(name=name, ref=f"{LAYOUTS}:{ref}", expect=by_t_max)
    out["level" if isinstance(text, int) else "map"] = text
    return out


CATALOGUE = [
    layout("level-6", "216-233", 6, expect_for([21], {2: True, 3: False})),
    layout("one-way-detour", "284-314", """
 .  . S0 S1 . .
L0E .  .  . @ .
 .  .  .  . . .
 .  .  .  . . .
 X  X  .  . . .
""", expect_for(range(6, 12), {2: False, 3: False})),
    layout("single-laser-asymmetric", "316-335", """
 @  S0 S1
L0E .  .
 @  X  X
""", expect_for([6], {2: False})),
    layout("sequence-4-with-mutual", "405-424", """
 @  S0 S1  @
L0E X  .   @
 @  S2 .   @
 @  .  X  L1W
 @  .  S3  @
L2E .  .   @
 @  X  X  L3W
""", expect_for([6], {2: True, 3: True, 4: True, 5: False})),
    layout("sequence-3-without-cycle", "426-445", """
 @  S0 S1  @
L0E X  .   @
 @  S2 .   @
 @  .  X  L1W
 @  .  S3  @
L2E X  .   @
 @  .  X   @
""", expect_for([6], {2: True, 3: True, 4: False})),
    layout("paper-sequence-2", "447-465", """
 @  S0 @ S1 @
L0E .  . .  @
 @  X  @ . S2
 @ L1E . .  .
 @  @  @ X  x
""", expect_for([10], {2: True, 3: False})),
    layout("paper-sequence-2-not-interdependent-3", "467-486", """
 @  S0 @  @  L1S S1
L0E .  .  .   .  .
 @  . S2 L2W  .  X
 @  .  .  .   .  X
L0E .  @  .   .  .
 @  X  @  .   .  .
""", expect_for([10], {2: True, 3: False})),
    layout("paper-convergent-2", "488-508", """
 @   S0  .  S2  .
L0E  .   .  .   @
 @   X   @  .   .
 @  L1E  .  S1  .
 @   @   @  X   X
""", expect_for([10], {2: False})),
    layout("two-agent-mutual-with-detours", "587-635", """
 .  . . S0 S1  .  . . .
L0E . .  .  .  @  @ @ .
 .  . @  .  . L1W . . .
 .  . .  .  .  .  . . .
 .  . .  X  X  .  . . .
""", expect_for([6], {2: True, 3: False})),
    layout("temporal-flattening-counterexample", "649-699", """
 @  @  L1S @ L3S  @   @
 @  S0 S1  @ S3  S2   @
L0E .   .  @  .   .  L2W
 @  .   X  @  X   .   @
 @  .   .  .  .   .   @
 @ L2E  X  @  X  L0W  @
""", expect_for([20], {2: True, 3: False})),
    layout("three-agent-temporal-cycle", "701-717", """
 @ L0S L2S L1S .
S0  .   .   .  X
S1  .   .   .  X
S2  .   .   .  X
""", expect_for([15], {2: True, 3: True, 4: False})),
    layout("three-agent-with-two-agent-cycle", "719-737", """
 .  S1  S0 S2 @ @
 . L0E  .  .  @ @
 .  .  L1W .  . .
 @  .   .  @  . .
L2E .   .  .  . .
 @  @   .  X  X X
""", expect_for([16], {2: True, 3: False})),
    layout("paper-interdependent-3", "739-759", """
 @   S0   @ L2S   S1 @
L0E  .    .   .   .  @
 @   .    @   X   .  @
 @   .    @   .   X L1W
 @   .    @   .   .  @
 @   .    .   X   S2 @
""", expect_for([10], {2: True, 3: True})),
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
""", expect_for([14], {2: True, 3: True, 4: True, 5: True, 6: True, 7: False})),
]

MAPS = {
    # the reference's (python/tests/world_layouts.py:576-585; it states no `sequential` for it): both agents keep blocking for two steps
    "two-agent-mutual-compact": """
 S0 . . S1
L0E . . .
 .  . . L1W
 X  . . X
""",
    # two-agent-mutual-compact with a fifth column that holds a gem off everybody's way
    "gem-detour": """
 S0 . . S1 G
L0E . . .  .
 .  . . L1W .
 X  . . X  .
""",
    # agents 0 and 2 have to enter row 2 in the same step, each blocking the beam that would kill the other, with agent 1 between them
    # helped by both: 0 <-> 2, 0 -> 1 and 2 -> 1 in one state, a trail of three edges at once
    "three-beam-cell": """
 @  S0 L1S S2  @
 @  .  S1  .   @
L0E .  .   G  L2W
 @  .  .   .   @
 @  X  X   X   @
""",
    # six agents: the mutual pair is 3 <-> 5, so agent 5's field (bits 20-23) counts
    "six-mutual": """
 @  S5 S3  @  S0 S1 S2 S4
L5E .  .   @  X  X  X  X
 @  .  .  L3W @  @  @  @
 @  X  X   @  @  @  @  @
""",
    # helpers 3 and 5 converge on agent 4, and help each other
    "six-converge": """
 @  S3 S4 S5  @  S0 S1 S2
L3E .  .  .   @  X  X  X
 @  .  .  .  L5W @  @  @
 @  X  X  X   @  @  @  @
""",
    "chain-in-one-state": """
 @   @    L1S  @
L0E  S0   .    S1
 @   X    .    @
 S2  .    .    X
 @   @    X    @
""",
    "chain-at-reset": """
 @   @   L1S  @
L0E  S0  S1   @
 @   X   .    @
 @   @   S2   X
 @   @   X    @
""",
    "decreasing-times": """
 @   @   L1S  @
 @   @   S1   @
 S2  .   .    X
L0E  S0  .    @
 @   X   X    @
""",
    # two-agent-mutual-compact with its exits walled off (nobody ever arrives) and two exits nobody can reach: the agents can hold the
    # mutual pair over STAYs for as long as N allows, so the trails grow to N - 1 <= 15 and every N in 2 .. 16 gives other counters
    "long-trails": """
 S0 . . S1  @ X
L0E . . .   @ X
 .  . . L1W @ @
 .  . . .   @ @
""",
}


def S(map_name, t_max, n, length, states, frontier, expanded, collect_gems=False, changes=None):
    out = dict(map=map_name, t_max=t_max, n=n, collect_gems=collect_gems, length=length, states=states, frontier=frontier, expanded=expanded)
    if changes is not None:
        out["changes"] = changes
    return out


# changes (see above)
OFF0 = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}]}
OFF1 = {"sources": [{"laser_id": 1, "enabled": False, "colour": None}]}
RECOLOUR1 = {"sources": [{"laser_id": 1, "enabled": None, "colour": 0}]}
ALL_OFF = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}, {"laser_id": 1, "enabled": False, "colour": None}]}


SEARCHES = [
    # two arcs of one state chain: no plan under no-sequence-2, the plan's last L is (0, 1, 2)
    S("chain-in-one-state", 8, 2, None, 32, [1, 3, 7, 7, 13, 1, 0], [12, 60, 100, 104, 67, 4]),
    S("chain-in-one-state", 8, 3, 5, 83, [1, 3, 10, 21, 30, 18], [12, 60, 174, 277, 264]),
    # the reset state holds the trail 0 -> 1 -> 2: rejected under no-sequence-2 (one record, no level), stored under no-sequence-3
    S("chain-at-reset", 6, 2, None, 1, [1], []),
    S("chain-at-reset", 6, 3, 3, 19, [1, 9, 6, 3], [16, 77, 28]),
    # 1 -> 2 at t, 0 -> 1 later: a plan under no-sequence-2 whose last L is (0, 1, 1); longer detours reach a trail of 3
    S("decreasing-times", 8, 2, 6, 203, [1, 13, 27, 40, 57, 37, 28], [16, 229, 292, 370, 622, 234]),
    S("decreasing-times", 8, 4, 6, 383, [1, 13, 27, 43, 81, 91, 127], [16, 229, 292, 424, 949, 835]),
    # a mutual pair held over a STAY: the flattened relation stops changing after the first such state, the trails grow by 2 per step,
    # up to 4 within t_max 6 -- N = 5 rejects nothing (and equals N = 16), N = 4 and N = 3 store fewer records, N = 2 finds no plan
    S("two-agent-mutual-compact", 6, 2, None, 100, [1, 3, 6, 12, 29, 40, 9], [6, 29, 61, 160, 345, 379]),
    S("two-agent-mutual-compact", 6, 3, 5, 119, [1, 3, 6, 13, 34, 62], [6, 29, 61, 172, 414]),
    S("two-agent-mutual-compact", 6, 4, 5, 125, [1, 3, 6, 13, 35, 67], [6, 29, 61, 172, 426]),
    S("two-agent-mutual-compact", 6, 5, 5, 126, [1, 3, 6, 13, 35, 68], [6, 29, 61, 172, 426]),
    S("two-agent-mutual-compact", 6, 16, 5, 126, [1, 3, 6, 13, 35, 68], [6, 29, 61, 172, 426]),
    # 0 <-> 2, 0 -> 1, 2 -> 1 in one state: a trail of three edges from one layer, a cycle inside it; trails reach 7 within t_max 5
    S("three-beam-cell", 5, 2, None, 8, [1, 7, 0], [16, 90]),
    S("three-beam-cell", 5, 3, None, 97, [1, 7, 1, 8, 48, 32], [16, 90, 64, 410, 896]),
    S("three-beam-cell", 5, 4, 4, 146, [1, 7, 2, 16, 120], [16, 90, 91, 767]),
    S("three-beam-cell", 5, 7, 4, 231, [1, 7, 2, 24, 197], [16, 90, 91, 1128]),
    S("three-beam-cell", 5, 8, 4, 232, [1, 7, 2, 24, 198], [16, 90, 91, 1128]),
    S("three-beam-cell", 5, 16, 4, 232, [1, 7, 2, 24, 198], [16, 90, 91, 1128]),
    S("gem-detour", 8, 2, None, 379, [1, 5, 13, 30, 62, 94, 76, 61, 37], [8, 51, 161, 430, 759, 1012, 775, 699], collect_gems=True),
    S("gem-detour", 8, 3, 7, 453, [1, 5, 13, 31, 67, 117, 118, 101], [8, 51, 161, 442, 828, 1277, 1173], collect_gems=True),
    S("gem-detour", 8, 3, 5, 162, [1, 5, 9, 22, 48, 77], [8, 51, 112, 313, 593]),
    # six agents at t_max 3: the plan's last L is (0, 0, 0, 1, 0, 2) and (0, 0, 0, 2, 2, 1): agent 5's field, bits 20-23
    S("six-mutual", 3, 2, None, 1536, [1, 47, 392, 1096], [64, 3561, 26972]),
    S("six-mutual", 3, 3, 3, 1856, [1, 47, 436, 1372], [64, 3561, 29933]),
    S("six-converge", 3, 3, 3, 4540, [1, 39, 728, 3772], [64, 6296, 110470]),
    # long-trails: no plan for any N; the mutual pair is held over STAYs until some trail has N edges, so the search stores 100 + 76 (N - 2)
    # records, its greatest stored field is N - 1 (up to 15) and its frontier runs empty at depth N + 5
    S("long-trails", 24, 2, None, 100, [1, 3, 6, 12, 29, 40, 9, 0], [6, 29, 61, 160, 345, 404, 84]),
    S("long-trails", 24, 3, None, 176, [1, 3, 6, 13, 34, 62, 46, 11, 0], [6, 29, 61, 172, 414, 705, 465, 102]),
    S("long-trails", 24, 4, None, 252, [1, 3, 6, 13, 35, 67, 68, 48, 11, 0], [6, 29, 61, 172, 426, 774, 766, 483, 102]),
    S("long-trails", 24, 5, None, 328, [1, 3, 6, 13, 35, 68, 73, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 835, 784, 483, 102]),
    S("long-trails", 24, 6, None, 404, [1, 3, 6, 13, 35, 68, 74, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 853, 784, 483, 102]),
    S("long-trails", 24, 7, None, 480, [1, 3, 6, 13, 35, 68, 74, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 8, None, 556, [1, 3, 6, 13, 35, 68, 74, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 9, None, 632, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 10, None, 708, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 11, None, 784, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 12, None, 860, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 13, None, 936, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 14, None, 1012, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 865, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 15, None, 1088, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 76, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 865, 865, 865, 865, 865, 853, 784, 483, 102]),
    S("long-trails", 24, 16, None, 1164, [1, 3, 6, 13, 35, 68, 74, 76, 76, 76, 76, 76, 76, 76, 76, 76, 76, 75, 70, 48, 11, 0], [6, 29, 61, 172, 426, 786, 847, 865, 865, 865, 865, 865, 865, 865, 865, 865, 865, 853, 784, 483, 102]),
    # changed worlds: one layout, four worlds, four answers under no-sequence-2 (unchanged: None / 100 above, at t_max 6 and 8 alike)
    S("two-agent-mutual-compact", 8, 2, 5, 164, [1, 3, 6, 18, 57, 79], [6, 29, 61, 262, 708], changes=OFF1),
    S("two-agent-mutual-compact", 8, 3, 5, 164, [1, 3, 6, 18, 57, 79], [6, 29, 61, 262, 708], changes=OFF1),
    S("two-agent-mutual-compact", 8, 2, 5, 130, [1, 5, 10, 17, 36, 61], [6, 47, 115, 208, 461], changes=OFF0),
    S("two-agent-mutual-compact", 8, 3, 5, 130, [1, 5, 10, 17, 36, 61], [6, 47, 115, 208, 461], changes=OFF0),
    S("two-agent-mutual-compact", 8, 2, None, 107, [1, 3, 6, 15, 39, 33, 10, 0], [6, 29, 61, 218, 440, 263, 35], changes=RECOLOUR1),
    S("two-agent-mutual-compact", 8, 3, None, 107, [1, 3, 6, 15, 39, 33, 10, 0], [6, 29, 61, 218, 440, 263, 35], changes=RECOLOUR1),
    S("long-trails", 24, 16, None, 198, [1, 3, 6, 18, 57, 79, 31, 3, 0], [6, 29, 61, 262, 708, 823, 259, 15], changes=OFF1),
    # every source disabled: nobody helps anybody, every N walks the plain search
    S("two-agent-mutual-compact", 8, 2, 5, 151, [1, 5, 10, 22, 57, 56], [6, 47, 115, 303, 718], changes=ALL_OFF),
    S("two-agent-mutual-compact", 8, 16, 5, 151, [1, 5, 10, 22, 57, 56], [6, 47, 115, 303, 718], changes=ALL_OFF),
]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "kat_trails.json"), "w") as f:
        json.dump(dict(catalogue=CATALOGUE, maps=MAPS, searches=SEARCHES), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
