"""Hand transcription of the reference's help-graph expectations as data; running it rewrites kat_helpgraph.json.

`catalogue` restates python/tests/world_layouts.py for eleven layouts: the map text and, per t_max, the stated `asymmetric`,
`fully_coupled`, `convergent`, `divergent` and `interdependent[2]`.  Every other stated field (`solvable`, `cooperative`: they are in
kat_solver.json; `sequential`, `interdependent[>= 3]`: they need temporal trails) is left out.  Nothing here imports or executes the
reference; only inputs and expected outputs are kept.

`searches` are the searches the GPU tests run, one per (map, t_max, mode, param, collect_gems): `length` (null: no plan) and `states`
(distinct (world state, help relation) records stored) were worked out with a plain-Python breadth-first search over the oracle before
tests/helpgraph_ref.py existed, `frontier` and `expanded` per depth are what tests/helpgraph_ref.py gives (tests/test_helpgraph_cpu.py
holds it to every entry here).  `maps` are the maps that are not the reference's.

A search may carry a `changes` key: what is done to the world of the map text BEFORE the search is set up, as plain data --
  {"sources": [{"laser_id": 0, "enabled": false, "colour": null}, ...], "exits": [[i, j], ...]}
`sources`: per listed source, `enabled` switches it on or off and `colour` recolours it (null or missing: as the text has it);
`exits`: the new exit cells, the old ones become floor (a cell under a beam may be given).  tests/helpgraph_ref.py applies it to the
oracle world (set_source / set_exits before the reset) and to an lle_amd.World (LaserSource.disable / enable / set_colour, the
exit_pos setter) before the solver is constructed, which keeps the map as it is at that moment.  A search without the key runs on the
map as written.

One layout of the catalogue has no search here: `fully-coupled-4agents` stores 84 128 records within its t_max of 8 (13 991 in the plain
search of lle_amd.Solver), far beyond what the restatement walks in test time.  Both searches, which step through `World.step`, find NO
plan within 8 steps on it, where the reference, whose solver is a SAT model of the rules, states `fully_coupled` for that horizon: the
stated values are kept as data and are not reproduced.
"""
import json
import os

LAYOUTS = "python/tests/world_layouts.py"


def expect_for(horizons, **fields):
    out = {}
    for key in ("convergent", "divergent", "interdependent"):
        if key in fields:
            fields[key] = {str(k): v for k, v in fields[key].items()}
    for t in horizons:
        out[str(t)] = {k: (dict(v) if isinstance(v, dict) else v) for k, v in fields.items()}
    return out


def layout(name, ref, text, *expectations):
    by_t_max = {}
    for e in expectations:
        by_t_max.update(e)
    return dict(name=name, ref=f"{LAYOUTS}:{ref}", map=text, expect=by_t_max)


CATALOGUE = [
    layout("single-laser-asymmetric", "316-335", """
 @  S0 S1
L0E .  .
 @  X  X
""", expect_for([6], asymmetric=True, convergent={2: False}, divergent={2: False}, interdependent={2: False})),
    layout("double-disjoint-asymmetric", "337-345", """
 @  S0 S1 @  @  S2 S3
L0E .  .  @ L2E .  .
 @  X  X  @  @  X  X
""", expect_for([6], asymmetric=True, convergent={2: False}, divergent={2: False})),
    layout("convergent-2-tight", "347-367", """
 @  S0  @  @  @  S2
L0E  .  .  .  .  .
 @   X  @  @  @  .
L1E  .  .  .  .  .
 @  S1  @  @  @  .
 @   X  @  @  @  X
""", expect_for([5], convergent={2: True, 3: False}, divergent={2: False})),
    layout("divergent-2-tight", "369-387", """
 @   X   X   X  @
L0E  .   .   .  .
 @  S0  S1  S2  @
""", expect_for([2, 8], convergent={2: False}, asymmetric=True, divergent={2: True, 3: False})),
    layout("divergent-2-with-detour", "389-403", """
 @   X   X   X  @   X
L0E  .   .   .  @   .
 @  S0  S1  S2  @   .
 @   @   @   .   .  .
""", expect_for([2, 5], divergent={2: True}), expect_for([6, 8], divergent={2: False})),
    layout("paper-convergent-2", "488-508", """
 @   S0  .  S2  .
L0E  .   .  .   @
 @   X   @  .   .
 @  L1E  .  S1  .
 @   @   @  X   X
""", expect_for([10], convergent={2: True, 3: False}, divergent={2: False}, interdependent={2: False}, asymmetric=True)),
    layout("paper-fully-coupled", "510-533", """
 @  L0S  @ @ @ @
S0   .   . . @ @
S1   .   . . . @
S2   .   . . . @
 @  L2E  . . . @
 @   @   X X X L1W
""", expect_for([10], asymmetric=False, fully_coupled=True, convergent={2: True, 3: False}, divergent={2: True, 3: False},
                interdependent={2: True})),
    layout("paper-fully-coupled-legacy", "535-556", """
 .  S0 S1 S2 .
L0E .  .  .  .
 .  .  .  . L2W
L1E .  .  .  .
 .  X  X  X  .
""", expect_for([10], asymmetric=False, fully_coupled=True, interdependent={2: True})),
    layout("fully-coupled-4agents", "558-574", """
 @  S0 S1 S2 S3 .
L0E .  .  .  .  .
L1E .  .  .  .  .
L2E .  .  .  .  .
L3E X  X  X  X  X
""", expect_for([8], fully_coupled=True, interdependent={2: True})),
    layout("two-agent-mutual-compact", "576-585", """
 S0 . . S1
L0E . . .
 .  . . L1W
 X  . . X
""", expect_for([6], asymmetric=False, interdependent={2: True})),
    layout("two-agent-mutual-with-detours", "587-635", """
 .  . . S0 S1  .  . . .
L0E . .  .  .  @  @ @ .
 .  . @  .  . L1W . . .
 .  . .  .  .  .  . . .
 .  . .  X  X  .  . . .
""", expect_for(range(5, 8), interdependent={2: True}), expect_for(range(8, 15), interdependent={2: False})),
]

# maps of this project's making
MAPS = {
    # six agents: the help bits of agent 5 lie in the second help word
    "six-agents": """
 @  S5 S4  @ S0 S1 S2 S3
L5E .  .   @ X  X  X  X
 @  X  X   @ @  @  @  @
""",
    # two-agent-mutual-compact with a fifth column that holds a gem off everybody's way
    "gem-detour": """
 S0 . . S1 G
L0E . . .  .
 .  . . L1W .
 X  . . X  .
""",
    # two sources of colour 0 (laser_id 0 on row 1, laser_id 1 on row 2) whose beams share no cell: agent 1 crosses both rows behind
    # agent 0, so the plan's edge (0, 1) comes from either source; the gem lies under the first beam, off the shortest way
    "shared-colour": """
 @  S0 S1  .  @
L0E .  .   G  @
L0E .  .   .  @
 @  X  X   @  @
""",
    # three beams of three colours run through (2, 2): L1S down column 2 (over the start of agent 1 and the exit (4, 2)), L0E and L2W
    # along row 2 (over the gem).  World.lasers lists the outer two layers of a cell only, so at (2, 2) the source parsed first, L1S,
    # owns no tile: there the cell's word holds two bits, not three.  Agents 0 and 2 have to enter row 2 in the same step, each
    # blocking the beam that would kill the other, with agent 1 between them helped by both.
    "three-beam-cell": """
 @  S0 L1S S2  @
 @  .  S1  .   @
L0E .  .   G  L2W
 @  .  .   .   @
 @  X  X   X   @
""",
    # six agents whose edges lie in both help words: (3, 5) is bit 29 of the low word, (5, 3) bit 43 = bit 11 of the high word
    "six-mutual": """
 @  S5 S3  @  S0 S1 S2 S4
L5E .  .   @  X  X  X  X
 @  .  .  L3W @  @  @  @
 @  X  X   @  @  @  @  @
""",
    # helpers 3 (low word) and 5 (high word) converge on agent 4
    "six-converge": """
 @  S3 S4 S5  @  S0 S1 S2
L3E .  .  .   @  X  X  X
 @  .  .  .  L5W @  @  @
 @  X  X  X   @  @  @  @
""",
}

# changes (see above)
OFF0 = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}]}
OFF2 = {"sources": [{"laser_id": 2, "enabled": False, "colour": None}]}
RECOLOURED = {"sources": [{"laser_id": 0, "enabled": None, "colour": 1}]}
ALL_OFF = {"sources": [{"laser_id": l, "enabled": False, "colour": None} for l in range(3)]}  # nobody can help anybody: every mode is `standard`
EXITS_SINGLE = {"exits": [[1, 1], [2, 2]]}   # single-laser-asymmetric: the exit (1, 1) lies under the beam, next to the source
EXITS_COMPACT = {"exits": [[3, 0], [2, 2]]}  # two-agent-mutual-compact: the exit (2, 2) lies under the beam of L1W


def S(map_name, t_max, mode, length, states, param=2, collect_gems=False, frontier=None, expanded=None, changes=None):
    out = dict(map=map_name, t_max=t_max, mode=mode, param=param, collect_gems=collect_gems, length=length, states=states, frontier=frontier,
               expanded=expanded)
    if changes is not None:
        out["changes"] = changes
    return out


SEARCHES = [
    S("single-laser-asymmetric", 6, "standard", 2, 14, frontier=[1, 2, 11], expanded=[4, 21]),
    S("single-laser-asymmetric", 6, "no-asymmetric", None, 26, frontier=[1, 2, 11, 9, 3, 0], expanded=[4, 21, 57, 43, 10]),
    S("double-disjoint-asymmetric", 6, "standard", 2, 196, frontier=[1, 8, 187], expanded=[16, 609]),
    S("double-disjoint-asymmetric", 6, "no-asymmetric", None, 676, frontier=[1, 8, 187, 333, 147, 0], expanded=[16, 609, 6099, 8901, 2600]),
    S("divergent-2-tight", 8, "no-asymmetric", None, 480, frontier=[1, 4, 68, 128, 146, 94, 39, 0], expanded=[8, 176, 1257, 2017, 1731, 845, 293]),
    S("divergent-2-tight", 8, "no-divergence", None, 252, frontier=[1, 3, 49, 81, 62, 41, 15, 0], expanded=[8, 140, 949, 1108, 695, 397, 116]),
    S("divergent-2-tight", 8, "no-divergence", 2, 73, param=3, frontier=[1, 4, 68], expanded=[8, 176]),
    S("divergent-2-with-detour", 5, "no-divergence", None, 963, frontier=[1, 6, 78, 202, 304, 372], expanded=[12, 250, 1776, 3998, 5987]),
    S("divergent-2-with-detour", 6, "no-divergence", 6, 1408, frontier=[1, 6, 78, 202, 304, 372, 445], expanded=[12, 250, 1776, 3998, 5987, 7543]),
    S("convergent-2-tight", 5, "no-convergence", None, 245, frontier=[1, 8, 68, 58, 58, 52], expanded=[12, 212, 1176, 1149, 1108]),
    S("convergent-2-tight", 5, "no-convergence", 5, 505, param=3, frontier=[1, 8, 68, 73, 155, 200], expanded=[12, 212, 1176, 1665, 3335]),
    S("two-agent-mutual-compact", 6, "standard", 5, 123, frontier=[1, 3, 6, 13, 35, 65], expanded=[6, 29, 61, 172, 426]),
    S("two-agent-mutual-compact", 6, "no-asymmetric", 5, 123, frontier=[1, 3, 6, 13, 35, 65], expanded=[6, 29, 61, 172, 426]),
    S("two-agent-mutual-compact", 6, "no-mutual", None, 100, frontier=[1, 3, 6, 12, 29, 40, 9], expanded=[6, 29, 61, 160, 345, 379]),
    S("two-agent-mutual-with-detours", 7, "no-mutual", None, 924, frontier=[1, 6, 26, 62, 95, 172, 244, 318], expanded=[9, 87, 352, 848, 1248, 2106, 3292]),
    S("two-agent-mutual-with-detours", 8, "no-mutual", 8, 1225, frontier=[1, 6, 26, 62, 95, 172, 244, 318, 301], expanded=[9, 87, 352, 848, 1248, 2106, 3292, 4334]),
    S("six-agents", 4, "standard", 2, 616, frontier=[1, 47, 568], expanded=[64, 3561]),
    S("six-agents", 4, "no-asymmetric", None, 2184, frontier=[1, 47, 568, 856, 712], expanded=[64, 3561, 23353, 26647]),
    S("gem-detour", 8, "no-asymmetric", 5, 166, frontier=[1, 5, 9, 22, 49, 80], expanded=[8, 51, 112, 313, 605]),
    S("gem-detour", 8, "no-asymmetric", 7, 494, collect_gems=True, frontier=[1, 5, 13, 31, 68, 120, 130, 126], expanded=[8, 51, 161, 442, 840, 1318, 1342]),
    S("paper-fully-coupled", 10, "standard", 8, 3965, frontier=[1, 4, 59, 357, 906, 1034, 422, 390, 792], expanded=[8, 151, 2416, 17103, 46037, 48491, 17755, 16740]),
    S("paper-fully-coupled", 10, "no-asymmetric", 8, 3965, frontier=[1, 4, 59, 357, 906, 1034, 422, 390, 792], expanded=[8, 151, 2416, 17103, 46037, 48491, 17755, 16740]),
    S("paper-fully-coupled", 10, "no-mutual", None, 4617, frontier=[1, 4, 59, 357, 906, 1034, 398, 302, 588, 599, 369], expanded=[8, 151, 2416, 17103, 46037, 48491, 17226, 13563, 27459, 25982]),
    S("paper-fully-coupled", 10, "no-fully-coupled", None, 6509, frontier=[1, 4, 59, 357, 906, 1034, 422, 390, 791, 1203, 1342], expanded=[8, 151, 2416, 17103, 46037, 48491, 17755, 16740, 39023, 56667]),
    S("paper-fully-coupled", 10, "no-convergence", None, 4016, frontier=[1, 4, 59, 357, 906, 1023, 332, 95, 160, 449, 630], expanded=[8, 151, 2416, 17103, 46037, 47979, 14280, 4122, 9788, 24034]),
    S("paper-fully-coupled", 10, "no-divergence", None, 1199, frontier=[1, 3, 43, 171, 293, 286, 88, 21, 39, 114, 140], expanded=[8, 124, 1641, 7098, 13250, 12154, 3816, 868, 2520, 6152]),
    S("paper-convergent-2", 10, "no-asymmetric", None, 4492, frontier=[1, 44, 163, 223, 318, 527, 455, 476, 614, 838, 833], expanded=[60, 1464, 3885, 5427, 8649, 11320, 9026, 9593, 13420, 18116]),
    S("paper-convergent-2", 10, "no-convergence", None, 2797, frontier=[1, 44, 163, 217, 285, 419, 328, 213, 271, 427, 429], expanded=[60, 1464, 3885, 5347, 7851, 9435, 6349, 4442, 6472, 9876]),
    S("paper-convergent-2", 10, "no-divergence", 5, 1003, frontier=[1, 44, 162, 209, 246, 341], expanded=[60, 1464, 3867, 5008, 6438]),
    S("paper-fully-coupled-legacy", 10, "standard", 6, 4375, frontier=[1, 9, 64, 301, 809, 1608, 1583], expanded=[18, 353, 2889, 13316, 34557, 57096]),
    S("paper-fully-coupled-legacy", 10, "no-asymmetric", 6, 4375, frontier=[1, 9, 64, 301, 809, 1608, 1583], expanded=[18, 353, 2889, 13316, 34557, 57096]),
    S("paper-fully-coupled-legacy", 10, "no-mutual", None, 2064, frontier=[1, 9, 59, 222, 439, 622, 442, 207, 55, 8, 0], expanded=[18, 353, 2533, 9246, 17609, 19879, 13602, 5378, 1144, 120]),
    S("paper-fully-coupled-legacy", 10, "no-fully-coupled", None, 7599, frontier=[1, 9, 64, 301, 809, 1606, 1565, 1293, 799, 717, 435], expanded=[18, 353, 2889, 13316, 34557, 57012, 51827, 40284, 25701, 21118]),
    S("paper-fully-coupled-legacy", 10, "no-convergence", None, 1744, frontier=[1, 9, 61, 270, 480, 523, 251, 124, 23, 2, 0], expanded=[18, 353, 2757, 11372, 18373, 15280, 6596, 3107, 264, 12]),
    S("paper-fully-coupled-legacy", 10, "no-convergence", 6, 4375, param=3, frontier=[1, 9, 64, 301, 809, 1608, 1583], expanded=[18, 353, 2889, 13316, 34557, 57096]),
    S("paper-fully-coupled-legacy", 10, "no-divergence", None, 930, frontier=[1, 8, 50, 184, 252, 247, 118, 58, 11, 1, 0], expanded=[18, 317, 2231, 7160, 8657, 6811, 2929, 1460, 129, 6]),
    S("paper-fully-coupled-legacy", 10, "no-divergence", 6, 4375, param=3, frontier=[1, 9, 64, 301, 809, 1608, 1583], expanded=[18, 353, 2889, 13316, 34557, 57096]),
    # ---- maps of this project's making and changed worlds, all worked out with tests/helpgraph_ref.py
    S("shared-colour", 6, "standard", 3, 49, frontier=[1, 4, 14, 30], expanded=[6, 49, 172]),
    S("shared-colour", 6, "no-asymmetric", None, 76, frontier=[1, 4, 14, 30, 21, 5, 1], expanded=[6, 49, 172, 288, 147, 26]),
    S("shared-colour", 6, "standard", 5, 123, collect_gems=True, frontier=[1, 4, 14, 37, 42, 25], expanded=[6, 49, 172, 375, 359]),
    S("three-beam-cell", 5, "standard", 4, 169, frontier=[1, 7, 2, 22, 137], expanded=[16, 90, 91, 1037]),
    S("three-beam-cell", 5, "no-mutual", None, 8, frontier=[1, 7, 0], expanded=[16, 90]),
    S("three-beam-cell", 5, "no-convergence", None, 75, frontier=[1, 7, 1, 12, 42, 12], expanded=[16, 90, 64, 536, 654]),
    S("three-beam-cell", 5, "no-divergence", None, 131, frontier=[1, 7, 1, 12, 50, 60], expanded=[16, 90, 64, 536, 960]),
    S("three-beam-cell", 5, "no-convergence", 4, 169, param=3, frontier=[1, 7, 2, 22, 137], expanded=[16, 90, 91, 1037]),
    # source 2 (L2W) disabled: agent 1 may stand on (2, 2) with agent 0 alone at its side
    S("three-beam-cell", 5, "standard", 4, 347, changes=OFF2, frontier=[1, 7, 8, 66, 265], expanded=[16, 90, 275, 2791]),
    S("three-beam-cell", 5, "no-asymmetric", None, 692, changes=OFF2, frontier=[1, 7, 8, 66, 265, 345], expanded=[16, 90, 275, 2791, 5918]),
    S("three-beam-cell", 5, "no-convergence", 4, 334, changes=OFF2, frontier=[1, 7, 8, 66, 252], expanded=[16, 90, 275, 2791]),
    # source 0 disabled / recoloured to 1 / an exit moved under a beam
    S("single-laser-asymmetric", 6, "standard", 2, 17, changes=OFF0, frontier=[1, 3, 13], expanded=[4, 33]),
    S("single-laser-asymmetric", 6, "no-asymmetric", 2, 17, changes=OFF0, frontier=[1, 3, 13], expanded=[4, 33]),
    S("single-laser-asymmetric", 6, "standard", 4, 17, changes=RECOLOURED, frontier=[1, 1, 5, 4, 6], expanded=[4, 12, 30, 19]),
    S("single-laser-asymmetric", 6, "no-asymmetric", None, 26, changes=RECOLOURED, frontier=[1, 1, 5, 4, 6, 6, 3], expanded=[4, 12, 30, 19, 27, 33]),
    S("single-laser-asymmetric", 6, "standard", 2, 6, changes=EXITS_SINGLE, frontier=[1, 2, 3], expanded=[4, 6]),
    S("single-laser-asymmetric", 6, "no-asymmetric", None, 7, changes=EXITS_SINGLE, frontier=[1, 2, 3, 1, 0], expanded=[4, 6, 6, 2]),
    S("two-agent-mutual-compact", 6, "standard", 5, 130, changes=OFF0, frontier=[1, 5, 10, 17, 36, 61], expanded=[6, 47, 115, 208, 461]),
    S("two-agent-mutual-compact", 6, "no-asymmetric", None, 205, changes=OFF0, frontier=[1, 5, 10, 17, 36, 61, 75], expanded=[6, 47, 115, 208, 461, 655]),
    S("two-agent-mutual-compact", 6, "no-mutual", 5, 130, changes=OFF0, frontier=[1, 5, 10, 17, 36, 61], expanded=[6, 47, 115, 208, 461]),
    S("two-agent-mutual-compact", 6, "standard", 5, 64, changes=EXITS_COMPACT, frontier=[1, 3, 6, 13, 22, 19], expanded=[6, 29, 61, 140, 167]),
    S("two-agent-mutual-compact", 6, "no-mutual", None, 58, changes=EXITS_COMPACT, frontier=[1, 3, 6, 12, 19, 15, 2], expanded=[6, 29, 61, 136, 156, 107]),
    S("paper-fully-coupled", 10, "standard", 7, 6346, changes=ALL_OFF, frontier=[1, 7, 73, 424, 1126, 1719, 1801, 1195], expanded=[8, 256, 3205, 20958, 55497, 77509, 62527]),
    # six agents at t_max 3, the shortest horizon at which 'no plan' says something: edges in both help words
    S("six-mutual", 3, "standard", 3, 1920, frontier=[1, 47, 436, 1436], expanded=[64, 3561, 29933]),
    S("six-mutual", 3, "no-mutual", None, 1536, frontier=[1, 47, 392, 1096], expanded=[64, 3561, 26972]),
    S("six-converge", 3, "standard", 3, 4880, frontier=[1, 39, 728, 4112], expanded=[64, 6296, 110470]),
    S("six-converge", 3, "no-mutual", None, 3300, frontier=[1, 39, 648, 2612], expanded=[64, 6296, 92900]),
    S("six-converge", 3, "no-convergence", None, 4220, frontier=[1, 39, 680, 3500], expanded=[64, 6296, 102700]),
    S("six-converge", 3, "no-divergence", None, 2420, frontier=[1, 31, 544, 1844], expanded=[64, 5216, 78650]),
    S("six-converge", 3, "no-divergence", 3, 4880, param=3, frontier=[1, 39, 728, 4112], expanded=[64, 6296, 110470]),
    S("six-converge", 3, "no-fully-coupled", 3, 4880, frontier=[1, 39, 728, 4112], expanded=[64, 6296, 110470]),
]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "kat_helpgraph.json"), "w") as f:
        json.dump(dict(catalogue=CATALOGUE, maps=MAPS, searches=SEARCHES), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
