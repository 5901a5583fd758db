"""Hand transcription of the reference's `interdependent` expectations for orders >= 3 as data; running it rewrites kat_cycles.json.

`catalogue` restates python/tests/world_layouts.py for every layout that states `interdependent` for an order of 3 or more and that the
closed-trail search can be held to: the map text and, per t_max, the stated booleans by order (orders >= 3 only; order 2 is in
kat_helpgraph.json).  Nothing here imports or executes the reference; only inputs and expected outputs are kept.

`maps` are the maps that are not in the catalogue: four of tests/golden/kat_helpgraph.json, repeated here so that this file stands
alone (`two-agent-mutual-compact` is the reference's, `gem-detour`, `six-mutual` and `six-converge` this project's), and five made for
the closed-trail search (the comments at each say what it forces).

`searches` are the searches the GPU tests run, one per (map, changes, t_max, n, collect_gems): `length` (null: no plan), `states`
(distinct (world state, triples) records stored), `frontier` and `expanded` per depth, all worked out with tests/cycles_ref.py
(tests/test_cycles_cpu.py holds it to every entry here).  `n` never exceeds the map's agents: above them no closed trail is possible
and CycleSolver answers with the standard search.  A search may carry a `changes` key, as in tests/golden/kat_trails.json.

Every stated value is reproduced by tests/cycles_ref.py and by liblle_cycles.so, with no contradiction.  Left out, by name:
  level-6                                 at t_max 21 the pool of 4 194 304 records overflows, as the plain search does at depth 11
  fully-coupled-4agents                   has no plan through World.step (the reference states its values for its SAT encoding)
  eight-agent-interdependent-8            more than six agents
  eight-agent-interdependent-8-perimeter  more than six agents
"""
import json
import os

LAYOUTS = "python/tests/world_layouts.py"


def expect_for(horizons, interdependent):
    return {str(t): {"interdependent": {str(k): v for k, v in interdependent.items()}} for t in horizons}


def layout(name, ref, text, *expectations):
    by_t_max = {}
    for e in expectations:
        by_t_max.update(e)
    return dict(name=name, ref=f"{LAYOUTS}:{ref}", expect=by_t_max, map=text)


CATALOGUE = [
    layout("one-way-detour", "284-314", """
 .  . S0 S1 . .
L0E .  .  . @ .
 .  .  .  . . .
 .  .  .  . . .
 X  X  .  . . .
""", expect_for(range(6, 12), {3: False})),
    layout("sequence-4-with-mutual", "405-424", """
 @  S0 S1  @
L0E X  .   @
 @  S2 .   @
 @  .  X  L1W
 @  .  S3  @
L2E .  .   @
 @  X  X  L3W
""", expect_for([6], {3: False, 4: False})),
    layout("sequence-3-without-cycle", "426-445", """
 @  S0 S1  @
L0E X  .   @
 @  S2 .   @
 @  .  X  L1W
 @  .  S3  @
L2E X  .   @
 @  .  X   @
""", expect_for([6], {3: False, 4: False})),
    layout("paper-sequence-2-not-interdependent-3", "467-486", """
 @  S0 @  @  L1S S1
L0E .  .  .   .  .
 @  . S2 L2W  .  X
 @  .  .  .   .  X
L0E .  @  .   .  .
 @  X  @  .   .  .
""", expect_for([10], {3: False})),
    layout("paper-fully-coupled", "510-533", """
 @  L0S  @ @ @ @
S0   .   . . @ @
S1   .   . . . @
S2   .   . . . @
 @  L2E  . . . @
 @   @   X X X L1W
""", expect_for([10], {3: True, 4: False})),
    layout("paper-fully-coupled-legacy", "535-556", """
 .  S0 S1 S2 .
L0E .  .  .  .
 .  .  .  . L2W
L1E .  .  .  .
 .  X  X  X  .
""", expect_for([10], {3: True, 4: False})),
    layout("two-agent-mutual-with-detours", "587-635", """
 .  . . S0 S1  .  . . .
L0E . .  .  .  @  @ @ .
 .  . @  .  . L1W . . .
 .  . .  .  .  .  . . .
 .  . .  X  X  .  . . .
""", expect_for([6], {3: False})),
    layout("temporal-flattening-counterexample", "649-699", """
 @  @  L1S @ L3S  @   @
 @  S0 S1  @ S3  S2   @
L0E .   .  @  .   .  L2W
 @  .   X  @  X   .   @
 @  .   .  .  .   .   @
 @ L2E  X  @  X  L0W  @
""", expect_for([20], {3: False})),
    layout("three-agent-temporal-cycle", "701-717", """
 @ L0S L2S L1S .
S0  .   .   .  X
S1  .   .   .  X
S2  .   .   .  X
""", expect_for([15], {3: True, 4: False})),
    layout("three-agent-with-two-agent-cycle", "719-737", """
 .  S1  S0 S2 @ @
 . L0E  .  .  @ @
 .  .  L1W .  . .
 @  .   .  @  . .
L2E .   .  .  . .
 @  @   .  X  X X
""", expect_for([16], {3: False})),
    layout("paper-interdependent-3", "739-759", """
 @   S0   @ L2S   S1 @
L0E  .    .   .   .  @
 @   .    @   X   .  @
 @   .    @   .   X L1W
 @   .    @   .   .  @
 @   .    .   X   S2 @
""", expect_for([10], {3: True, 4: False})),
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
""", expect_for([14], {3: True, 4: True, 5: False})),
]

MAPS = {
    "two-agent-mutual-compact": """
 S0 . . S1
L0E . . .
 .  . . L1W
 X  . . X
""",
    "gem-detour": """
 S0 . . S1 G
L0E . . .  .
 .  . . L1W .
 X  . . X  .
""",
    "six-mutual": """
 @  S5 S3  @  S0 S1 S2 S4
L5E .  .   @  X  X  X  X
 @  .  .  L3W @  @  @  @
 @  X  X   @  @  @  @  @
""",
    "six-converge": """
 @  S3 S4 S5  @  S0 S1 S2
L3E .  .  .   @  X  X  X
 @  .  .  .  L5W @  @  @
 @  X  X  X   @  @  @  @
""",
    # 0 -> 1 (row 1), 1 -> 2 (row 2), 2 -> 3 (row 3), 3 -> 0 (row 5), forced in this order: a ring over four agents without a chord, so no
    # closed trail over two or three agents
    "ring-of-four": """
 @  S0  @  S1  @  S2  @  S3  @
L0E .   .  .   @  .   @  .   @
 @  .  L1E .   .  .   @  .   @
 @  .   @  .  L2E .   .  .   @
 @  .   @  X   @  X   @  .   @
 @  .   .  .   .  .   .  .  L3W
 @  X   @  @   @  @   @  X   @
""",
    # 0 <-> 1 in rows 1 and 2, then 0 <-> 2 in rows 4 and 5: the only closed trail over three agents is 0 -> 1 -> 0 -> 2 -> 0, through the
    # closed triple (0, 0, {0, 1}); the flattened relation holds no cycle over three agents
    "revisited-anchor": """
 @  S2  @   S0  @   S1  @
 @  .  L0E  .   .   .   @
 @  .   @   .   .   .  L1W
 @  .   @   .   @   X   @
 @  .   .   .  L0W  @   @
L2E .   .   .   @   @   @
 @  X   @   X   @   @   @
""",
    # 2 -> 0 in row 1, then 1 -> 2 in row 2, then 0 -> 1 in row 4, forced in this order by the way down: the flattened relation is the
    # 3-cycle 0 -> 1 -> 2 -> 0, the times decrease along it, no closed trail exists
    "cycle-against-time": """
 @  S0  @  S2  @   S1  @
 @  .   .  .  L2W  .   @
 @  .   @  .   .   .  L1W
 @  .   @  X   @   .   @
L0E .   .  .   .   .   @
 @  X   @  @   @   X   @
""",
    # the reset state holds 0 -> 1 -> 2 in ONE state (agent 1 on the crossing of L0E and its own L1S, agent 2 below it), agent 0 can leave only
    # through L2W behind agent 2: 0 -> 1, 1 -> 2 at t = 0 and 2 -> 0 later close order 3 only if the two arcs of the reset state chain
    "closes-in-one-state": """
 @   @   @  L1S  @
L0E  S0  .  S1   @
 @   .   @  .    X
 @   .   @  S2   X
 @   .   .  .   L2W
 @   X   @  @    @
""",
    # both agents start between the two sources that face each other: the reset state itself holds 0 <-> 1
    "mutual-at-reset": """
L0E S0 S1 L1W
 @  X  X  @
""",
}


def S(map_name, t_max, n, length, states, frontier, expanded, collect_gems=False, changes=None):
    out = dict(map=map_name, t_max=t_max, n=n, collect_gems=collect_gems, length=length, states=states, frontier=frontier, expanded=expanded)
    if changes is not None:
        out["changes"] = changes
    return out


# changes of closes-in-one-state (sources in reading order: 0 = L1S, 1 = L0E, 2 = L2W)
OFF2 = {"sources": [{"laser_id": 2, "enabled": False, "colour": None}]}       # nobody has to help agent 0 out: a plan under order 3
RECOLOUR2 = {"sources": [{"laser_id": 2, "enabled": None, "colour": 1}]}      # the last beam is agent 1's: 1 -> 0 closes order 2, not 3


SEARCHES = [
    # the catalogue (the comments: closed orders of the plan's last state, twins and merges as tests/cycles_ref.py counts them)
    S("sequence-3-without-cycle", 6, 3, 6, 122, [1, 11, 14, 19, 22, 23, 32], [64, 480, 408, 408, 497, 305]),  # closed orders [] twins 31 merges 175
    S("sequence-3-without-cycle", 6, 4, 6, 122, [1, 11, 14, 19, 22, 23, 32], [64, 480, 408, 408, 497, 305]),  # closed orders [] twins 31 merges 175
    S("sequence-4-with-mutual", 6, 3, 6, 127, [1, 11, 14, 19, 22, 23, 37], [64, 480, 408, 408, 497, 320]),  # closed orders [2] twins 33 merges 175
    S("sequence-4-with-mutual", 6, 4, 6, 127, [1, 11, 14, 19, 22, 23, 37], [64, 480, 408, 408, 497, 320]),  # closed orders [2] twins 33 merges 175
    S("paper-interdependent-3", 10, 3, None, 188, [1, 8, 47, 37, 29, 33, 29, 4, 0], [12, 212, 1264, 498, 420, 429, 419, 27]),  # closed orders None twins 70 merges 333
    S("paper-fully-coupled", 10, 3, None, 6500, [1, 4, 59, 357, 906, 1034, 422, 390, 789, 1200, 1338], [8, 151, 2416, 17103, 46037, 48491, 17755, 16740, 39014, 56653]),  # closed orders None twins 2526 merges 40913
    S("paper-fully-coupled-legacy", 10, 3, None, 13854, [1, 9, 64, 301, 898, 2120, 2841, 3348, 2230, 1513, 529], [18, 353, 2889, 13316, 39757, 82040, 108732, 109903, 73814, 40895]),  # closed orders None twins 12135 merges 58068
    S("three-agent-temporal-cycle", 15, 3, None, 3879, [1, 4, 36, 79, 92, 69, 119, 257, 390, 388, 593, 485, 412, 275, 338, 341], [8, 151, 1175, 2531, 2883, 2699, 4820, 9838, 12732, 13698, 19800, 15005, 12444, 10024, 10217]),  # closed orders None twins 2356 merges 14135
    S("paper-sequence-2-not-interdependent-3", 10, 3, 7, 6011, [1, 10, 78, 179, 498, 1045, 1852, 2348], [16, 332, 2337, 5973, 15936, 35644, 67491]),  # closed orders [] twins 5294 merges 24887
    S("three-agent-with-two-agent-cycle", 16, 3, 11, 8951, [1, 5, 31, 97, 222, 390, 746, 893, 1298, 1353, 1579, 2336], [8, 108, 668, 2589, 6232, 14190, 23355, 25377, 39849, 40234, 46498]),  # closed orders [2] twins 2160 merges 46346
    S("four-agent-interdependent-4-sequence-6", 14, 3, None, 6589, [1, 2, 8, 19, 29, 52, 74, 200, 457, 840, 882, 708, 901, 1118, 1298], [16, 84, 308, 660, 1204, 2272, 3910, 9637, 21362, 37137, 38070, 31262, 36012, 39985]),  # closed orders None twins 2782 merges 22684
    S("four-agent-interdependent-4-sequence-6", 14, 4, None, 7770, [1, 2, 8, 19, 29, 52, 74, 200, 457, 840, 908, 782, 1152, 1447, 1799], [16, 84, 308, 660, 1204, 2272, 3910, 9637, 21362, 37137, 38242, 33537, 42386, 48533]),  # closed orders None twins 3664 merges 26928
    S("temporal-flattening-counterexample", 20, 3, 11, 21345, [1, 8, 160, 456, 531, 1735, 2158, 3182, 2173, 2646, 3124, 5171], [16, 609, 9176, 24795, 41029, 104790, 119751, 147668, 112857, 132392, 178154]),  # closed orders [2] twins 21116 merges 90471
    S("closes-in-one-state", 8, 2, 5, 178, [1, 17, 33, 32, 55, 40], [36, 321, 587, 683, 715]),  # closed orders [] twins 0 merges 409
    S("closes-in-one-state", 8, 3, None, 131, [1, 17, 33, 26, 39, 15, 0], [36, 321, 587, 551, 465, 170]),  # closed orders None twins 0 merges 324
    S("cycle-against-time", 7, 2, 5, 751, [1, 5, 33, 104, 200, 408], [8, 132, 791, 2337, 5072]),  # closed orders [] twins 476 merges 2092
    S("cycle-against-time", 7, 3, 5, 856, [1, 5, 33, 104, 240, 473], [8, 132, 791, 2337, 6002]),  # closed orders [] twins 561 merges 2258
    S("revisited-anchor", 8, 2, None, 144, [1, 5, 30, 56, 32, 20, 0], [8, 132, 772, 1200, 825, 528]),  # closed orders None twins 24 merges 446
    S("revisited-anchor", 8, 3, None, 1196, [1, 5, 33, 93, 128, 175, 173, 212, 376], [8, 132, 900, 2315, 3585, 4957, 4886, 6961]),  # closed orders None twins 384 merges 3864
    S("mutual-at-reset", 4, 2, None, 1, [1], []),  # closed orders None twins 0 merges 0
    S("two-agent-mutual-compact", 6, 2, None, 100, [1, 3, 6, 12, 29, 40, 9], [6, 29, 61, 160, 345, 379]),  # closed orders None twins 10 merges 135
    S("gem-detour", 8, 2, None, 379, [1, 5, 13, 30, 62, 94, 76, 61, 37], [8, 51, 161, 430, 759, 1012, 775, 699], collect_gems=True),  # closed orders None twins 88 merges 625
    S("gem-detour", 8, 2, None, 212, [1, 5, 9, 21, 43, 55, 45, 17, 16], [8, 51, 112, 301, 524, 611, 395, 167]),  # closed orders None twins 60 merges 344
    S("six-mutual", 3, 2, None, 1536, [1, 47, 392, 1096], [64, 3561, 26972]),  # closed orders None twins 312 merges 7259
    S("six-mutual", 3, 3, 3, 1920, [1, 47, 436, 1436], [64, 3561, 29933]),  # closed orders [2] twins 520 merges 8749
    S("six-converge", 3, 2, None, 3300, [1, 39, 648, 2612], [64, 6296, 92900]),  # closed orders None twins 1664 merges 23958
    S("six-converge", 3, 3, 3, 4880, [1, 39, 728, 4112], [64, 6296, 110470]),  # closed orders [2] twins 3304 merges 33802
    S("ring-of-four", 6, 3, 6, 6194, [1, 11, 90, 290, 1182, 1179, 3441], [16, 684, 5796, 23280, 63924, 90017]),  # closed orders [] twins 2244 merges 50986
    S("ring-of-four", 6, 4, None, 5548, [1, 11, 90, 290, 1182, 1149, 2825], [16, 684, 5796, 23280, 63924, 85745]),  # closed orders None twins 1938 merges 48648
    # changed worlds
    S("closes-in-one-state", 8, 3, 4, 183, [1, 17, 33, 50, 82], [36, 321, 587, 979], changes=OFF2),  # closed orders [] twins 0 merges 434
    S("closes-in-one-state", 8, 3, 6, 108, [1, 12, 13, 8, 17, 22, 35], [36, 174, 104, 75, 139, 178], changes=RECOLOUR2),  # closed orders [2] twins 18 merges 89
]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "kat_cycles.json"), "w") as f:
        json.dump(dict(catalogue=CATALOGUE, maps=MAPS, searches=SEARCHES), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
