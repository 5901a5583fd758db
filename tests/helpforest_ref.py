"""The fixed input sets of the help-forest tests (tests/test_helpforest_cpu.py, tests/test_gpu_helpforest.py) and their oracle: per map
`tests/helpgraph_ref.search` (the modes over the flattened help relation) or `tests/trails_ref.search` (no-sequence-N), whose results are
recorded in tests/golden/kat_helpforest.json by tests/golden/make_kat_helpforest.py.

Every set is equally shaped: a smaller map sits in the bottom-right corner of a walled frame (`helpgraph_ref.embed`: the same world).
The named maps are those of tests/golden/kat_helpgraph.json and tests/golden/kat_trails.json.

Set S (4x6, 3 agents, 1 source, t_max 6): divergent-2-tight, divergent-2-with-detour and the six maps of forest_ref.SET_C.  The modes
      decide something here: no-divergence-2 and no-asymmetric take the plan of the first map away, the second keeps one of 6 steps
      under no-divergence-2 only, and no-asymmetric turns one generated map from solved to unsolved; two generated maps have no plan.
Set P (5x9, 2 agents, 2 sources, t_max 8): two-agent-mutual-compact, two-agent-mutual-with-detours and six generated 5x5 maps.
      no-mutual = no-sequence-2 on two agents; no-sequence-3 stores other records than standard (the trail word joins the identity).
Set R (6x6, 3 agents, 2 sources, t_max 5): convergent-2-tight, paper-convergent-2, chain-in-one-state, chain-at-reset,
      decreasing-times: no-convergence-2/3 and no-sequence-2/3, with a reset state that already holds a trail.
Set Q (6x6, 3 agents, 3 sources, t_max 10): paper-fully-coupled, paper-fully-coupled-legacy, for no-fully-coupled.
Set X (4x8, 6 agents, 2 sources, t_max 3): six-mutual, six-converge: the second help word, the sixth trail field.
Set G (4x5, 2 agents, 2 sources, 1 gem, t_max 8): gem-detour, shared-colour, searched with collect_gems=True.
Set L (4x6, 2 agents, 2 sources, t_max 24): long-trails, long-trails with source 1 disabled, two-agent-mutual-compact: no-sequence-8,
      -15 and -16 store trail fields up to 15 in the first map, which walks N + 5 levels until its frontier runs empty while the third is
      solved at depth 5; the second differs from the first by its edge rule alone.
Set C (4x4, 2 agents, 2 sources, t_max 8): two-agent-mutual-compact four times -- unchanged, source 1 disabled, source 0 disabled,
      source 1 recoloured to 0: ONE layout, four edge rules, four different (length, records) under no-sequence-2.

A set may carry `changes`, one entry per map in the plain-data form of tests/helpgraph_ref.py (None: the map as its text gives it): the
oracle searches `oracle_world(text, changes)`, the device is given `world_of(text, changes)`.
"""
import json
import os
from dataclasses import dataclass

from lle_amd import mapgen
from tests import forest_ref, helpgraph_ref, trails_ref

HERE = os.path.dirname(os.path.abspath(__file__))
_HG, _TR = helpgraph_ref.load_cases(), trails_ref.load_cases()
CATALOGUE = {c["name"]: c for c in _TR["catalogue"] + _HG["catalogue"] if "map" in c}
MAPS = {name: c["map"] for name, c in CATALOGUE.items()}
MAPS.update(_HG["maps"])
MAPS.update(_TR["maps"])  # (the maps both files hold are the same text)


@dataclass(frozen=True)
class InputSet:
    name: str
    names: tuple      # per map: the catalogue name, or "<generator>-<seed>"
    maps: tuple
    t_max: int
    modes: tuple      # (mode, param) of helpgraph_ref.MODES, or ("no-sequence", N)
    collect_gems: bool = False
    changes: tuple = None  # per map: `changes` of tests/helpgraph_ref.py, or None; None here: no map is changed

    def __post_init__(self):
        if self.changes is None:
            object.__setattr__(self, "changes", (None,) * len(self.maps))
        assert len(self.changes) == len(self.maps) == len(self.names)

    @property
    def worlds(self):
        """What HelpForestSolver is given: the map text, or an lle_amd.World with the map's changes applied."""
        return [world_of(text, changes) for text, changes in zip(self.maps, self.changes)]


def embed_top_left(text, height, width):
    """The map `text` in the TOP-LEFT corner of a height x width map of walls: the same world as `helpgraph_ref.embed` gives, on the
    other end of the cell table."""
    rows = [line.split() for line in text.strip().splitlines()]
    h, w = len(rows), len(rows[0])
    assert all(len(r) == w for r in rows) and h <= height and w <= width
    return "\n".join(" ".join(rows[i][j] if i < h and j < w else "@" for j in range(width)) for i in range(height))


def _named(names, height, width):
    return tuple(helpgraph_ref.embed(MAPS[n], height, width) for n in names)


_S_NAMES = ("divergent-2-tight", "divergent-2-with-detour")
_P_NAMES = ("two-agent-mutual-compact", "two-agent-mutual-with-detours")
_P_GENERATED = tuple(mapgen.generate(5, 5, 2, 2, 0, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s) for s in range(6))
_R_NAMES = ("convergent-2-tight", "paper-convergent-2", "chain-in-one-state", "chain-at-reset", "decreasing-times")
_Q_NAMES = ("paper-fully-coupled", "paper-fully-coupled-legacy")
_X_NAMES = ("six-mutual", "six-converge")
_G_NAMES = ("gem-detour", "shared-colour")

SET_S = InputSet("S", _S_NAMES + tuple(f"set-c-{s}" for s in range(6)), _named(_S_NAMES, 4, 6) + tuple(helpgraph_ref.embed(t, 4, 6) for t in forest_ref.SET_C.maps), 6,
                 (("standard", 2), ("no-divergence", 2), ("no-asymmetric", 2)))
SET_P = InputSet("P", _P_NAMES + tuple(f"generated-{s}" for s in range(6)), _named(_P_NAMES, 5, 9) + tuple(helpgraph_ref.embed(t, 5, 9) for t in _P_GENERATED), 8,
                 (("standard", 2), ("no-mutual", 2), ("no-sequence", 2), ("no-sequence", 3)))
SET_R = InputSet("R", _R_NAMES, _named(_R_NAMES, 6, 6), 5, (("standard", 2), ("no-convergence", 2), ("no-convergence", 3), ("no-sequence", 2), ("no-sequence", 3)))
SET_Q = InputSet("Q", _Q_NAMES, _named(_Q_NAMES, 6, 6), 10, (("no-fully-coupled", 2),))
SET_X = InputSet("X", _X_NAMES, _named(_X_NAMES, 4, 8), 3, (("standard", 2), ("no-mutual", 2), ("no-convergence", 2), ("no-sequence", 2), ("no-sequence", 3)))
SET_G = InputSet("G", _G_NAMES, _named(_G_NAMES, 4, 5), 8, (("standard", 2), ("no-asymmetric", 2), ("no-sequence", 3)), collect_gems=True)
OFF0 = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}]}
OFF1 = {"sources": [{"laser_id": 1, "enabled": False, "colour": None}]}
RECOLOUR1 = {"sources": [{"laser_id": 1, "enabled": None, "colour": 0}]}
_L_NAMES = ("long-trails", "long-trails", "two-agent-mutual-compact")
SET_L = InputSet("L", ("long-trails", "long-trails-source1-off", "two-agent-mutual-compact"), _named(_L_NAMES, 4, 6), 24,
                 (("no-sequence", 8), ("no-sequence", 15), ("no-sequence", 16), ("standard", 2)), changes=(None, OFF1, None))
SET_C = InputSet("C", tuple("two-agent-mutual-compact" + helpgraph_ref.changes_label(c) for c in (None, OFF1, OFF0, RECOLOUR1)),
                 _named(("two-agent-mutual-compact",) * 4, 4, 4), 8, (("standard", 2), ("no-mutual", 2), ("no-sequence", 2), ("no-sequence", 3)),
                 changes=(None, OFF1, OFF0, RECOLOUR1))
SETS = {s.name: s for s in (SET_S, SET_P, SET_R, SET_Q, SET_X, SET_G, SET_L, SET_C)}

# what the issue states for the catalogue maps of S and P: (length, stored records) of map 0 and map 1
S_STATED = {("standard", 2): ((2, 73), (2, 102)), ("no-divergence", 2): ((None, 252), (6, 1408)), ("no-asymmetric", 2): ((None, 480), (None, 1954))}
P_STATED = {("standard", 2): ((5, 123), (4, 237)), ("no-mutual", 2): ((None, 100), (8, 1225)), ("no-sequence", 2): ((None, 100), (8, 1225)),
            ("no-sequence", 3): ((5, 119), (4, 232))}


def stated(name, t_max):
    """What the reference's catalogue states for the layout `name` at the horizon t_max, both golden files merged: a dict with some of
    asymmetric, fully_coupled (booleans), convergent, divergent, interdependent, sequential ({"k": boolean}); {} where it states nothing."""
    out = {}
    for cases in (_HG, _TR):
        for c in cases["catalogue"]:
            if c["name"] == name:
                for key, value in c["expect"].get(str(t_max), {}).items():
                    if isinstance(value, dict):
                        out.setdefault(key, {}).update(value)
                    else:
                        out[key] = value
    return out


def mode_text(mode, param=2):
    """The solve mode's text as lle_amd parses it."""
    return f"{mode}-{param}" if mode in ("no-convergence", "no-divergence", "no-sequence") else mode


def world_of(text, changes=None):
    """The map for a solver of lle_amd: its text, or -- changed -- an lle_amd.World with `changes` applied through its public mutators."""
    if changes is None:
        return text
    from lle_amd import World
    return helpgraph_ref.apply_changes(World(text), changes)


def search(text, t_max, mode, param=2, collect_gems=False, changes=None):
    """The restatement's Result for one map: trails_ref for no-sequence, helpgraph_ref otherwise."""
    if mode == "no-sequence":
        return trails_ref.search(text, t_max, param, collect_gems, changes=changes)
    return helpgraph_ref.search(text, t_max, mode, param, collect_gems, changes=changes)


def check_plan(text, plan, mode, param=2, collect_gems=False, length=None, changes=None):
    """Replay `plan` under the mode (and the map's changes); returns what the goal's record must carry: the set of help edges, or the
    tuple L."""
    if mode == "no-sequence":
        return trails_ref.check_plan(text, plan, param, collect_gems, length=length, changes=changes)
    return helpgraph_ref.check_plan(text, plan, mode, param, collect_gems, length=length, changes=changes)


def load_golden():
    """tests/golden/kat_helpforest.json: {set: {"mode/param": [per map {length, frontier, expanded, states}]}}."""
    with open(os.path.join(HERE, "golden", "kat_helpforest.json")) as f:
        return json.load(f)


def golden_key(mode, param):
    return f"{mode}/{param}"


def assert_map_equals_golden(text, ref, res, m, mode, param, collect_gems=False, changes=None):
    """Map m of the HelpForestResult `res` against its recorded entry `ref`: length, counters, stored records, the plan replayed (on the
    oracle world under `changes`) and the goal's help edges or trail equal to the replay's."""
    length = None if res.length[m] < 0 else int(res.length[m])
    assert res.status[m] == 0, (m, res.status[m])
    assert length == ref["length"], (m, length, ref["length"])
    assert res.frontier[m] == ref["frontier"] and res.expanded[m] == ref["expanded"], (m, res.frontier[m], ref["frontier"], res.expanded[m], ref["expanded"])
    assert int(res.n_states[m]) == ref["states"] and int(res.depth_reached[m]) == len(ref["expanded"]), (m, res.n_states[m], ref["states"])
    assert (res.plans[m] is None) == (ref["length"] is None)
    if res.plans[m] is None:
        assert res.help_edges[m] is None and res.trail[m] is None
        return
    carried = check_plan(text, [[a.value for a in row] for row in res.plans[m]], mode, param, collect_gems, length=ref["length"], changes=changes)
    if mode == "no-sequence":
        assert tuple(res.trail[m]) == tuple(carried) and res.help_edges[m] is None, (m, res.trail[m], carried)
    else:
        assert res.help_edges[m] == carried and res.trail[m] is None, (m, res.help_edges[m], carried)
