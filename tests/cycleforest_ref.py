"""The fixed input sets of the cycle-forest tests (tests/test_cycleforest_cpu.py, tests/test_gpu_cycleforest.py) and their oracle: per
map `tests/cycles_ref.search` (the closed-trail search restated over the oracle), whose results are recorded in
tests/golden/kat_cycleforest.json by tests/golden/make_kat_cycleforest.py.

Every set is equally shaped: a smaller map sits in the bottom-right corner of a walled frame (`helpgraph_ref.embed`: the same world).
The map texts are those of tests/golden/kat_cycles.json.

Set T (6x7, 3 agents, 3 sources, t_max 8, orders 2 and 3): closes-in-one-state, cycle-against-time, paper-interdependent-3,
      three-agent-temporal-cycle, paper-fully-coupled-legacy, paper-fully-coupled, three-agent-with-two-agent-cycle.  The orders decide
      different things on the same forest, and some maps are solved at depth 5 while others walk all 8 levels.
Set F (7x9, 4 agents, 4 sources, t_max 6, orders 3 and 4): ring-of-four, sequence-4-with-mutual, ring-of-four with source 1 disabled:
      the full agent class 4.
Set X (4x8, 6 agents, 2 sources, t_max 3, orders 2 and 3): six-mutual, six-converge: 21 value words, a closed field in words of its own.
Set M (4x4, 2 agents, 2 sources, t_max 6, order 2): two-agent-mutual-compact unchanged, with source 1 disabled, with source 1
      recoloured to 0 -- one layout under three edge rules -- and mutual-at-reset, whose reset state already closes: 1 record.

A set may carry `changes`, one entry per map in the plain-data form of tests/helpgraph_ref.py (None: the map as its text gives it): the
oracle searches under them, the device is given `world_of(text, changes)`.
"""
import json
import os
from dataclasses import dataclass

from tests import cycles_ref, helpgraph_ref
from tests.helpforest_ref import OFF1, RECOLOUR1, world_of  # noqa: F401  (one meaning of the changes, re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
_CY = cycles_ref.load_cases()
MAPS = {c["name"]: c["map"] for c in _CY["catalogue"] if "map" in c}
MAPS.update(_CY["maps"])


@dataclass(frozen=True)
class InputSet:
    name: str
    names: tuple      # per map: the name in kat_cycles.json, with the label of its changes
    base: tuple       # per map: the name in kat_cycles.json
    maps: tuple
    t_max: int
    orders: tuple
    changes: tuple = None  # per map: `changes` of tests/helpgraph_ref.py, or None; None here: no map is changed

    def __post_init__(self):
        if self.changes is None:
            object.__setattr__(self, "changes", (None,) * len(self.maps))
        assert len(self.changes) == len(self.maps) == len(self.names) == len(self.base)

    @property
    def worlds(self):
        """What CycleForestSolver is given: the map text, or an lle_amd.World with the map's changes applied."""
        return [world_of(text, changes) for text, changes in zip(self.maps, self.changes)]


def _set(name, base, height, width, t_max, orders, changes=None):
    changes = (None,) * len(base) if changes is None else changes
    return InputSet(name, tuple(b + helpgraph_ref.changes_label(c) for b, c in zip(base, changes)), tuple(base),
                    tuple(helpgraph_ref.embed(MAPS[b], height, width) for b in base), t_max, orders, changes)


SET_T = _set("T", ("closes-in-one-state", "cycle-against-time", "paper-interdependent-3", "three-agent-temporal-cycle", "paper-fully-coupled-legacy",
                   "paper-fully-coupled", "three-agent-with-two-agent-cycle"), 6, 7, 8, (2, 3))
SET_F = _set("F", ("ring-of-four", "sequence-4-with-mutual", "ring-of-four"), 7, 9, 6, (3, 4), changes=(None, None, OFF1))
SET_X = _set("X", ("six-mutual", "six-converge"), 4, 8, 3, (2, 3))
SET_M = _set("M", ("two-agent-mutual-compact", "two-agent-mutual-compact", "two-agent-mutual-compact", "mutual-at-reset"), 4, 4, 6, (2,),
             changes=(None, OFF1, RECOLOUR1, None))
SETS = {s.name: s for s in (SET_T, SET_F, SET_X, SET_M)}

# what the issue states: {(set, map name, order): (length, stored records)}
STATED = {("T", "closes-in-one-state", 2): (5, 178), ("T", "closes-in-one-state", 3): (None, 131), ("T", "cycle-against-time", 2): (5, 751),
          ("T", "cycle-against-time", 3): (5, 856), ("T", "paper-interdependent-3", 2): (7, 191), ("T", "paper-interdependent-3", 3): (None, 188),
          ("T", "three-agent-temporal-cycle", 3): (None, 1047), ("T", "paper-fully-coupled-legacy", 3): (None, 11812),
          ("T", "paper-fully-coupled", 3): (None, 3962), ("F", "ring-of-four", 3): (6, 6194), ("F", "ring-of-four", 4): (None, 5548),
          ("X", "six-mutual", 3): (3, 1920), ("X", "six-converge", 3): (3, 4880), ("X", "six-mutual", 2): (None, 1536), ("X", "six-converge", 2): (None, 3300),
          ("M", "mutual-at-reset", 2): (None, 1)}


def single_search(name, t_max, order):
    """The search kat_cycles.json records for the unchanged map `name` at this horizon and order (gems not collected), or None."""
    for c in _CY["searches"]:
        if c["map"] == name and c["t_max"] == t_max and c["n"] == order and not c["collect_gems"] and "changes" not in c:
            return dict(length=c["length"], frontier=c["frontier"], expanded=c["expanded"], states=c["states"])
    return None


def stated_interdependent(name, t_max):
    """{order: boolean}: what the reference's catalogue states for is_interdependent of the layout `name` at the horizon t_max."""
    for c in _CY["catalogue"]:
        if c["name"] == name:
            return {int(k): v for k, v in c["expect"].get(str(t_max), {}).get("interdependent", {}).items()}
    return {}


def search(s, m, order):
    """The restatement's Result for map m of the set under no closed trail of `order`."""
    return cycles_ref.search(s.maps[m], s.t_max, order, changes=s.changes[m])


def row_of(r):
    return dict(length=r.length, frontier=list(r.frontier), expanded=list(r.expanded), states=r.n_states)


def load_golden():
    """tests/golden/kat_cycleforest.json: {set: {"order": [per map {length, frontier, expanded, states}]}}."""
    with open(os.path.join(HERE, "golden", "kat_cycleforest.json")) as f:
        return json.load(f)


def assert_map_equals_golden(s, i, ref, res, m, order):
    """Map m of the CycleForestResult `res` (map i of the set `s`) against its recorded entry `ref`: length, counters, stored records,
    the plan replayed on the oracle under the map's changes -- no closed trail of `order`, the closed orders below it, and the triples
    equal to the replay's."""
    length = None if res.length[m] < 0 else int(res.length[m])
    assert res.status[m] == 0, (m, res.status[m])
    assert length == ref["length"], (m, length, ref["length"])
    assert res.frontier[m] == ref["frontier"] and res.expanded[m] == ref["expanded"], (m, res.frontier[m], ref["frontier"], res.expanded[m], ref["expanded"])
    assert int(res.n_states[m]) == ref["states"] and int(res.depth_reached[m]) == len(ref["expanded"]), (m, res.n_states[m], ref["states"])
    assert (res.plans[m] is None) == (ref["length"] is None)
    if res.plans[m] is None:
        assert res.triples[m] is None and res.closed_orders[m] is None
        return
    cycles_ref.check_plan(s.maps[i], [[a.value for a in row] for row in res.plans[m]], order, length=ref["length"], changes=s.changes[i],
                          triples=res.triples[m], closed_orders=res.closed_orders[m])
