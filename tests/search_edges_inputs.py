"""The fixed inputs of tests/test_search_edges_cpu.py and tests/test_gpu_search_edges.py -- TEST INFRASTRUCTURE.  No new reference code:
every expectation comes from the three restatements over the oracle (tests/search_ref.py, policy_ref.py, helpgraph_ref.py); this
module only names the maps, builds the two derived ones and walks an `oracle.OracleBatch` the way a training loop walks a batch.

SIX            six agents: agents 0-3 stand above their exits, 4 and 5 walk a corridor that the beam of colour 5 crosses.
SIX_VARIANT    SIX with the exit below S4 and the floor above it swapped: the same shape, no plan within two steps.
LANES6         six lanes of one step each: all 5^6 = 15 625 codes of the reset state, 63 successors.
"""
import functools
from dataclasses import dataclass

import numpy as np

from tests import helpgraph_ref, policy_ref, search_ref

HG_CASES = helpgraph_ref.load_cases()
CATALOGUE = {c["name"]: c for c in search_ref.load_cases()["catalogue"]}
SIX = HG_CASES["maps"]["six-agents"]
LANES6 = " @ ".join(f"S{k} X" for k in range(6))
GEMS = "S0 . G .\n.  . . .\nX  . . G"  # tests/test_gpu_solver.py: GEMS


def text(name):
    return search_ref.map_text(CATALOGUE[name])


def _six_variant():
    rows = [line.split() for line in SIX.strip().splitlines()]
    assert rows[1][2] == "." and rows[2][2] == "X"
    rows[1][2], rows[2][2] = rows[2][2], rows[1][2]
    return "\n".join(" ".join(r) for r in rows)


SIX_VARIANT = _six_variant()

# ---- a pool that one mode overflows and another fits, on one handle
CAPACITY_MAP, CAPACITY_T_MAX = "convergent-2-tight", 5
SEARCH_POOL = 128                    # standard stores 363 states, no-cooperation 55
HELPGRAPH_POOL = 256                 # no-convergence-3 stores 505 records, no-convergence-2 245
HELPGRAPH_OVER, HELPGRAPH_FITS = ("no-convergence", 3), ("no-convergence", 2)

# ---- exact fit
EXACT_MAP, EXACT_T_MAX, EXACT_HORIZON = "single-laser-asymmetric", 6, 30

# ---- one policy handle built again and again: (horizon, collect_gems) in this order.  The third table is the largest, the fourth is
# cut at its horizon (UNKNOWN answers) and smaller than the one before it, the fifth drops the gem word from the identity again.
REBUILDS = [(7, False), (12, False), (12, True), (3, True), (12, False)]

# ---- lived-in batches
LIVED_ENVS, LIVED_STEPS, LIVED_SEED = 1000, 30, 3
ROLLOUT_CHUNKS = (7, 11, 12)         # fused steps per rollout() call; their sum is LIVED_STEPS
LIVED = {"single-laser-asymmetric": 30, "one-way-detour": 40}  # map -> horizon of a complete table
PADDED_MAP, PADDED_HORIZON, PADDED_STEPS = "three-agent-temporal-cycle", 15, 12


@dataclass
class Lived:
    """What an OracleBatch gives step by step under sampled actions with auto-reset: per step the joint actions taken [n, A], the
    expected steps_to_go [n], the environments that were reset at the start of the step, and the gem flags [n, G] after it."""
    actions: list
    want: list
    was_reset: list
    gems: list
    keys: list          # of the last step only: identity without the gem flags per environment, None where somebody is dead
    last_codes: list    # of the last step only: the joint-action code the table holds (all STAY where the answer is negative)
    root_steps: object


def expected_steps(ob, table, collect_gems):
    """int32 [n]: table[identity] where everybody is alive, DEAD_END elsewhere (a complete table holds every reachable such state)."""
    alive = ob.dump()["alive"].all(1)
    return np.array([table[search_ref.identity(ob.world(e), collect_gems)][0] if alive[e] else policy_ref.DEAD_END for e in range(ob.n)], np.int32)


@functools.lru_cache(maxsize=None)
def lived_in(map_text, horizon, collect_gems=False, steps=LIVED_STEPS, n=LIVED_ENVS, seed=LIVED_SEED):
    from oracle import oracle
    t = policy_ref.build(map_text, horizon, collect_gems)
    assert t.complete
    table = t.table
    ob = oracle.OracleBatch(map_text, n)
    out = Lived([], [], [], [], None, None, t.root_steps)
    for step in range(steps):
        res = ob.step(None, auto_reset=True, seed=seed, t=step, want_obs=False)
        out.actions.append(res["actions"].copy())
        out.was_reset.append((res["ev_count"] & 128) != 0)
        out.want.append(expected_steps(ob, table, collect_gems))
        out.gems.append(ob.dump()["gems"].astype(bool))
    alive = ob.dump()["alive"].all(1)
    out.keys = [search_ref.identity(ob.world(e), False) if alive[e] else None for e in range(n)]
    stay = policy_ref.code_of([policy_ref.STAY] * t.n_agents)
    out.last_codes = [table[search_ref.identity(ob.world(e), collect_gems)][1] if alive[e] else stay for e in range(n)]
    return out


def gem_word(flags):
    """The LLE_BUF_GEMS word of a row of collected flags: bit g = gem g."""
    return sum(1 << g for g, f in enumerate(flags) if f)


def answer_with_gems(table, key, word, n_gems):
    """What a lookup over a collect_gems table answers for the identity `key` (without gems) and the gem word `word`: the table's
    steps for that identity, UNKNOWN when it holds none -- a word with a bit beyond the map's gems is no state of any table."""
    if key is None:
        return policy_ref.DEAD_END
    if word >> n_gems:
        return policy_ref.UNKNOWN
    entry = table.get(key + (tuple(bool((word >> g) & 1) for g in range(n_gems)),))
    return policy_ref.UNKNOWN if entry is None else entry[0]
