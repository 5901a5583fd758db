"""The forest of steps-to-go tables (liblle_policyforest.so) restated without a GPU: the table of map m in a forest IS the single
table of that map, so this module only loops `tests/policy_ref.build` (cached per (map, horizon, collect_gems)) over a fixed set of
`tests/forest_ref.py` and lays the states out for a batch of several maps: state k of map m in environment m * E_c + k, spare
environments at the reset state.
"""
import functools

import numpy as np

from tests import policy_ref
from tests.forest_ref import SET_A, SET_B, SET_C, SETS  # noqa: F401  (the tests take the sets from here)

UNKNOWN, DEAD_END, STAY = policy_ref.UNKNOWN, policy_ref.DEAD_END, policy_ref.STAY
HORIZONS = (6, 40)

# What the restatement gives for the sets (pinned by tests/test_policyforest_cpu.py, so the GPU tests cannot pass on empty ground).
A40_N_STATES = [135, 123, 183, 198, 146, 211, 165, 183, 76, 210, 146, 198, 160, 81, 106, 198]
A6_N_STATES = [117, 116, 182, 159, 145, 70, 111, 111, 53, 210, 96, 189, 132, 72, 105, 150]
A6_ROOTS = [4, 6, 5, 6, 3, None, 5, None, None, 1, 6, 5, 2, None, 3, 5]
A40_UNSOLVABLE, A6_NO_PLAN, B40_UNSOLVABLE, B6_COMPLETE = [8, 13], [5, 7, 8, 13], [5, 8, 14], {1: (46, 6), 13: (24, 5)}
C40_N_STATES, C6_N_STATES = [1386, 34, 920, 1452, 1232, 920], [466, 34, 776, 926, 733, 322]


@functools.lru_cache(maxsize=None)
def tables(name, horizon, collect_gems=False):
    """[policy_ref.Table] per map of the set."""
    return tuple(policy_ref.build(text, horizon, collect_gems) for text in SETS[name].maps)


def root_answer(t):
    """What a lookup gives for the reset state of table t (an int: steps, UNKNOWN or DEAD_END)."""
    return t.answer(t.states[0])[0]


def envs_per_map(ts):
    return max(t.n_states for t in ts)


@functools.lru_cache(maxsize=None)
def expected(name, horizon, collect_gems=False, E_c=None):
    """(steps int32 [M * E_c], actions uint8 [M * E_c, A]) of a batch with state k of map m in environment m * E_c + k and the reset
    state in the spare ones; E_c: the largest state count of the set, or smaller -- then the first E_c states of every map."""
    ts = tables(name, horizon, collect_gems)
    E_c = envs_per_map(ts) if E_c is None else E_c
    A = ts[0].n_agents
    steps, actions = np.zeros(len(ts) * E_c, np.int32), np.zeros((len(ts) * E_c, A), np.uint8)
    for m, t in enumerate(ts):
        for k in range(E_c):
            s, code = t.answer(t.states[k if k < t.n_states else 0])
            steps[m * E_c + k], actions[m * E_c + k] = s, policy_ref.joint_of(code, A)
    return steps, actions


def replay_rows(ts, E_c):
    """The joint actions that bring a freshly reset batch to the layout of `expected`: a list over steps of uint8 [M * E_c, A] arrays,
    prefixes padded with all-STAY rows (which lead back to the same state: tests/test_policy_ref_cpu.py)."""
    A = ts[0].n_agents
    chosen = [[t.states[k if k < t.n_states else 0] for k in range(E_c)] for t in ts]
    longest = max(len(s.prefix) for row in chosen for s in row)
    out = []
    for step in range(longest):
        rows = np.full((len(ts) * E_c, A), STAY, np.uint8)
        for m, row in enumerate(chosen):
            for k, s in enumerate(row):
                if step < len(s.prefix):
                    rows[m * E_c + k] = s.prefix[step]
        out.append(rows)
    return out


def kinds(t):
    """(exact, no plan known, plan known but beyond the horizon, dead end) answer counts over the states of table t."""
    answers = [t.answer(s)[0] for s in t.states]
    exact = sum(a >= 0 for a in answers)
    dead = sum(a == DEAD_END for a in answers)
    no_plan = sum(s.steps is None for s in t.states) - dead
    return exact, no_plan, len(answers) - exact - no_plan - dead, dead


# ---- sampled mid-episode states (the expert rollouts of tests/test_gpu_policyforest.py)
ROLLOUT = dict(name="A", horizon=40, seed=2, steps=5, envs_per_map=64)


@functools.lru_cache(maxsize=None)
def sampled_answers(name, horizon, seed, n_steps, E, auto_reset=False):
    """What a batch of E environments per map of the set holds after n_steps sampled steps of (seed, t = 0 .. n_steps - 1), by the
    oracle: (answers int32 [M * E] of the restatement -- DEAD_END where an agent is dead --, everybody alive bool [M * E])."""
    from oracle import oracle
    from tests.search_ref import identity
    ts = tables(name, horizon)
    steps, alive = np.zeros(len(ts) * E, np.int32), np.zeros(len(ts) * E, bool)
    for m, t in enumerate(ts):
        ob = oracle.OracleBatch(t.text, E)
        for k in range(n_steps):  # (a sampled action is drawn from (seed, global environment index, t))
            ob.step(None, auto_reset=auto_reset, seed=seed, t=k, env_offset=m * E, want_obs=False)
        live = ob.dump()["alive"].all(1)
        table = t.table
        for e in range(E):
            alive[m * E + e] = live[e]
            steps[m * E + e] = table[identity(ob.world(e), t.collect_gems)][0] if live[e] else DEAD_END
    return steps, alive


def rollout_classes(steps, alive, E):
    """(environments with an answer >= 0, DEAD_END with a dead agent, DEAD_END with everybody alive, anything else)."""
    exact, dead_agent = int((steps >= 0).sum()), int((~alive).sum())
    dead_map = int(((steps == DEAD_END) & alive).sum())
    return exact, dead_agent, dead_map, len(steps) - exact - dead_agent - dead_map
