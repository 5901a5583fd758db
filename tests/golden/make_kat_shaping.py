"""Known-answer tests for potential-based reward shaping (PotentialShapedLLE) and the LaserSubgoal extras, hand-transcribed from
the reference's python/tests/test_reward_strategy.py:62-154, test_observations.py:410-497 and test_env.py:333-378.  Same rules as
make_kat.py: each case restates ONE reference test as data (map, configuration, script, the assertions that test makes; `ref` =
file:line); nothing here imports or executes the reference.

Running this file rewrites tests/golden/kat_shaping.json.

Configuration: {"multi_objective": bool,
                "pbrs": null | {"gamma": g, "reward_value": v, "lasers": null | [[i, j], ...], "with_extras": bool}
                        (Builder.pbrs, python/lle/env/builder.py:78-110: with_extras adds LaserSubgoal over the same sources),
                "add_extras": [...]  (Builder.add_extras: "laser_subgoal")}
Script ops: {"op": "reset", "extras": [[...] per agent] | null}        (Observation.extras of LLE.reset)
            {"op": "step", "actions": [...], "reward": r | [gem, exit, death, done, pbrs] | null, "done": bool | null,
             "extras_sums": [sum per agent] | null   (what the reference's test asserts),
             "extras": [[...] per agent] | null}     (derived: the matrix those sums come from)
Static expectations: "extras_shape": [E] | null, "objectives": [...] | null.
Rewards are Python floats, computed here in double exactly as the reference's tests write them; the reference compares its
float32 reward with them under numpy's weak-scalar rule, i.e. as float32(expected).
Codes: actions N=0 S=1 E=2 W=3 STAY=4.  REWARD_EXIT = REWARD_DONE = 1 (python/lle/env/reward_strategy.py:22-25).
"""
import json
import os

N, S, E, W, STAY = 0, 1, 2, 3, 4
REWARD_EXIT = REWARD_DONE = 1.0
CASES = []


def case(name, ref, map, script, multi_objective=False, pbrs=None, add_extras=(), extras_shape=None, objectives=None):
    CASES.append({"name": name, "ref": ref, "map": map, "multi_objective": multi_objective, "pbrs": pbrs, "add_extras": list(add_extras),
                  "extras_shape": extras_shape, "objectives": objectives, "script": script})


def pbrs(gamma=0.99, reward_value=0.5, lasers=None, with_extras=True):  # the defaults of Builder.pbrs (builder.py:78-84)
    return {"gamma": gamma, "reward_value": reward_value, "lasers": lasers, "with_extras": with_extras}


def reset(extras=None):
    return {"op": "reset", "extras": extras}


def step(actions, reward=None, done=None, extras_sums=None, extras=None):
    return {"op": "step", "actions": list(actions), "reward": reward, "done": done, "extras_sums": extras_sums, "extras": extras}


MAP_ONE = "\n                S0 .  .\n                .  . L0W\n                X  .  ."
GAMMA, VALUE = 0.99, 0.5

# the strategy is built around a freshly reset world and never reset itself: what LLE.reset leaves
case("pbrs_single_objective", "python/tests/test_reward_strategy.py:62-86", MAP_ONE,
     [reset(), step([E], GAMMA * VALUE - VALUE), step([S], VALUE * GAMMA), step([S], 0.0)], pbrs=pbrs(GAMMA, VALUE, with_extras=False))
case("pbrs_multi_objective", "python/tests/test_reward_strategy.py:107-136", MAP_ONE,
     [reset(), step([E], [0.0] * 4 + [GAMMA * VALUE - VALUE]), step([S], [0.0] * 4 + [VALUE * GAMMA]), step([S], [0.0] * 4 + [0.0])],
     multi_objective=True, pbrs=pbrs(GAMMA, VALUE, with_extras=False), objectives=["gem", "exit", "death", "done", "PBRS"])
# `.multi_objective().pbrs()` succeeds (test_reward_strategy.py:89-94); the other order raises ValueError (:96-104): here the
# contradiction is multi_objective=True around a PotentialShapedLLE over SingleObjective (tests/test_shaping_cpu.py)
case("pbrs_after_multi_objective", "python/tests/test_reward_strategy.py:89-94", MAP_ONE, [reset()], multi_objective=True, pbrs=pbrs(),
     objectives=["gem", "exit", "death", "done", "PBRS"], extras_shape=[1])
case("pbrs_with_lle", "python/tests/test_reward_strategy.py:139-154", MAP_ONE,
     [reset(), step([E], 0.5 * 0.99 - 0.5), step([S], 0.5 * 0.99 - 0), step([S], 0.0)], pbrs=pbrs(gamma=0.99, reward_value=0.5))

MAP_EXTRAS_ONE = "\n                       S0  X\n                       .  L0W"
_one = [reset([[0.0]]), reset([[0.0]])]
case("subgoal_extras_one_laser", "python/tests/test_observations.py:410-428", MAP_EXTRAS_ONE, _one, add_extras=["laser_subgoal"], extras_shape=[1])
case("pbrs_subgoals_extras_one_laser", "python/tests/test_observations.py:431-441", MAP_EXTRAS_ONE, _one, pbrs=pbrs(with_extras=True),
     extras_shape=[1])

MAP_EXTRAS_TWO = "\n                       S0  S1 X  X\n                       .   .  . L0W\n                       .   .  . L1W"
_two = [reset([[0.0, 0.0], [0.0, 0.0]]),
        step([S, STAY], extras_sums=[1.0, 0.0], extras=[[1.0, 0.0], [0.0, 0.0]]),
        step([N, STAY], extras_sums=[1.0, 0.0], extras=[[1.0, 0.0], [0.0, 0.0]]),
        # "Even when an agent dies, the subgoal is reached" (:463-469): agent 1 walks into agent 0's beam
        step([STAY, S], done=True, extras_sums=[1.0, 1.0], extras=[[1.0, 0.0], [1.0, 0.0]])]
case("pbrs_subgoals_extras_two_lasers_two_agents", "python/tests/test_observations.py:444-483", MAP_EXTRAS_TWO, _two * 2, pbrs=pbrs(with_extras=True),
     extras_shape=[2])
case("extras_subgoals_extras_two_lasers_two_agents", "python/tests/test_observations.py:444-469,486-497", MAP_EXTRAS_TWO, _two * 2,
     add_extras=["laser_subgoal"], extras_shape=[2])

SHAPED_REWARD = 1.0
_episode = [reset(), step([S], SHAPED_REWARD), step([E], 0.0), step([S], 0.0), step([W], REWARD_EXIT + REWARD_DONE)]
case("pbrs_reset_between_two_episodes", "python/tests/test_env.py:333-364", "\n                       S0 .  .\n                       .  . L0W\n                       X  .  .",
     _episode * 5, pbrs=pbrs(reward_value=SHAPED_REWARD, gamma=1.0))
case("pbrs_not_all_lasers", "python/tests/test_env.py:367-378",
     "\n                       S0 .  .\n                       .  . L0W\n                       .  . L0W\n                       X  .  .",
     [reset()], pbrs=pbrs(lasers=[[1, 2]]), extras_shape=[1])

if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_shaping.json")
    with open(out, "w") as f:
        json.dump({"cases": CASES}, f, indent=1)
        f.write("\n")
    print(f"wrote {len(CASES)} cases to {out}")
