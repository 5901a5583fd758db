"""BatchedLLE with reward_strategy= / extras_generator= (the shaping kernel, lle_amd/shaping/shaping.hip) against the per-env numpy
restatement of the reference's PotentialShapedLLE and LaserSubgoal on oracle worlds (tests/oracle_shaping.py): the reference's own
tests (tests/golden/kat_shaping.json) and differential rollouts, compared EXACTLY (torch.equal) on reward and extras at every step.

The rollouts' actions come from the oracle side (uniform over each agent's available actions, numpy generator), so a rollout is
the same on every box; `play(..., gpu=False)` runs the oracle side alone -- seeds and lengths below were chosen with it so that
every rollout sees auto-resets and deaths, which each rollout then asserts."""
import numpy as np
import pytest

from oracle.levels import LEVELS
from tests import oracle_shaping
from tests.oracle_shaping import SHAPING_MAPS, OracleShapedLLE
from tests.parity_util import EXTRA_MAPS, LONG_MAPS

pytestmark = pytest.mark.gpu

CASES = oracle_shaping.load_cases()
PARAMS = [(0.99, 0.5), (1.0, 1.0), (0.9, 0.3)]


def _text(name):
    if name.startswith("level"):
        return LEVELS[int(name[-1])]
    for d in (EXTRA_MAPS, LONG_MAPS, SHAPING_MAPS):
        if name in d:
            return d[name]
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------- the reference's own tests
class _BatchedAdapter:
    def __init__(self, case):
        from lle_amd import BatchedLLE, LaserSubgoal, MultiGenerator, MultiObjective, PotentialShapedLLE, SingleObjective
        self.n = 70  # every env plays the same script; all must agree, the first is returned
        pb = case["pbrs"]
        tup = lambda ps: None if ps is None else [tuple(p) for p in ps]  # noqa: E731
        base = MultiObjective() if case["multi_objective"] else SingleObjective()
        strategy = base if pb is None else PotentialShapedLLE(base, None, pb["gamma"], pb["reward_value"], tup(pb["lasers"]))
        gens = [LaserSubgoal(None, tup(g)) for g in oracle_shaping.case_generators(case)]
        extras = None if not gens else gens[0] if len(gens) == 1 else MultiGenerator(*gens)  # builder.py:142-145
        self.env = BatchedLLE(case["map"], self.n, reward_strategy=strategy, extras_generator=extras)
        self.extras_shape, self.objectives = self.env.extras_shape, self.env.objectives

    def _same(self, t):
        a = t.cpu().numpy()
        assert all(np.array_equal(a[0], a[k]) for k in range(1, self.n))
        return a[0]

    def reset(self):
        self.env.reset()
        return self._same(self.env.extras())

    def step(self, actions):
        import torch
        out = self.env.step(torch.tensor([actions] * self.n, dtype=torch.uint8))
        assert int(out["err"].max()) == 0
        assert ("extras" in out) == (self.env.extras_generator is not None)
        extras = out["extras"] if "extras" in out else self.env.extras()
        assert out["reward"].dtype == torch.float32 and extras.dtype == torch.float32
        return self._same(out["reward"]), bool(self._same(out["done"])), self._same(extras)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_shaping_kat_through_batched_lle(case):
    oracle_shaping.run_case(_BatchedAdapter, case)


# ---------------------------------------------------------------------------------------------- differential rollouts
def play(oracle_mod, maps, per_map, steps, seed, multi_objective=False, params=(0.99, 0.5), lasers="all", extras="all", randomize=False,
         step_kw=None, reset_by="auto", set_state_at=None, lockstep=None, gpu=True, need_events=True, rewards_seen=None):
    """One rollout of a batch of len(maps) * per_map environments (map m owns block m) against one OracleShapedLLE per environment.
    lasers / extras: "all", None (no shaping / no generator) or a list of laser_ids (pbrs: in that order, duplicates kept).
    reset_by: "auto" = step(auto_reset=True); "mask" = reset(env_mask=done) ahead of a plain step.
    set_state_at: step index at which every environment is handed a state through set_state -- its own state of ten steps before
    where World.set_state accepts it, its start state otherwise.
    lockstep: k -> only k oracle environments are played; environment e of the batch gets the actions of oracle environment e % k
    and must return its results (batches too large for one oracle world each).
    rewards_seen: a list that receives the oracle side's rewards of every step (numpy [k, width]).
    Returns (resets, deaths) seen by the oracle side."""
    texts = [m if (" " in m or "\n" in m) else _text(m) for m in maps]  # names, or map texts
    n = per_map * len(texts)
    k = n if lockstep is None else lockstep
    assert lockstep is None or (len(texts) == 1 and not randomize)
    step_kw = dict(step_kw or {})
    gamma, value = params
    worlds = [oracle_mod.OracleWorld(texts[(e * len(texts)) // k if lockstep is None else 0]) for e in range(k)]
    L, A, G = worlds[0].n_sources, worlds[0].n_agents, worlds[0].n_gems
    every = list(range(L))
    pbrs_ids = None if lasers is None else every if lasers == "all" else list(lasers)
    extras_ids = None if extras is None else every if extras == "all" else list(extras)
    refs = [OracleShapedLLE(w, pbrs=None if pbrs_ids is None else dict(gamma=gamma, reward_value=value, lasers=pbrs_ids),
                            extras=[] if extras_ids is None else [extras_ids], multi_objective=multi_objective) for w in worlds]
    for r in refs:
        r.free_running = True
    start_avail = [r.w.available_actions() for r in refs]
    start_pos = [r.w.start_pos for r in refs]
    rng = np.random.default_rng(seed)
    env = None
    if gpu:
        import torch

        from lle_amd import BatchedLLE, MultiObjective, PotentialShapedLLE, SingleObjective

        class _Src:  # "objects with .laser_id"
            def __init__(self, l):
                self.laser_id = l
        base = MultiObjective() if multi_objective else SingleObjective()
        strategy = base if pbrs_ids is None else PotentialShapedLLE(base, None, gamma, value, None if lasers == "all" else [_Src(l) for l in pbrs_ids])
        from lle_amd import LaserSubgoal
        generator = None if extras_ids is None else "laser_subgoal" if extras == "all" else LaserSubgoal(None, [_Src(l) for l in extras_ids])
        env = BatchedLLE(texts if len(texts) > 1 else texts[0], n, randomize_lasers=randomize, seed=seed, reward_strategy=strategy,
                         extras_generator=generator)
        first_words = env.world.map.source_first_words()
        width = (5 if pbrs_ids is not None else 4) if multi_objective else 1
        assert env.extras_shape == (0 if extras_ids is None else len(extras_ids),)
        if extras_ids is not None:
            assert env.extras_meanings == refs[0].extras_meanings

    def colours_now():
        return env.world.src_colour.cpu().numpy()[:, first_words] if L else np.zeros((n, 0), np.uint8)

    def compare(out, rewards, where):
        if not gpu:
            return
        want_e = np.stack([r.compute_extras() for r in refs])
        got_e = (out["extras"] if out is not None and "extras" in out else env.extras())
        assert got_e.dtype == torch.float32 and tuple(got_e.shape) == (n, A, want_e.shape[2])
        idx = torch.arange(n) % k
        assert torch.equal(got_e.cpu(), torch.from_numpy(want_e)[idx]), f"{where}: extras differ"
        if out is not None:
            assert (out.get("extras") is not None) == (extras_ids is not None)
            want_r = torch.from_numpy(np.stack(rewards))[idx]
            got_r = out["reward"].cpu()
            assert got_r.dtype == torch.float32 and tuple(got_r.shape) == (n, width)
            if not torch.equal(got_r, want_r):
                bad = int((got_r != want_r).any(dim=1).nonzero()[0])
                raise AssertionError(f"{where}: reward differs in env {bad}: {got_r[bad].tolist()} != {want_r[bad].tolist()}")
            assert torch.equal(out["done"].cpu(), torch.tensor([r.done for r in refs])[idx]), f"{where}: done differs"
            assert int(out["err"].max()) == 0, where

    if gpu:
        env.reset()
        cols = colours_now() if randomize else None
    for e, r in enumerate(refs):
        r.reset(cols[e] if gpu and randomize else None)
    if not gpu:
        for r in refs:
            r.compute_extras()
    compare(None, None, "after reset")
    resets = deaths = 0
    history = []
    for t in range(steps):
        over = np.array([r.done for r in refs])
        resets += int(over.sum())
        actions = np.zeros((k, A), np.uint8)
        for e, r in enumerate(refs):
            lists = start_avail[e] if over[e] else r.w.available_actions()
            for a in range(A):
                actions[e, a] = lists[a][int(rng.integers(len(lists[a])))]
        out = None
        if gpu:
            acts = torch.from_numpy(actions[np.arange(n) % k]).cuda()
            if reset_by == "mask":
                if over.any():
                    env.reset(env_mask=torch.from_numpy(over[np.arange(n) % k].astype(np.uint8)).cuda())
                out = env.step(acts, **step_kw)
            else:
                out = env.step(acts, auto_reset=True, **step_kw)
            cols = colours_now() if randomize else None
        rewards = []
        for e, r in enumerate(refs):
            if over[e]:
                r.reset(cols[e] if gpu and randomize else None)
                r.compute_extras()  # (LLE.reset returns the observation, whose extras mark the agents at their start cells)
            before = r.n_deads
            rewards.append(r.step(actions[e])[0])
            deaths += r.n_deads - before
        compare(out, rewards, f"t={t}")
        if rewards_seen is not None:
            rewards_seen.append(np.stack(rewards))
        if set_state_at is not None:
            history.append([(r.w.positions(), r.w.gems_collected(), all(r.w.alive()) and not r.done) for r in refs])
        if set_state_at is not None and t == set_state_at:
            states = []
            for e, r in enumerate(refs):
                pos, gems, fine = history[max(0, t - 10)][e]
                if fine:
                    probe = oracle_mod.OracleWorld(r.w.map_str)
                    try:
                        probe.set_state(pos, gems, [True] * A)
                    except oracle_mod.OracleError:
                        fine = False
                states.append((pos, gems) if fine else (start_pos[e], [False] * G))
            if gpu:
                sel = np.arange(n) % k
                err = env.set_state(torch.tensor([states[e][0] for e in sel], dtype=torch.uint8),
                                    torch.tensor([states[e][1] for e in sel], dtype=torch.bool).reshape(n, G))
                assert int(err.max()) == 0
            for e, r in enumerate(refs):
                r.set_state(states[e][0], states[e][1], [True] * A)
            # (the reference leaves the extras generator alone in set_state: the next compare marks both sides where the agents stand now)
            compare(None, None, f"after set_state at t={t}")
    if need_events:
        assert resets > 0 and deaths > 0, f"the rollout saw {resets} resets and {deaths} deaths: it proves nothing about them"
    return resets, deaths


# (name, steps, seed).  A seed per map (11 + its index).  With those seeds play(gpu=False) counts at least 20 resets and 20 deaths within
# the first 60 steps on every map (fewest: level3 with 21 / 22, level4 36 / 37, level5 64 / 66, level6 71 / 77; the others 100 to
# 1 500); a rollout extends its shorter self (same generator), so any length from 60 on keeps the in-rollout assertion true.  The
# lengths are a few hundred steps as the episodes of a map are long: 400 on the levels, whose episodes last longest, 200 elsewhere.
ROLLOUT_MAPS = [("level3", 400, 11), ("level4", 400, 12), ("level5", 400, 13), ("level6", 400, 14), ("nested", 200, 15), ("three_beams", 200, 16),
                ("four_layers", 200, 17), ("three_beam_cell", 200, 18), ("long_crossing", 200, 19), ("many_agents", 200, 20), ("q1", 200, 21),
                ("start_on_beam", 200, 22)]


@pytest.mark.parametrize("name,steps,seed", ROLLOUT_MAPS, ids=[m[0] for m in ROLLOUT_MAPS])
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_rollout_matches_restatement(oracle_mod, name, steps, seed, multi):
    play(oracle_mod, [name], 24, steps, seed, multi_objective=multi, params=PARAMS[(len(name) + multi) % 3])


@pytest.mark.parametrize("path", ["default", "fused", "two_launches", "persistent"])
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("name", ["level1", "level2"])
def test_levels_without_beams(oracle_mod, name, multi, path):
    """No source, nothing to reward: the shaped term is 0 (potential of an empty array) on EVERY step path -- the wrapped strategy's
    gem / exit / done rewards must still come through, step after step, also from the persistent tensors --, the extras are [n, A, 0]."""
    seen = []
    play(oracle_mod, [name], 16, 120, 2, multi_objective=multi, step_kw=STEP_PATHS[path], need_events=False, rewards_seen=seen)
    assert any(r.any() for r in seen[1:]), "no non-zero reward after the first step: the rollout proves nothing about stale rewards"


@pytest.mark.parametrize("path", ["default", "persistent"])
def test_empty_lasers_to_reward(oracle_mod, path):
    """lasers_to_reward=[] on a map WITH sources: the same empty potential, next to real extras."""
    play(oracle_mod, ["level6"], 16, 200, 23, multi_objective=True, lasers=[], step_kw=STEP_PATHS[path])


def test_start_cells_on_beams(oracle_mod):
    """Both agents of `start_on_beam` start on a tile of their own beam: after every reset -- reset(), reset(env_mask), the step kernel's
    auto-reset -- those sources count as reached, and an auto-reset's previous potential is the one at the start cells."""
    import torch

    from lle_amd import BatchedLLE, LaserSubgoal, PotentialShapedLLE, SingleObjective
    env = BatchedLLE(SHAPING_MAPS["start_on_beam"], 8, reward_strategy=PotentialShapedLLE(SingleObjective(), gamma=1.0, reward_value=1.0),
                     extras_generator=LaserSubgoal())
    env.reset()
    assert env.extras()[0].tolist() == [[1.0, 0.0], [0.0, 1.0]]
    # nobody moves: two of the four entries are reached from the start, so the potential stays 2 and the shaped term is 1.0 * 2 - 2 = 0
    assert env.step(torch.full((8, 2), 4, dtype=torch.uint8))["reward"].flatten().tolist() == [0.0] * 8
    for multi in (False, True):
        play(oracle_mod, ["start_on_beam"], 32, 200, 22, multi_objective=multi, params=(0.9, 0.3), reset_by="mask")
        play(oracle_mod, ["start_on_beam"], 32, 200, 22, multi_objective=multi, step_kw=dict(persistent=True))


@pytest.mark.parametrize("params", PARAMS, ids=[f"g{g}-v{v}" for g, v in PARAMS])
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_gamma_and_reward_value(oracle_mod, params, multi):
    play(oracle_mod, ["level6"], 32, 300, 3, multi_objective=multi, params=params)


def test_source_subset_with_a_duplicate(oracle_mod):
    """lasers_to_reward = [2, 0, 2]: source 2 counts twice in the potential, source 1 not at all; extras over [1, 2] only."""
    for multi in (False, True):
        play(oracle_mod, ["level6"], 32, 300, 4, multi_objective=multi, params=(0.9, 0.3), lasers=[2, 0, 2], extras=[1, 2])
    play(oracle_mod, ["level6"], 16, 300, 4, lasers=None, extras=[0])      # extras without shaping
    play(oracle_mod, ["level6"], 16, 300, 4, lasers=[1], extras=None)      # shaping without extras


STEP_PATHS = {"default": {}, "fused": dict(fused=True), "two_launches": dict(fused=False), "persistent": dict(persistent=True)}


@pytest.mark.parametrize("path", sorted(STEP_PATHS))
@pytest.mark.parametrize("randomize", [False, True], ids=["own_colours", "randomize_lasers"])
@pytest.mark.parametrize("name", ["level6", "three_beam_cell"])
def test_every_step_path(oracle_mod, path, randomize, name):
    """default / fused=True / fused=False / persistent=True, with and without randomize_lasers: level 6 re-colours the envs it resets
    inside the step kernel; the three-beam map (a cell of more than two layers) resets on the host ahead of the step."""
    play(oracle_mod, [name], 32, 300, 5, multi_objective=(path in ("fused", "persistent")), randomize=randomize, step_kw=STEP_PATHS[path])


def test_multi_map_batch(oracle_mod):
    """Map m owns block m: the cell table and the start cells are the block's own.  3 environments per map (a workgroup spans
    several maps: the table stays in global memory) and 128 (one map per workgroup: the table in LDS)."""
    from lle_amd import mapgen
    texts = [mapgen.generate(seed=100 + s, height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2) for s in range(4)]
    play(oracle_mod, texts, 3, 300, 6, multi_objective=True)
    play(oracle_mod, texts, 128, 60, 6, params=(1.0, 1.0))


def test_reset_with_env_mask(oracle_mod):
    play(oracle_mod, ["level6"], 32, 300, 7, reset_by="mask", multi_objective=True)
    play(oracle_mod, ["nested"], 32, 300, 7, reset_by="mask", step_kw=dict(persistent=True))


def test_set_state_mid_episode(oracle_mod):
    for multi in (False, True):
        play(oracle_mod, ["level6"], 32, 300, 8, multi_objective=multi, set_state_at=40)


def test_level6_at_65536_environments(oracle_mod):
    n = 65536
    play(oracle_mod, ["level6"], n, 6, 9, lockstep=64, need_events=False)
    play(oracle_mod, ["level6"], n, 4, 9, lockstep=64, multi_objective=True, step_kw=dict(persistent=True), need_events=False)


def test_update_map_validates(oracle_mod):
    """Exits and colours do not enter the tables: lle_shaping_update_map accepts the map after set_exits and refuses another map."""
    from lle_amd import BatchedLLE, Map
    env = BatchedLLE(LEVELS[6], 8, extras_generator="laser_subgoal")
    st = env.world._stream()
    env._shaping.update_map(0, env.world.map, st)
    with pytest.raises(RuntimeError, match="not a recompilation"):
        env._shaping.update_map(0, Map(EXTRA_MAPS["nested"]), st)
    with pytest.raises(RuntimeError, match="map_index"):
        env._shaping.update_map(1, env.world.map, st)


def test_without_the_arguments_nothing_changes():
    """A BatchedLLE built without reward_strategy / extras_generator returns the dict keys it always did and never loads the
    library (a fresh interpreter: this process has loaded it)."""
    import subprocess
    import sys
    code = ("import sys, torch\n"
            "from lle_amd import BatchedLLE\n"
            "env = BatchedLLE(%r, 64)\n"
            "env.reset()\n"
            "acts = torch.full((64, env.n_agents), 4, dtype=torch.uint8, device='cuda')\n"
            "keys = set()\n"
            "for kw in ({}, dict(fused=True), dict(fused=False), dict(persistent=True)):\n"
            "    keys |= set(env.step(acts, auto_reset=True, **kw))\n"
            "assert keys == {'obs', 'state', 'reward', 'done', 'available_actions', 'err'}, keys\n"
            "assert env.extras().shape == (64, env.n_agents, 0) and env.extras_shape == (0,) and env.objectives == ['reward']\n"
            "assert 'lle_amd.shaping' not in sys.modules\n"
            "assert 'liblle_shaping' not in open('/proc/self/maps').read()\n"
            "print('untouched')\n" % LEVELS[6])
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=300)
    assert res.returncode == 0 and "untouched" in res.stdout, res.stdout + res.stderr


def test_contradictions_and_reward_accessor():
    import torch

    from lle_amd import BatchedLLE, MultiObjective, PotentialShapedLLE, SingleObjective
    with pytest.raises(ValueError):  # python/tests/test_reward_strategy.py:96-104: `.pbrs().multi_objective()`
        BatchedLLE(LEVELS[3], 4, multi_objective=True, reward_strategy=PotentialShapedLLE(SingleObjective()))
    with pytest.raises(ValueError):
        BatchedLLE(LEVELS[3], 4, multi_objective=True, reward_strategy=SingleObjective())
    with pytest.raises(ValueError, match="Invalid extra type"):
        BatchedLLE(LEVELS[3], 4, extras_generator=3)
    with pytest.raises(ValueError, match="not a laser source"):
        BatchedLLE(LEVELS[6], 4, reward_strategy=PotentialShapedLLE(SingleObjective(), lasers_to_reward=[(0, 0)]))
    assert BatchedLLE(LEVELS[3], 4, reward_strategy=MultiObjective()).multi_objective
    assert BatchedLLE(LEVELS[3], 4, multi_objective=True, reward_strategy=PotentialShapedLLE(MultiObjective())).objectives[-1] == "PBRS"
    import lle_amd
    env = lle_amd.level(6).build(8, reward_strategy=PotentialShapedLLE(SingleObjective(), gamma=1.0, reward_value=1.0), extras_generator="laser_subgoal")
    assert env.extras_shape == (3,) and env.name == "LLE-lvl6"
    # the "extras" key follows the generator, not the library: a generator without columns gives [n, A, 0] on every path, with or without shaping
    from lle_amd import LaserSubgoal, NoExtras
    for text, gen, strategy in ((LEVELS[6], NoExtras(), None), (LEVELS[1], LaserSubgoal(), None), (LEVELS[1], "laser_subgoal", PotentialShapedLLE(MultiObjective())),
                                (LEVELS[6], NoExtras(), PotentialShapedLLE(SingleObjective()))):
        e = BatchedLLE(text, 8, extras_generator=gen, reward_strategy=strategy)
        stay = torch.full((8, e.n_agents), 4, dtype=torch.uint8)
        for kw in ({}, dict(fused=True), dict(fused=False), dict(persistent=True)):
            got = e.step(stay, **kw)
            assert tuple(got["extras"].shape) == (8, e.n_agents, 0) and got["extras"].dtype == torch.float32, (gen, kw)
    assert "extras" not in BatchedLLE(LEVELS[6], 8, reward_strategy=PotentialShapedLLE(SingleObjective())).step(torch.full((8, 4), 4, dtype=torch.uint8))
    out = env.step(torch.full((8, 4), 4, dtype=torch.uint8))
    assert torch.equal(env.reward(), out["reward"]) and set(out) == {"obs", "state", "reward", "done", "available_actions", "err", "extras"}


def test_every_compiled_kernel_is_launched(oracle_mod):
    """The library holds ten instantiations (lanes per environment 1 / 2 / 4 / 8 / 16 x cell table in LDS or in global memory).  Each is
    driven here against the restatement -- one map per batch (LDS) and two maps at 3 environments each (global memory) for every
    group size -- and must then be named by lle_shaping_debug_launched."""
    from lle_amd import mapgen, shaping
    shapes = {1: dict(height=6, width=7, n_agents=1, n_lasers=2, n_gems=2, n_voids=1), 2: dict(height=7, width=7, n_agents=2, n_lasers=3, n_gems=1, n_voids=1),
              4: dict(height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2), 8: dict(height=12, width=12, n_agents=7, n_lasers=5, n_gems=2, n_voids=2),
              16: dict(height=16, width=16, n_agents=12, n_lasers=10, n_gems=6, n_voids=3)}
    for g, shape in shapes.items():
        texts = [mapgen.generate(seed=200 + s, **shape) for s in range(2)]
        play(oracle_mod, texts[:1], 40, 40, 10 + g, multi_objective=bool(g & 5), need_events=False)
        play(oracle_mod, texts, 3, 40, 10 + g, multi_objective=not (g & 5), need_events=False)
    missing = sorted(set(shaping.compiled_kernels()) - set(shaping.launched_kernels()))
    assert not missing, f"compiled but never launched: {missing}"
    assert len(shaping.compiled_kernels()) == 10
