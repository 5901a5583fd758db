"""BatchedLLE(cooperation="temporal") -- the coop kernel and behind it the cooptrails kernel, lle_amd/cooptrails/cooptrails.hip --
in differential rollouts: the coop arrays against tests/coop_ref.py, the trail arrays against the restatement from the definition of
a trail (tests/cooptrails_ref.py), EVERY buffer of the tracker compared exactly (torch.equal) after every step.

The actions come from the oracle side (uniform over each agent's available actions, numpy generator), so a rollout is the same on every
box; `play(..., gpu=False)` runs the oracle side alone.  Random play rarely cooperates in depth: every rollout asserts its coverage
from the restatement alone, and the maps, shapes and seeds below were chosen with play(gpu=False) so that it is there (the counts are
written next to them)."""
import json
import os

import numpy as np
import pytest

from tests import coop_ref, cooptrails_ref
from tests.oracle_env import OracleLLE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGHT = {c["name"]: c for c in coop_ref.load_cases()["worlds"]}["eight-agent-interdependent-8"]["map"]
TRAIL_MAPS = {c["name"]: c["map"] for c in json.load(open(os.path.join(ROOT, "tests", "golden", "kat_trails.json")))["catalogue"] if "map" in c}
CYCLE3 = TRAIL_MAPS["three-agent-temporal-cycle"]
PAPER2 = TRAIL_MAPS["paper-sequence-2"]
PAPER2_OPEN = PAPER2.replace(" @  @  @ X  x", " @  @  . X  x", 1)  # a wall that nobody needs opened: another map of the same shape
FOUR = TRAIL_MAPS["four-agent-interdependent-4-sequence-6"]
STEP_PATHS = {"default": {}, "fused": dict(fused=True), "two_launches": dict(fused=False), "persistent": dict(persistent=True)}
COOP_NAMES = ("step_edges", "episode_edges", "last_edges", "episode_profile", "last_profile")
TRAIL_NAMES = ("episode_trails", "last_trails", "episode_tprofile", "last_tprofile")


def compare(tracker, refs, trefs, where):
    import torch
    cols = list(zip(*[r.arrays() for r in refs]))
    want = [torch.tensor(cols[k], dtype=torch.int32) for k in range(3)] + [torch.tensor(cols[k], dtype=torch.uint8) for k in (3, 4)]
    tcols = list(zip(*[r.arrays() for r in trefs]))
    want += [torch.tensor(tcols[k], dtype=torch.int64) for k in range(2)] + [torch.tensor(tcols[k], dtype=torch.uint8) for k in (2, 3)]
    for name, want_k in zip(COOP_NAMES + TRAIL_NAMES, want):
        got = getattr(tracker, name).cpu()
        if not torch.equal(got, want_k):
            bad = int((got != want_k).reshape(len(refs), -1).any(dim=1).nonzero()[0])
            raise AssertionError(f"{where}: {name} differs in env {bad}: {got[bad].tolist()} != {want_k[bad].tolist()}")


def play(oracle_mod, texts, per_map, steps, seed, randomize=False, step_kw=None, reset_by="auto", gpu=True, set_state_at=None, unavailable=0.0):
    """One rollout of len(texts) * per_map environments (map m owns block m) against one oracle world, one coop_ref.EnvRef and one
    cooptrails_ref.EnvRef per environment.  reset_by: "auto" = step(auto_reset=True); "mask" = reset(env_mask=done) ahead of a plain
    step; "none" = plain steps.  set_state_at: step after which every environment is handed its own current state through set_state
    (the episode continues: one more state).  unavailable: share of the environments that are handed an action their first agent cannot
    take -- the step is refused there, which adds no state to the trails.  Returns the coverage counted from the restatement."""
    n = per_map * len(texts)
    step_kw = dict(step_kw or {})
    worlds = [oracle_mod.OracleWorld(texts[e // per_map]) for e in range(n)]
    A, L, G = worlds[0].n_agents, worlds[0].n_sources, worlds[0].n_gems
    lles = [OracleLLE(w) for w in worlds]
    for r in lles:
        r.free_running = True
    refs = [coop_ref.EnvRef(A) for _ in range(n)]
    trefs = [cooptrails_ref.EnvRef(A) for _ in range(n)]
    rng = np.random.default_rng(seed)
    cover = {"edges": 0, "arcs2": 0, "long2": [0] * len(texts), "long3": 0, "saturated": 0, "refused": 0, "refused_and_reset": 0, "finished_sequential": 0}
    env = None
    if gpu:
        import torch

        from lle_amd import BatchedLLE
        from lle_amd.cooptrails import TemporalCooperationTracker
        env = BatchedLLE(texts if len(texts) > 1 else texts[0], n, randomize_lasers=randomize, seed=seed, cooperation="temporal")
        first_words = env.world.map.source_first_words()
        assert isinstance(env.cooperation, TemporalCooperationTracker) and env.cooperation.n_envs == n

    def colours_now():
        return env.world.src_colour.cpu().numpy()[:, first_words]

    def both(e, ops, state=(), starts=(), was_reset=False, refused=False):
        refs[e].update(ops, state, start_edges=starts, was_reset=was_reset)
        trefs[e].update(ops, state, start_edges=starts, was_reset=was_reset, refused=refused)

    def count(e):
        longest = max(trefs[e].lengths())
        cover["edges"] += len(refs[e].step) >= 1
        cover["arcs2"] += len(refs[e].step) >= 2
        cover["long2"][e // per_map] += longest >= 2
        cover["long3"] += longest >= 3
        cover["saturated"] += longest == 15

    cols = None
    if gpu:
        env.reset()
        cols = colours_now() if randomize else None
    for e, r in enumerate(lles):
        r.reset(cols[e] if cols is not None else None)
        # BatchedLLE marks the state of its construction (CLEAR | MARK_POS), then reset() finishes that episode and marks again
        both(e, coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(oracle_mod.OracleWorld(texts[e // per_map])))
        both(e, coop_ref.FINISH | coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(r.w))
    if gpu:
        compare(env.cooperation, refs, trefs, "after reset")
    for t in range(steps):
        over = np.array([r.done for r in lles])
        resetting = [int(e) for e in np.nonzero(over)[0]] if reset_by != "none" else []
        in_kernel_colours = randomize and reset_by == "auto"  # drawn by the step kernel: known only after the step
        if gpu and reset_by == "mask" and resetting:
            env.reset(env_mask=torch.from_numpy(over.astype(np.uint8)).cuda())
            cols = colours_now() if randomize else None
        starts = {}
        for e in resetting:
            cover["finished_sequential"] += max(trefs[e].lengths()) >= 2
            lles[e].reset(cols[e] if (cols is not None and reset_by == "mask") else None)
            if reset_by == "mask":
                both(e, coop_ref.FINISH | coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(worlds[e]))
            elif not in_kernel_colours:
                starts[e] = coop_ref.detect(worlds[e])
        actions = np.zeros((n, A), np.uint8)
        bad = rng.random(n) < unavailable
        for e, w in enumerate(worlds):
            for a, mask in enumerate(w.available_mask()):
                opts = [k for k in range(5) if (mask >> k) & 1]
                actions[e, a] = opts[int(rng.integers(len(opts)))]
            closed = [k for k in range(5) if not (w.available_mask()[0] >> k) & 1]
            bad[e] = bad[e] and bool(closed)
            if bad[e]:
                actions[e, 0] = closed[int(rng.integers(len(closed)))]
        if gpu:
            out = env.step(torch.from_numpy(actions).cuda(), auto_reset=(reset_by == "auto"), **step_kw)
            assert ((out["err"] != 0).cpu().numpy() == bad).all(), f"t={t}: the refused steps are not the ones handed an unavailable action"
            if in_kernel_colours:
                cols = colours_now()
        if in_kernel_colours:
            for e in resetting:  # LLE.reset: world.reset() under the colours the env had, then the new ones on the live world
                for l in range(L):
                    if cols is not None:
                        worlds[e].set_source(l, colour=int(cols[e][l]))
                starts[e] = coop_ref.detect(worlds[e])
        for e, r in enumerate(lles):
            if bad[e]:
                with pytest.raises(oracle_mod.OracleError):
                    r.step(actions[e])
                cover["refused"] += 1
                cover["refused_and_reset"] += reset_by == "auto" and e in starts
            else:
                r.step(actions[e])
            both(e, coop_ref.MARK_POS, coop_ref.detect(r.w), starts.get(e, ()), was_reset=reset_by == "auto" and e in starts, refused=bool(bad[e]))
            count(e)
        if gpu:
            compare(env.cooperation, refs, trefs, f"t={t}")
        if set_state_at is not None and t == set_state_at:
            pos = [w.positions() for w in worlds]
            gems = [w.gems_collected() for w in worlds]
            alive = [w.alive() for w in worlds]
            if gpu:
                err = env.set_state(torch.tensor(pos, dtype=torch.uint8), torch.tensor(gems, dtype=torch.bool).reshape(n, G), torch.tensor(alive, dtype=torch.bool))
                ok = (err == 0).cpu().numpy()
            else:
                ok = np.ones(n, bool)
            for e, r in enumerate(lles):
                try:
                    r.set_state(pos[e], gems[e], alive[e])
                    assert ok[e]
                except oracle_mod.OracleError:
                    assert not ok[e]
                both(e, coop_ref.MARK_POS, coop_ref.detect(r.w))  # (after set_state no SKIP_REFUSED: the state handed in is one more state)
            if gpu:
                compare(env.cooperation, refs, trefs, f"after set_state at t={t}")
    if gpu:  # the queries, against the restatement and the flattened edges
        tr = env.cooperation
        lengths = [r.lengths() for r in trefs]
        assert tr.trail_lengths().cpu().tolist() == lengths and tr.longest_trail().cpu().tolist() == [max(v) for v in lengths]
        for k in (2, 3, 8, 15):
            assert tr.is_sequential(k).cpu().tolist() == [max(v) >= k for v in lengths]
            assert tr.is_sequential(k, last=True).cpu().tolist() == [r.last_valid and max(r.last_lengths) >= k for r in trefs]
        assert tr.is_mutual().cpu().tolist() == [cooptrails_ref.is_mutual(r.episode) for r in refs]
        assert tr.is_mutual(last=True).cpu().tolist() == [cooptrails_ref.is_mutual(r.last) for r in refs]
        assert bool(tr.trails_exact().all()) and bool(tr.trails_exact(last=True).all())
    return cover


# ---- the rollouts; the counts in the docstrings are those of play(gpu=False) with the very arguments of the test
def test_ring_of_eight(oracle_mod):
    """Every reset state holds the eight ring edges: a trail of 8 from the first state on; the episodes that last reach the saturation.
    64 x 150, seed 61: 5 243 environment-steps whose state holds >= 2 arcs, every one with a longest trail >= 8, 17 saturated."""
    cover = play(oracle_mod, [EIGHT], 64, 150, 61)
    assert cover["arcs2"] >= 500 and cover["saturated"] >= 10 and cover["long2"][0] == 64 * 150, cover


@pytest.mark.parametrize("path", sorted(STEP_PATHS))
def test_every_step_path(oracle_mod, path):
    """16 x 30, seed 62: 260 environment-steps with >= 2 arcs, all 480 with a longest trail >= 3."""
    cover = play(oracle_mod, [EIGHT], 16, 30, 62, step_kw=STEP_PATHS[path])
    assert cover["arcs2"] >= 100 and cover["long3"] >= 100, cover


@pytest.mark.parametrize("reset_by", ["auto", "mask", "none"])
def test_three_agents(oracle_mod, reset_by):
    """paper-sequence-2 (three agents, two sources), 64 x 60, seed 64: 130 environment-steps with a longest trail >= 2 (auto and mask; 98 without resets)."""
    cover = play(oracle_mod, [PAPER2], 64, 60, 64, reset_by=reset_by)
    assert cover["long2"][0] >= 50, cover


def test_states_of_several_arcs(oracle_mod):
    """three-agent-temporal-cycle, 64 x 60, seed 63: 280 environment-steps whose state holds >= 2 arcs."""
    cover = play(oracle_mod, [CYCLE3], 64, 60, 63)
    assert cover["arcs2"] >= 100, cover


def test_four_agents(oracle_mod):
    """four-agent-interdependent-4-sequence-6, 64 x 60, seed 65: 35 environment-steps with a longest trail >= 2."""
    cover = play(oracle_mod, [FOUR], 64, 60, 65)
    assert cover["long2"][0] >= 20, cover


def test_set_state_mid_episode(oracle_mod):
    """16 x 20, seed 66: 194 environment-steps with >= 2 arcs, all 320 with a longest trail >= 3."""
    cover = play(oracle_mod, [EIGHT], 16, 20, 66, set_state_at=8)
    assert cover["long3"] >= 100, cover


def test_randomize_lasers(oracle_mod):
    """Level 6, 512 x 40: the colours are drawn on the device, so the coverage is not known beforehand; some environment-steps have an
    edge (tests/test_gpu_coop.py sees 20 and more in 1 024 x 40)."""
    from oracle.levels import LEVELS
    cover = play(oracle_mod, [LEVELS[6]], 512, 40, 67, randomize=True)
    assert cover["edges"] >= 5, cover


def test_two_maps(oracle_mod):
    """paper-sequence-2 and the same with one wall opened, 2 x 33, 60 steps, seed 68: 43 and 46 environment-steps with a longest trail >= 2."""
    cover = play(oracle_mod, [PAPER2, PAPER2_OPEN], 33, 60, 68)
    assert min(cover["long2"]) >= 20, cover


def test_unavailable_actions_add_no_layer(oracle_mod):
    """A fifth of the environments is handed an action its first agent cannot take: the step is refused, the coop tracker marks the
    unchanged state again and the trails do not move -- also in an environment the step kernel reset first.  32 x 40, seed 69:
    272 refused steps, 169 of them in an environment that was reset first."""
    cover = play(oracle_mod, [EIGHT], 32, 40, 69, unavailable=0.2)
    assert cover["refused"] >= 100 and cover["refused_and_reset"] >= 10 and cover["long3"] >= 100, cover


def test_cooperation_true_is_the_plain_tracker():
    import lle_amd
    from lle_amd.cooptrails import TemporalCooperationTracker
    plain = lle_amd.level(6).build(8, cooperation=True)
    assert type(plain.cooperation) is lle_amd.CooperationTracker and not hasattr(plain.cooperation, "episode_trails")
    temporal = lle_amd.level(6).build(8, cooperation="temporal")
    assert type(temporal.cooperation) is TemporalCooperationTracker
    assert lle_amd.level(6).build(8).cooperation is None
    with pytest.raises(ValueError, match="temporal"):
        lle_amd.level(6).build(8, cooperation="flattened")


def test_without_the_argument_the_library_is_not_loaded():
    """cooperation=True in a fresh interpreter never loads liblle_cooptrails.so."""
    import subprocess
    import sys
    code = ("import sys, torch, lle_amd\n"
            "env = lle_amd.level(6).build(64, cooperation=True)\n"
            "env.reset()\n"
            "env.step(torch.full((64, env.n_agents), 4, dtype=torch.uint8, device='cuda'), auto_reset=True)\n"
            "assert 'lle_amd.cooptrails' not in sys.modules\n"
            "assert 'liblle_cooptrails' not in open('/proc/self/maps').read() and 'liblle_coop' in open('/proc/self/maps').read()\n"
            "print('untouched')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0 and "untouched" in res.stdout, res.stdout + res.stderr


def test_every_compiled_kernel_is_launched(oracle_mod):
    """Last in the module: 8 agents (G = 8), 3 (G = 4) and 4 (G = 4) ran above; one short rollout each for G = 1, 2 and 16 against the
    restatement; then each cooptrails_kernel<G> must be named by lle_cooptrails_debug_launched."""
    from lle_amd import cooptrails
    from tests.test_gpu_coop import line_map
    play(oracle_mod, ["L0E S0 . . X\n. . . . ."], 16, 10, 70)
    for n_agents in (2, 16):
        play(oracle_mod, [line_map(n_agents)], 16, 10, 71)
    missing = sorted(set(cooptrails.compiled_kernels()) - set(cooptrails.launched_kernels()))
    assert not missing, f"compiled but never launched: {missing}"
    assert len(cooptrails.compiled_kernels()) == 5
