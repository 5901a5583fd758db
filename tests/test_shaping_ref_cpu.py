"""tests/shaping_ref.py (the array-level restatement of lle_shaping_update that tests/test_gpu_shaping_states.py compares the kernel
with) against the per-environment restatement of the reference, OracleShapedLLE (tests/oracle_shaping.py), without a GPU.

The array-level reference is driven with the sequence of lle_shaping_update calls BatchedLLE makes (lle_amd/env.py: reset, extras(),
the step's launch with and without LLE_SHAPING_HONOUR_AUTO_RESET, reset(env_mask), set_state) on the positions and reset bits of
oracle rollouts, and must return OracleShapedLLE's rewards and extras exactly.  The exact-arithmetic helpers are checked on the cases
the kernel tests rely on."""
from fractions import Fraction

import numpy as np
import pytest

from oracle.levels import LEVELS
from tests import instantiation_maps, shaping_ref
from tests.oracle_env import OracleLLE
from tests.oracle_shaping import SHAPING_MAPS, OracleShapedLLE
from tests.parity_util import LONG_MAPS
from tests.shaping_ref import CLEAR, HONOUR_AUTO_RESET, MARK_POS, MARK_STARTS, ShapingRef

MAPS = {"level6": LEVELS[6], "three_beam_cell": SHAPING_MAPS["three_beam_cell"], "start_on_beam": SHAPING_MAPS["start_on_beam"],
        "long_crossing": LONG_MAPS["long_crossing"], "agents16": instantiation_maps.build(16, 12, crossing=True, seed=3)}
BOTH = CLEAR | MARK_STARTS


def drive(oracle_mod, text, k, steps, seed, multi, params, lasers="all", extras="all", reset_by="auto", set_state_at=None):
    """k oracle environments of one map, played like tests/test_gpu_shaping.play, with ShapingRef in the place of the batch.
    Returns (resets, deaths, non-zero shaped terms) seen."""
    gamma, value = params
    worlds = [oracle_mod.OracleWorld(text) for _ in range(k)]
    L, A, G = worlds[0].n_sources, worlds[0].n_agents, worlds[0].n_gems
    every = list(range(L))
    pbrs_ids = None if lasers is None else every if lasers == "all" else list(lasers)
    extras_ids = None if extras is None else every if extras == "all" else list(extras)
    refs = [OracleShapedLLE(w, pbrs=None if pbrs_ids is None else dict(gamma=gamma, reward_value=value, lasers=pbrs_ids),
                            extras=[] if extras_ids is None else [extras_ids], multi_objective=multi) for w in worlds]
    twins = [OracleLLE(oracle_mod.OracleWorld(text), multi_objective=multi) for _ in range(k)]  # the wrapped strategy's reward
    for r in refs + twins:
        r.free_running = True
    start_avail = [r.w.available_actions() for r in refs]
    start_pos = [r.w.start_pos for r in refs]
    rng = np.random.default_rng(seed)
    ref = ShapingRef([oracle_mod.OracleWorld(text)], k, pbrs_ids or [], extras_ids or [], gamma, value)
    shaped, kind = pbrs_ids is not None, int(multi)

    def positions():
        return np.array([r.w.positions() for r in refs], np.uint8).reshape(k, A, 2)

    def low_bits():
        return rng.integers(0, 128, k).astype(np.uint8)

    def check_extras(state, where):
        # BatchedLLE.extras(): MARK_POS on the extras array alone, extras_out
        state, (_, got) = ref.update(state, positions(), low_bits(), 0, MARK_POS, 0, kind, None, None)
        want = np.stack([r.compute_extras() for r in refs])
        assert got.dtype == np.float32 and np.array_equal(got, want), f"{where}: extras differ"
        return state

    # BatchedLLE.__init__ / reset(): _shaping_reset(None), then the world's reset
    state, _ = ref.update(ref.empty_state(), positions(), low_bits(), BOTH, BOTH, 0, kind, None, None)
    for r in refs + twins:
        r.reset()
    state = check_extras(state, "after reset")
    resets = deaths = shaped_steps = 0
    history = []
    for t in range(steps):
        over = np.array([r.done for r in refs])
        assert over.tolist() == [b.done for b in twins]
        resets += int(over.sum())
        actions = np.zeros((k, A), np.uint8)
        for e, r in enumerate(refs):
            lists = start_avail[e] if over[e] else r.w.available_actions()
            for a in range(A):
                actions[e, a] = lists[a][int(rng.integers(len(lists[a])))]
        if reset_by == "mask" and over.any():   # BatchedLLE.reset(env_mask=done) ahead of a plain step
            state, _ = ref.update(state, positions(), low_bits(), BOTH, BOTH, 0, kind, over.astype(np.uint8), None)
        rewards, bases = [], []
        for e, (r, b) in enumerate(zip(refs, twins)):
            if over[e]:
                r.reset()
                r.compute_extras()
                b.reset()
            before = r.n_deads
            rewards.append(r.step(actions[e])[0])
            bases.append(b.step(actions[e])[0])
            deaths += r.n_deads - before
        # the step's launch: MARK_POS on both arrays, the flag after an auto-resetting step (bit 7 of evcount = the kernel reset the env)
        flags = HONOUR_AUTO_RESET if reset_by == "auto" else 0
        evcount = low_bits() | (over.astype(np.uint8) << 7 if reset_by == "auto" else rng.integers(0, 2, k).astype(np.uint8) << 7)
        base = np.stack(bases).astype(np.float32)
        state, (got_r, got_e) = ref.update(state, positions(), evcount, MARK_POS, MARK_POS, flags, kind, None, base if shaped else None)
        want_r = np.stack(rewards).astype(np.float32)
        if shaped:
            assert got_r.dtype == np.float32 and got_r.shape == want_r.shape
            assert np.array_equal(got_r.view(np.uint32), want_r.view(np.uint32)), f"t={t}: reward {got_r.tolist()} != {want_r.tolist()}"
            shaped_steps += int((want_r[:, -1] != base[:, -1]).sum()) if not multi else int((want_r[:, 4] != 0).sum())
        else:
            assert got_r is None and np.array_equal(want_r, base)
        want_e = np.stack([r.compute_extras() for r in refs])
        assert np.array_equal(got_e, want_e), f"t={t}: extras differ"
        history.append([(r.w.positions(), r.w.gems_collected(), all(r.w.alive()) and not r.done) for r in refs])
        if set_state_at is not None and t == set_state_at:
            states = []
            for e, r in enumerate(refs):
                pos, gems, fine = history[max(0, t - 10)][e]
                if fine:
                    probe = oracle_mod.OracleWorld(text)
                    try:
                        probe.set_state(pos, gems, [True] * A)
                    except oracle_mod.OracleError:
                        fine = False
                states.append((pos, gems) if fine else (start_pos[e], [False] * G))
            if shaped:  # BatchedLLE.set_state: CLEAR | MARK_POS where the agents stand before the call, MARK_POS after it
                state, _ = ref.update(state, positions(), low_bits(), CLEAR | MARK_POS, 0, 0, kind, None, None)
            for e, (r, b) in enumerate(zip(refs, twins)):
                r.set_state(states[e][0], states[e][1], [True] * A)
                b.set_state(states[e][0], states[e][1], [True] * A)
            if shaped:
                state, _ = ref.update(state, positions(), low_bits(), MARK_POS, 0, 0, kind, None, None)
            state = check_extras(state, f"after set_state at t={t}")
    # the device layout round-trips: nothing of the state is lost in the u32 words
    back = ref.from_words(*ref.to_words(state))
    for a, b in ((back.strategy, state.strategy), (back.extras, state.extras)):
        assert np.array_equal(a.listed, b.listed) and np.array_equal(a.rest, b.rest)
    return resets, deaths, shaped_steps


# seeds as in tests/test_gpu_shaping.py where the map is played there; each rollout must see resets and shaped terms
@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("name,steps,seed", [("level6", 150, 14), ("three_beam_cell", 100, 18), ("start_on_beam", 100, 22), ("long_crossing", 100, 19),
                                             ("agents16", 60, 24)])
def test_reference_reproduces_oracle_rollouts(oracle_mod, name, steps, seed, multi):
    params = [(0.99, 0.5), (1.0, 1.0), (0.9, 0.3)][(len(name) + multi) % 3]
    for reset_by in ("auto", "mask"):
        resets, deaths, shaped = drive(oracle_mod, MAPS[name], 8, steps, seed, multi, params, reset_by=reset_by)
        assert resets > 0 and shaped > 0, f"{name} {reset_by}: {resets} resets, {deaths} deaths, {shaped} shaped terms: the rollout proves nothing"


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
def test_reference_with_a_duplicated_source(oracle_mod, multi):
    """lasers_to_reward = [2, 0, 2]: two columns for source 2, none for source 1; extras over [1, 2]."""
    resets, _, shaped = drive(oracle_mod, MAPS["level6"], 8, 150, 4, multi, (0.9, 0.3), lasers=[2, 0, 2], extras=[1, 2])
    assert resets > 0 and shaped > 0
    drive(oracle_mod, MAPS["level6"], 6, 100, 4, multi, (0.9, 0.3), lasers=None, extras=[0])
    drive(oracle_mod, MAPS["level6"], 6, 100, 4, multi, (0.9, 0.3), lasers=[1], extras=None)
    drive(oracle_mod, MAPS["level6"], 6, 100, 4, multi, (0.9, 0.3), lasers=[], extras="all")


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi"])
@pytest.mark.parametrize("name", ["level6", "start_on_beam"])
def test_reference_through_set_state(oracle_mod, name, multi):
    resets, _, shaped = drive(oracle_mod, MAPS[name], 8, 80, 8, multi, (0.7, 0.7), lasers=[2, 0, 2] if name == "level6" else "all", set_state_at=40)
    assert resets > 0 and shaped > 0


def test_unselected_and_outside_positions(oracle_mod):
    """env_mask leaves an environment's state alone; (255, 255) marks nothing; unlisted sources are carried in the words but never count."""
    ref = ShapingRef([oracle_mod.OracleWorld(MAPS["level6"])], 4, [2], [0], 0.9, 0.3)
    A = ref.A
    words = np.full((4, A), 0b010, np.uint32)   # source 1: listed by neither array
    state = ref.from_words(words, words)
    assert not state.strategy.listed.any() and state.strategy.rest.any()
    assert all(np.array_equal(w, words) for w in ref.to_words(state))
    cell = next((r[0], r[1]) for r in oracle_mod.OracleWorld(MAPS["level6"]).lasers() if r[2] == 2)
    pos = np.zeros((4, A, 2), np.uint8)
    pos[:] = cell
    pos[1] = 255
    mask = np.array([1, 1, 0, 1], np.uint8)
    new, (reward, extras) = ref.update(state, pos, np.zeros(4, np.uint8), MARK_POS, MARK_POS, 0, 0, mask, np.zeros(4, np.float32))
    ws, we = ref.to_words(new)
    assert (ws[0] & 0b100).all() and np.array_equal(ws[1], words[1]) and np.array_equal(ws[2], words[2]) and np.array_equal(we[2], words[2])
    full = A * 0.3
    assert reward[0, 0] == np.float32(0.9 * full - 0.0) and reward[1, 0] == np.float32(0.9 * full - full)


# ---------------------------------------------------------------------------------------------- exact arithmetic
def test_exact_rounding_helpers():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        num, den = int(rng.integers(-10**12, 10**12)), int(rng.integers(1, 10**9))
        scale = Fraction(2) ** int(rng.integers(-160, 140))
        f = Fraction(num, den) * scale
        got = shaping_ref.round_f64(f)
        assert got is not None and float(got) == float(f) and Fraction(float(got)) == got   # Python's own correctly rounded conversion
        got32 = shaping_ref.round_f32(f)
        x = np.float64(float(got))  # values whose float64 is exact: float32(float64) is one rounding
        if Fraction(float(x)) == f:
            with np.errstate(all="ignore"):
                want32 = np.float32(x)
            assert (got32 is None and np.isinf(want32)) or Fraction(float(want32)) == got32
    assert shaping_ref.round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == 1                       # a tie goes to even
    assert shaping_ref.round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == 1 + Fraction(1, 2 ** 22)
    assert shaping_ref.round_f32(Fraction(1e-40)) == Fraction(float(np.float32(1e-40)))           # denormal
    assert shaping_ref.round_f32(Fraction(2) ** 128) is None


def test_fma_sensitive_pairs_of_the_issue():
    """The (count before, count after) pairs that tell a fused multiply-add from the documented arithmetic, as the kernel tests use them."""
    pairs = shaping_ref.fma_sensitive_pairs
    assert pairs(0.9, 0.3, 12) == [(2, 3)]
    documented, fused = shaping_ref.shaped_terms(0.9, 0.3, 12, 2, 3)
    assert float(documented) == float(np.float32(4.440892098500626e-16)) and float(fused) == float(np.float32(3.3306690738754696e-16))
    # ... which is what Python floats give
    assert float(documented) == float(np.float32(0.9 * (10 * 0.3) - 9 * 0.3))
    wide = pairs(0.9, 0.3, 128)
    assert len(wide) == 12 and (8, 20) in wide
    assert pairs(0.7, 0.7, 12) == [(2, 5)]
    assert (28, 29) in pairs(0.99, 0.5, 128)
    assert pairs(1.0, 1.0, 12) == [] and pairs(1.0, 1.0, 128) == []
    for b, a in wide:
        assert shaping_ref.fma_sensitive(0.9, 0.3, 128, b, a)
    # the narrowed search finds what the exhaustive one finds
    for gamma, value in ((0.9, 0.3), (0.7, 0.7), (0.99, 0.5), (0.95, 0.1)):
        for size in (12, 128):
            assert pairs(gamma, value, size) == pairs(gamma, value, size, brute_force=True), (gamma, value, size)
    assert not shaping_ref.fma_sensitive(0.9, 0.3, 12, 0, 0)


def test_double_rounding_sensitive_fraction():
    """`base + float(p)` against `float(base + p)`: the exact-rational answer is numpy's on every case, and both outcomes occur often."""
    rng = np.random.default_rng(6)
    hits = 0
    for _ in range(2000):
        base = np.float32(rng.choice([1.0, -1.0, 3.0]))
        p = float(rng.integers(-128, 129)) * 0.3 * 0.9 - float(rng.integers(0, 129)) * 0.3
        s = shaping_ref.double_rounding_sensitive(base, p)
        with np.errstate(all="ignore"):
            assert s == (np.float32(base) + np.float32(p) != np.float32(np.float64(base) + np.float64(p)))
        hits += s
    assert 50 < hits < 1950, hits
    assert not shaping_ref.double_rounding_sensitive(np.float32(np.inf), 0.3) and not shaping_ref.double_rounding_sensitive(np.float32(0.0), 0.3)
