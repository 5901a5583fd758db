"""The back end of a single step (step_kernel.hpp post_step): in the single-step kernels the final state and the wavefront's counters
are written where post_step runs -- in front of the observation stream on the youngest quarter of the grid, behind it elsewhere --
and the counters are summed as two packed words of 8-bit fields through DPP (kernel_common.hpp flush_stats_packed; step_logic.hpp
stat_pack_*).  Nothing the kernels write may change with that placement, and LLE_BUF_STATS must stay exact.

Sampled actions: level 6 with auto-reset at 256 / 203 / 5 environments (full wavefronts, a ragged last one, a single partial one) over
40 steps, on MODE 6 (row heads), MODE 0 (LLE_ROW_HEADS=0), MODE 7 (BatchedLLE.step fused), MODE 8 (the same with randomize_lasers) and
MODE 4 (fused without row heads: no preloaded counters, so its flush stays behind the stream), each with LLE_POST_FIRST unset, 0 and
1.  After every step every buffer and the observation equal the oracle's; at the end stats() equals the oracle's totals and the totals
recomputed from the per-step reward words, `err` and the reset bit of `evcount`.

Field width: level 1 (one lane per environment, 64 environments per wavefront) at 128 and 70 environments, every environment
replaying one plan found with the oracle, so that a whole wavefront collects, arrives, is reset and is refused in the same step; a
one-agent map with a foreign beam on which a whole wavefront dies in the same step.  Every counter then reaches 64 in one step of one
wavefront -- the largest sum an 8-bit field has to hold.

Other paths: an 8-agent map (G = 8), a fused rollout against single steps (MODE 1: 32-bit sums through the same wave sum), and the
lane-per-environment step of world_kernel."""
import collections

import numpy as np
import pytest

from oracle.levels import LEVELS
from tests.parity_util import EXTRA_MAPS, assert_state_equal, assert_step_equal, unpack_engine
from tests.test_gpu_parity import check, dims_of

pytestmark = pytest.mark.gpu

EPW = 16
SIZES = (256, 203, 5)
STEPS = 40
KEYS = ["env_steps", "agent_steps", "gems", "exits", "deaths", "invalid", "auto_resets", "reward_sum"]
EV_EXIT, EV_GEM, EV_DIED = 0, 1, 2

EIGHT_AGENTS = (
    "S0 S1 S2 S3 S4 S5 S6 S7 . .\n"
    ". . G . . . . G . .\n"
    "L1E . . . . . . . . .\n"
    ". . . . G . . . . .\n"
    "X X X X X X X X . ."
)


def counters(n, A, counts, refused, resets):
    """One step's addition to the eight counters, from [n, 4] (gems, exits, deaths, bonus), the refusals and the resets."""
    c = counts.astype(np.int64)
    return np.array([n, n * A, c[:, 0].sum(), c[:, 1].sum(), c[:, 2].sum(), int(refused.sum()), int(resets.astype(np.int64).sum()),
                     (c[:, 0] + c[:, 1] - c[:, 2] + c[:, 3]).sum()], dtype=np.int64)


class Totals:
    """The eight counters of LLE_BUF_STATS, kept twice: from the oracle's step, and from what the engine wrote per step."""

    def __init__(self, A):
        self.A = A
        self.oracle = np.zeros(8, np.int64)
        self.engine = np.zeros(8, np.int64)

    def add(self, bw, ob, ostep, oracle_resets=None):
        n = ob.n
        cnt = (ostep["ev_count"] & 0x7F).astype(np.int64)
        valid = np.arange(ostep["events"].shape[1])[None, :] < cnt[:, None]
        ty = ostep["events"][:, :, 0]
        d = ob.dump()
        want = np.stack([((ty == EV_GEM) & valid).sum(1), ((ty == EV_EXIT) & valid).sum(1), ((ty == EV_DIED) & valid).sum(1),
                         ((ostep["err"] == 0) & d["arrived"].all(1)).astype(np.int64)], axis=1)
        resets = (ostep["ev_count"] >> 7).astype(np.int64) if oracle_resets is None else oracle_resets.astype(np.int64)
        self.oracle += counters(n, self.A, want, ostep["err"] != 0, resets)
        # ---- the per-step outputs of the engine: reward words, done flags; and the totals they add up to
        got = bw.reward.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want), "reward words"
        done = ((d["alive"] == 0).any(1) | d["arrived"].all(1)).astype(np.uint8)
        assert np.array_equal(bw.done.cpu().numpy(), done), "done flags"
        err, evc = bw.err.cpu().numpy(), bw.evcount.cpu().numpy()
        self.engine += counters(n, self.A, got, err != 0, evc >> 7)
        return want, resets

    def check(self, bw, where):
        st = bw.stats()
        got = [st[k] for k in KEYS]
        assert got == self.oracle.tolist(), (where, "stats() against the oracle's totals", got, self.oracle.tolist())
        assert got == self.engine.tolist(), (where, "stats() against the per-step outputs", got, self.engine.tolist())


def set_rules(monkeypatch, heads, post_first, epw=EPW):
    monkeypatch.setenv("LLE_ROW_HEADS", heads)
    monkeypatch.setenv("LLE_STEP_EPW", str(epw))
    if post_first is None:
        monkeypatch.delenv("LLE_POST_FIRST", raising=False)
    else:
        monkeypatch.setenv("LLE_POST_FIRST", post_first)


POST = [None, "0", "1"]
POST_IDS = ["post-by-position", "post-last", "post-first"]


@pytest.mark.parametrize("post_first", POST, ids=POST_IDS)
@pytest.mark.parametrize("heads", ["1", "0"], ids=["mode6", "mode0"])
def test_world_step_sampled(oracle_mod, monkeypatch, heads, post_first):
    from lle_amd import BatchedWorld, _capi

    set_rules(monkeypatch, heads, post_first)
    for n in SIZES:
        ob = oracle_mod.OracleBatch(LEVELS[6], n)
        bw = BatchedWorld(LEVELS[6], n)
        t_ = bw.tuning()
        assert (t_["row_heads"], t_["envs_per_wave"]) == (int(heads), EPW), t_
        tot = Totals(ob.A)
        for t in range(STEPS):
            bw.obs_rows.fill_(55)
            bw.step(sample=True, auto_reset=True, seed=31, t=t, env_offset=5)
            ostep = ob.step(None, auto_reset=True, seed=31, t=t, env_offset=5)
            check(bw, ob, ostep, f"heads={heads} post_first={post_first} n={n} t={t}")
            tot.add(bw, ob, ostep)
        assert tot.oracle[6] > 0 and tot.oracle[4] > 0  # (environments did end and restart)
        tot.check(bw, f"heads={heads} post_first={post_first} n={n}")
    assert f"step_kernel<4,4,{6 if heads == '1' else 0},true,3>" in _capi.launched_kernels()


def available_draw(rng, avail):
    """One available action per agent, uniformly (avail: bool [n, A, 5]; STAY is always available)."""
    return (rng.random(avail.shape) * avail).argmax(-1).astype(np.uint8)


@pytest.mark.parametrize("post_first", POST, ids=POST_IDS)
@pytest.mark.parametrize("heads,randomize,mode", [("1", False, 7), ("1", True, 8), ("0", False, 4)], ids=["mode7", "mode8", "mode4"])
def test_batched_lle_fused_step_sampled(oracle_mod, monkeypatch, heads, randomize, mode, post_first):
    import torch

    from lle_amd import BatchedLLE, _capi
    from lle_amd._capi import RECOLOUR_SALT

    set_rules(monkeypatch, heads, post_first)
    rng = np.random.default_rng(40 + mode)
    seed = 21
    for n in SIZES:
        env = BatchedLLE(LEVELS[6], n, obs_type="layered", randomize_lasers=randomize, seed=seed)
        w, m = env.world, env.world.map
        A, L = m.n_agents, m.n_sources
        assert not randomize or env._recolour_in_step
        t_ = w.tuning()
        assert (t_["row_heads"], t_["envs_per_wave"]) == (int(heads), EPW), t_
        env.reset()
        ob = oracle_mod.OracleBatch(LEVELS[6], n)
        colours = None
        if randomize:  # (reset() draws from the torch generator: the oracle takes the colours it drew)
            colours = w.src_colour[:, :L].cpu().numpy().copy()
            for e in range(n):
                for s in range(L):
                    ob.world(e).set_source(s, colour=int(colours[e, s]))
        tot = Totals(A)
        for t in range(STEPS):
            over = w.done.cpu().numpy().astype(bool)
            actions = available_draw(rng, env.available_actions().cpu().numpy().astype(bool))
            if randomize:
                # what the kernel does with an environment that is over: world.reset() under the colours it had, then a fresh colour per
                # source from the documented hash (tests/test_gpu_env_sources.py::test_recolour_resets_inside_the_step)
                for e in np.nonzero(over)[0]:
                    ow = ob.world(int(e))
                    ow.reset()
                    for s in range(L):
                        h = oracle_mod.action_hash(seed ^ RECOLOUR_SALT, int(e), env._t, s)
                        colours[e, s] = (h * A) >> 16
                        ow.set_source(s, colour=int(colours[e, s]))
            w.obs_rows.fill_(55)
            env.step(torch.from_numpy(actions).cuda(), auto_reset=True, fused=True)
            ostep = ob.step(actions, auto_reset=not randomize)
            eng = unpack_engine(w.host_buffers(), *dims_of(ob))
            where = f"mode {mode} post_first={post_first} n={n} t={t}"
            if randomize:
                assert np.array_equal(eng["ev_count"] >> 7, over.astype(np.uint8)), f"{where}: which envs were reset"
                eng["ev_count"] = eng["ev_count"] & 0x7F
                assert np.array_equal(w.src_colour.cpu().numpy()[:, :L], colours), where
            assert_step_equal(eng, ostep, where)
            assert_state_equal(eng, ob.dump(), where)
            tot.add(w, ob, ostep, oracle_resets=over if randomize else None)
        assert tot.oracle[6] > 0
        tot.check(w, f"mode {mode} post_first={post_first} n={n}")
    assert f"step_kernel<4,4,{mode},true,3>" in _capi.launched_kernels()


# ---- field width: a whole wavefront of 64 environments does the same thing in the same step

def find_plan(oracle_mod, text, goal):
    """The shortest joint-action sequence of a ONE-agent map after which `goal(world)` holds: breadth first, every node replayed from reset."""
    w = oracle_mod.OracleWorld(text)
    assert w.n_agents == 1
    seen, queue = set(), collections.deque([()])
    while queue:
        plan = queue.popleft()
        w.reset()
        for a in plan:
            w.step([a])
        if goal(w):
            return list(plan)
        key = (tuple(w.positions()[0]), tuple(w.gems_collected()), tuple(w.alive()))
        if key in seen or not all(w.alive()):
            continue
        seen.add(key)
        for a in w.available_actions()[0]:
            queue.append(plan + (a,))
    raise AssertionError("no plan")


def replay(oracle_mod, monkeypatch, text, n, plan, post_first):
    """Every environment plays `plan`, then -- reset by the next step -- an action that is unavailable at the start.  Returns the per-step
    [n, 4] reward counts, the per-step refusals and resets."""
    import torch

    from lle_amd import BatchedWorld

    set_rules(monkeypatch, "1", post_first, epw=64)
    w0 = oracle_mod.OracleWorld(text)
    refused = [a for a in range(4) if a not in w0.available_actions()[0]][0]
    ob = oracle_mod.OracleBatch(text, n)
    bw = BatchedWorld(text, n)
    assert bw.tuning()["envs_per_wave"] == 64 and bw.kernel_info()["kernel"].startswith("step_kernel<1,")
    tot = Totals(1)
    rewards, refusals, resets = [], [], []
    for t, a in enumerate(plan + [refused, 4]):
        actions = np.full((n, 1), a, np.uint8)
        bw.step(torch.from_numpy(actions).cuda(), auto_reset=True)
        ostep = ob.step(actions, auto_reset=True)
        check(bw, ob, ostep, f"n={n} t={t}")
        want, was_reset = tot.add(bw, ob, ostep)
        rewards.append(want)
        refusals.append(ostep["err"] != 0)
        resets.append(was_reset)
    tot.check(bw, f"n={n} post_first={post_first}")
    return rewards, refusals, resets


@pytest.mark.parametrize("post_first", POST, ids=POST_IDS)
@pytest.mark.parametrize("n", [128, 70])
def test_every_field_at_64_in_one_wavefront(oracle_mod, monkeypatch, n, post_first):
    plan = find_plan(oracle_mod, LEVELS[1], lambda w: all(w.arrived()) and all(w.gems_collected()))
    rewards, refusals, resets = replay(oracle_mod, monkeypatch, LEVELS[1], n, plan, post_first)
    # in some step EVERY environment -- so all 64 of the first wavefront -- collects / arrives and earns the bonus / is reset / is refused
    for col, what in ((0, "gems"), (1, "exits"), (3, "bonus")):
        assert any(r[:, col].all() for r in rewards), what
    assert any(r.all() for r in refusals) and any(r.all() for r in resets)
    # ... and dies: one agent, a beam of another colour two cells from its start
    lethal = EXTRA_MAPS["colour_alias"]
    plan = find_plan(oracle_mod, lethal, lambda w: not all(w.alive()))
    rewards, refusals, resets = replay(oracle_mod, monkeypatch, lethal, n, plan, post_first)
    assert any(r[:, 2].all() for r in rewards) and any(r.all() for r in refusals) and any(r.all() for r in resets)


# ---- other paths

def test_eight_agents(oracle_mod):
    from lle_amd import BatchedWorld

    n = 16
    ob = oracle_mod.OracleBatch(EIGHT_AGENTS, n)
    bw = BatchedWorld(EIGHT_AGENTS, n)
    assert bw.kernel_info()["kernel"].startswith("step_kernel<8,")
    tot = Totals(ob.A)
    for t in range(STEPS):
        bw.step(sample=True, auto_reset=True, seed=8, t=t)
        ostep = ob.step(None, auto_reset=True, seed=8, t=t)
        check(bw, ob, ostep, f"eight agents t={t}")
        tot.add(bw, ob, ostep)
    assert tot.oracle[4] > 0 and tot.oracle[6] > 0
    tot.check(bw, "eight agents")


def test_fused_rollout_counts_like_single_steps(oracle_mod):
    import torch

    from lle_amd import BatchedWorld

    n, T = 203, 8
    a, b = BatchedWorld(LEVELS[6], n), BatchedWorld(LEVELS[6], n)
    ob = oracle_mod.OracleBatch(LEVELS[6], n)
    for t0 in (0, T):  # (the second rollout starts among finished environments)
        a.rollout(T, auto_reset=True, seed=17, t=t0)
        for j in range(T):
            b.step(sample=True, auto_reset=True, seed=17, t=t0 + j)
    stats = np.zeros(8, np.int64)
    for t in range(2 * T):
        ostep = ob.step(None, auto_reset=True, seed=17, t=t, stats=stats)
    check(a, ob, None, "after the rollouts")
    for k in ("pos", "bits", "gems", "beams", "avail", "err", "evcount", "events", "done", "obs"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    sa = a.stats()
    assert sa == b.stats()
    assert [sa[k] for k in KEYS[:7]] == stats[:7].tolist()


@pytest.mark.parametrize("epw", [8, 64])
def test_lane_per_environment_step(oracle_mod, epw):
    from lle_amd import BatchedWorld

    n = 203
    ob = oracle_mod.OracleBatch(LEVELS[6], n)
    bw = BatchedWorld(LEVELS[6], n, envs_per_wave=epw)  # (lle_batch_set_envs_per_wave: world_kernel steps)
    tot = Totals(ob.A)
    for t in range(12):
        bw.step(sample=True, auto_reset=True, seed=5, t=t)
        ostep = ob.step(None, auto_reset=True, seed=5, t=t)
        check(bw, ob, ostep, f"epw={epw} t={t}")
        tot.add(bw, ob, ostep)
    tot.check(bw, f"lane per environment epw={epw}")
