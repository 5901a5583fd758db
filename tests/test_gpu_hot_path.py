"""The hot / cold split of the step kernels with row heads (step_kernel MODE 6 / 7 / 8; obs_stream.hpp HeadPath): a launch with the
default rules -- write-through, every wavefront stores its own heads, no row rotation -- runs the straight-line copies of the head
stores and of the row loop, every other rule the cold copies behind them.  Here every combination of the three rules is forced
(LLE_WRITE_THROUGH x LLE_HEAD_GROUP x LLE_ROW_ROTATE; the existing tests force them one at a time) with row heads on and 16
environments per wavefront, at three batch sizes: 256 (every wavefront full), 203 (a ragged last wavefront beside full ones) and 5
(a single wavefront below its 16 rows).  Eight steps each, sampled and given actions alternating -- the given ones include
unavailable and out-of-range actions, which the step refuses --, auto-reset from the third step on; the rows are filled with garbage
before every step (the launch must write every byte of every row), and every buffer and the int8 observation are compared with the
oracle after every step.

The same through BatchedLLE.step(fused=True) (MODE 7: the fused outputs) and with randomize_lasers (MODE 8: per-environment sources,
finished environments re-coloured inside the step).  BatchedLLE.step takes the actions from the caller, so the `sampled` steps there
are draws from each agent's available actions; its outputs are held against a twin that steps in two launches."""
import itertools

import numpy as np
import pytest

from oracle.levels import LEVELS
from tests.parity_util import assert_state_equal, assert_step_equal, unpack_engine
from tests.test_gpu_parity import check, dims_of

pytestmark = pytest.mark.gpu

EPW = 16
SIZES = (256, 203, 5)
STEPS = 8
RULES = list(itertools.product((6, 3), ("0", "1"), ("1", "2", "4"), ("0", "1")))
IDS = [f"level{lv}-wt{wt}-group{hg}-rot{rot}" for lv, wt, hg, rot in RULES]


def force(monkeypatch, wt, hg, rot):
    for k, v in (("LLE_ROW_HEADS", "1"), ("LLE_STEP_EPW", str(EPW)), ("LLE_WRITE_THROUGH", wt), ("LLE_HEAD_GROUP", hg), ("LLE_ROW_ROTATE", rot)):
        monkeypatch.setenv(k, v)


def assert_rules(bw, wt, hg, rot):
    t = bw.tuning()
    got = {k: t[k] for k in ("row_heads", "envs_per_wave", "write_through", "head_group", "rotate_rows")}
    assert got == dict(row_heads=1, envs_per_wave=EPW, write_through=int(wt), head_group=int(hg), rotate_rows=int(rot)), got


def given_actions(rng, n, A):
    return rng.integers(0, 6, size=(n, A), dtype=np.uint8)  # unavailable and out-of-range (5) included


@pytest.mark.parametrize("level,wt,hg,rot", RULES, ids=IDS)
def test_world_step_under_every_rule(oracle_mod, monkeypatch, level, wt, hg, rot):
    import torch

    from lle_amd import BatchedWorld, Map

    force(monkeypatch, wt, hg, rot)
    rng = np.random.default_rng(level)
    for n in SIZES:
        m = Map(LEVELS[level])
        assert m.row_head[1] > 0
        ob = oracle_mod.OracleBatch(LEVELS[level], n)
        bw = BatchedWorld(m, n)
        assert_rules(bw, wt, hg, rot)
        for t in range(STEPS):
            auto = t >= 2
            bw.obs_rows.fill_(55)
            if t % 2 == 0:
                bw.step(sample=True, auto_reset=auto, seed=77, t=t, env_offset=9)
                ostep = ob.step(None, auto_reset=auto, seed=77, t=t, env_offset=9)
            else:
                actions = given_actions(rng, n, ob.A)
                bw.step(torch.from_numpy(actions).cuda(), auto_reset=auto)
                ostep = ob.step(actions, auto_reset=auto)
            check(bw, ob, ostep, f"level {level} n={n} t={t}")
            if m.obs_stride > m.obs_bytes:
                assert int(bw.obs_rows[:, m.obs_bytes:].abs().max()) == 0  # the padding of a row is written too


def available_draw(rng, avail):
    """One available action per agent, uniformly (avail: bool [n, A, 5])."""
    n, A = avail.shape[:2]
    out = np.zeros((n, A), np.uint8)
    for e in range(n):
        for a in range(A):
            out[e, a] = rng.choice(np.nonzero(avail[e, a])[0])
    return out


@pytest.mark.parametrize("randomize", [False, True], ids=["fused", "fused-randomize_lasers"])
@pytest.mark.parametrize("level,wt,hg,rot", RULES, ids=IDS)
def test_batched_lle_fused_step_under_every_rule(oracle_mod, monkeypatch, level, wt, hg, rot, randomize):
    import torch

    from lle_amd import BatchedLLE
    from lle_amd._capi import RECOLOUR_SALT

    force(monkeypatch, wt, hg, rot)
    rng = np.random.default_rng(10 + level)
    seed = 21
    for n in SIZES:
        env = BatchedLLE(LEVELS[level], n, obs_type="layered", randomize_lasers=randomize, seed=seed)
        twin = BatchedLLE(LEVELS[level], n, obs_type="layered", randomize_lasers=randomize, seed=seed)
        w, m = env.world, env.world.map
        A, L = m.n_agents, m.n_sources
        assert m.row_head[1] > 0 and (not randomize or env._recolour_in_step)
        assert_rules(w, wt, hg, rot)
        env.reset(), twin.reset()
        ob = oracle_mod.OracleBatch(LEVELS[level], n)
        colours = None
        if randomize:  # (reset() draws from the torch generator: the twin and the oracle take the colours it drew)
            colours = w.src_colour[:, :L].cpu().numpy().copy()
            twin.world.set_sources(colours=torch.from_numpy(colours).cuda())
            for e in range(n):
                for s in range(L):
                    ob.world(e).set_source(s, colour=int(colours[e, s]))
        check(w, ob, None, f"level {level} n={n} after reset")
        for t in range(STEPS):
            auto = t >= 2
            over = w.done.cpu().numpy().astype(bool)
            actions = available_draw(rng, env.available_actions().cpu().numpy()) if t % 2 == 0 else given_actions(rng, n, A)
            if auto and randomize:
                # what the kernel does with an environment that is over: world.reset() under the colours it had, then a fresh colour per
                # source from the documented hash (tests/test_gpu_env_sources.py::test_recolour_resets_inside_the_step)
                for e in np.nonzero(over)[0]:
                    ow = ob.world(int(e))
                    ow.reset()
                    for s in range(L):
                        h = oracle_mod.action_hash(seed ^ RECOLOUR_SALT, int(e), env._t, s)  # (keyed by the env's step counter)
                        colours[e, s] = (h * A) >> 16  # (every colour is allowed on these maps)
                        ow.set_source(s, colour=int(colours[e, s]))
            w.obs_rows.fill_(55)
            acts = torch.from_numpy(actions).cuda()
            x, y = env.step(acts, auto_reset=auto, fused=True), twin.step(acts, auto_reset=auto, fused=False)
            ostep = ob.step(actions, auto_reset=auto and not randomize)
            eng = unpack_engine(w.host_buffers(), *dims_of(ob))
            if auto and randomize:
                assert np.array_equal(eng["ev_count"] >> 7, over.astype(np.uint8)), f"level {level} n={n} t={t}: which envs were reset"
                eng["ev_count"] = eng["ev_count"] & 0x7F
            where = f"level {level} n={n} randomize={randomize} t={t}"
            assert_step_equal(eng, ostep, where)
            assert_state_equal(eng, ob.dump(), where)
            if randomize:
                assert np.array_equal(w.src_colour.cpu().numpy()[:, :L], colours), where
            for k in ("obs", "state", "reward", "done", "available_actions", "err"):
                assert torch.equal(x[k], y[k]), (k, where)
