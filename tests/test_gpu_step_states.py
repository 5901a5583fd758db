"""Steps from set states over every joint action (tests/step_states.py) through the step kernels, map x launch variant.

Every case: create the batch, apply the variant's layout (two maps, per-environment sources), `set_state` the whole batch in one
launch -- err 0 everywhere, the full state and the observation against the oracle --, take the explicit step (one env per state
and joint action, refusals by every agent included), two sampled steps without auto-reset (they start from stale beams and corpses
no set_state can produce) and one with auto-reset (envs finished by the last arrival or by a death restart).  After every step,
every env: pos, alive / arrived / occupant bits, gems, beams (chained words through first_words), avail, actions, err, ev_count,
ordered events, the whole int8 observation, done, the reward counters -- equality, no tolerance: every quantity is integral or an
exactly representable float32.  The oracle decides everywhere; no output is compared with another kernel's.

The launch rule picks G, LM, ML1 and LX; the variant only drives the MODE, and every case asserts that its step_kernel<G,LM,MODE,ML1,LX>
is among lle_debug_launched() (`-s` prints it).  Not every map can take every variant:

* heads (MODE 6 / 7 / 8) need at most 8 beam words and a row whose planes leave whole 128-byte lines without a dynamic byte:
  HEAD_MAPS / PES_HEAD_MAPS; the 4 x 4 to 6 x 6 maps (colour_alias, four_layers, exit_under_beam, voids_gems, q1_pair, q1, three_beams;
  solo_beams and gems32 under per-env sources) have rows of one or two lines, im_3_20, im_13_12x and many_agents more than 8 beam words;
* the partial writer (MODE 9) serves at most 8 beam words (not im_3_20, im_13_12x, many_agents), and on colour_alias the reference
  itself raises IndexError (a laser colour without a layer);
* per-environment sources need a source: not gems32.

The coverage of the batches (which classes of steps they hold) is asserted on the CPU, tests/test_step_states_cpu.py."""
import functools
import time

import numpy as np
import pytest

from tests import instantiation_maps as im
from tests import step_states as ss
from tests.parity_util import assert_set_state_events, assert_state_equal, assert_step_equal, legal_colours, unpack_engine

pytestmark = pytest.mark.gpu

HEAD_MAPS = ["solo_beams", "long_q1", "gems32", "nested", "long_crossing", "long_three_words", "im_7_7x"]
PES_HEAD_MAPS = ["long_q1", "nested", "long_crossing", "long_three_words", "im_7_7x"]
NO_PARTIAL = ["colour_alias", "im_3_20", "im_13_12x", "many_agents"]
SMALL = ("pos", "bits", "gems", "beams", "avail", "actions", "err", "evcount", "events", "done")

CASES = ([(name, "step") for name in ss.MAP_NAMES] + [(name, "heads") for name in HEAD_MAPS] +
         [(name, "outputs") for name in ss.MAP_NAMES] + [(name, "outputs-heads") for name in HEAD_MAPS] +
         [(name, "per-env") for name in ss.MAP_NAMES if name != "gems32"] + [(name, "per-env-heads") for name in PES_HEAD_MAPS] +
         [(name, "partial") for name in ss.MAP_NAMES if name not in NO_PARTIAL] +
         [(name, "rollout") for name in ss.MAP_NAMES] + [(name, "incremental") for name in ss.MAP_NAMES])
MODE = {"step": 0, "heads": 6, "outputs": 4, "outputs-heads": 7, "per-env": 5, "per-env-heads": 8, "partial": 9, "rollout": 1, "incremental": 0}


def kernel_name(m, mode):
    """The instantiation the launch rule takes for map `m` in `mode` (lle_amd/csrc/step_kernel.hpp launch_step_mode*)."""
    lm, ml1 = im.lm_of(m.n_beam_words), m.max_cell_layers <= 1
    lx = m.n_beam_words if (lm == 4 and ml1) else -1
    return f"step_kernel<{ss.group_size(m.n_agents)},{lm},{mode},{'true' if ml1 else 'false'},{lx}>"


@functools.lru_cache(maxsize=None)
def _reference(name):
    from oracle import oracle
    return ss.reference_run(oracle, ss.build_case(name))


def _observer_extras(ob):
    """What LLE.step returns besides the observation, from oracle/observers.py, for every env."""
    from oracle import observers as oo
    worlds = [ob.world(e) for e in range(ob.n)]
    return {"state": np.stack([oo.state_observe(w, False)[0] for w in worlds]), "state_norm": np.stack([oo.state_observe(w, True)[0] for w in worlds]),
            "available": np.stack([oo.available_actions(w, True) for w in worlds])}


@functools.lru_cache(maxsize=None)
def _reference_blocks(name):
    """Two blocks of one two-map batch: the map and its variant-1 twin where instantiation_maps can build one, else the same text twice."""
    from oracle import oracle
    variants = (0, 1) if ss.has_twin(name) else (0, 0)
    per = ss.block_size(min(ss.build_case(name, v).n for v in variants))
    return [ss.reference_run(oracle, ss.build_case(name, v, n=per), env_offset=ss.ENV_OFFSET + m * per, extras=_observer_extras) for m, v in enumerate(variants)]


@functools.lru_cache(maxsize=None)
def _reference_per_env(name):
    from oracle import oracle
    from lle_amd import _capi
    from tests.test_gpu_env_sources import Mirror
    case = ss.build_case(name)
    m = _capi.Map(case.text)
    L = m.n_sources
    rng = np.random.default_rng(100 + ss.MAP_NAMES.index(name))
    colours = legal_colours(m, rng.integers(0, case.A, size=(case.n, L), dtype=np.uint8))
    enabled = rng.integers(0, 1 << L, size=case.n, dtype=np.int64)
    ref = ss.reference_run(oracle, case, sources=lambda ob: Mirror(ob, case.n, L).apply(colours, enabled, None), rng=rng)
    ref.colours, ref.enabled = colours, enabled
    return ref


@functools.lru_cache(maxsize=None)
def _reference_rollout(name):
    """One launch has one auto-reset flag: the explicit step and three sampled ones without auto-reset are ONE fused rollout of four
    steps, the step with auto-reset a second launch of the rollout kernel."""
    from oracle import oracle
    return ss.reference_run(oracle, ss.build_case(name), follow_ups=[(1, False), (2, False), (3, False), (4, True)])


@functools.lru_cache(maxsize=None)
def _reference_partial(name):
    from oracle import oracle
    from oracle import observers as oo
    case = ss.build_case(name)
    ks = iter([3, 3, 5, 3, 5])  # (after set_state: unused; then k = 3 and 5 alternating, tests/test_gpu_instantiations.py)

    def extras(ob):
        k = next(ks)
        return {"k": k, "partial": np.stack([oo.partial_observe(ob.world(e), k) for e in range(ob.n)]),
                "state": np.stack([oo.state_array(ob.world(e)) for e in range(ob.n)])}
    return ss.reference_run(oracle, case, extras=extras)


def _engine(bw, ref, lo, names=SMALL + ("obs",)):
    bufs = {k: v[lo:lo + ref.case.n] for k, v in bw.host_buffers(names).items()}
    return unpack_engine(bufs, *ref.ob.dims), bufs


def _check_set_state(bw, refs, tag):
    err = bw.err.cpu().numpy()
    assert not err.any(), f"{tag}: set_state refused envs {np.nonzero(err)[0][:8].tolist()} (codes {err[err != 0][:8].tolist()}) that the oracle accepts"
    lo = 0
    for m, ref in enumerate(refs):
        eng, bufs = _engine(bw, ref, lo)
        rec = ref.after_set_state
        assert_state_equal(eng, rec["dump"], f"{tag} after set_state, block {m}")
        assert_set_state_events(eng, rec, f"{tag} after set_state, block {m}")
        assert np.array_equal(eng["obs"], rec["obs"]), f"{tag}: observation after set_state, block {m}"
        assert np.array_equal(bufs["done"], rec["done"]), f"{tag}: done after set_state, block {m}"
        lo += ref.case.n


def _check_step(bw, refs, k, tag, check_obs=True):
    reward = bw.reward.cpu().numpy().astype(np.int64)
    lo = 0
    for m, ref in enumerate(refs):
        rec, where = ref.steps[k], f"{tag} t={ref.steps[k]['t']} block {m}"
        eng, bufs = _engine(bw, ref, lo, SMALL + (("obs",) if check_obs else ()))
        assert_step_equal(eng, rec["ostep"], where, check_obs=check_obs)
        assert_state_equal(eng, rec["dump"], where)
        assert np.array_equal(bufs["done"], rec["done"]), f"{where}: done"
        assert np.array_equal(reward[lo:lo + ref.case.n], rec["reward"]), f"{where}: reward counters [gems, exits, deaths, all arrived]"
        lo += ref.case.n


def _requests(refs):
    import torch
    cat = lambda key: torch.from_numpy(np.concatenate([getattr(r.case, key) for r in refs]))  # noqa: E731
    return cat("pos"), cat("gems"), cat("alive")


def _take_step(bw, refs, k, **kw):
    import torch
    rec = refs[0].steps[k]
    if rec["actions"] is not None:
        acts = np.concatenate([r.steps[k]["actions"] for r in refs])
        bw.step(torch.from_numpy(acts).cuda(), auto_reset=rec["auto_reset"], **kw)
    else:
        bw.step(sample=True, auto_reset=rec["auto_reset"], seed=ss.SEED, t=rec["t"], env_offset=ss.ENV_OFFSET, **kw)


def _sentinel_outputs(n, A, G, multi):
    import torch
    return dict(state=torch.full((n, 3 * A + G), -7.0, device="cuda"), reward=torch.full((n, 4 if multi else 1), -7.0, device="cuda"),
                done=torch.full((n,), 9, dtype=torch.uint8, device="cuda"), available=torch.full((n, A, 5), 9, dtype=torch.uint8, device="cuda"),
                alive=torch.full((n, A), 9, dtype=torch.uint8, device="cuda"), arrived=torch.full((n, A), 9, dtype=torch.uint8, device="cuda"))


def _check_outputs(outs, refs, k, multi, norm, tag):
    got = {key: t.cpu().numpy() for key, t in outs.items()}
    lo = 0
    for m, ref in enumerate(refs):
        rec, sl, where = ref.steps[k], slice(lo, lo + ref.case.n), f"{tag} t={ref.steps[k]['t']} block {m}"
        want_state = rec["extras"]["state_norm" if norm else "state"]
        assert np.array_equal(got["state"][sl].view(np.int32), want_state.view(np.int32)), f"{where}: state"
        assert np.array_equal(got["available"][sl], rec["extras"]["available"].astype(np.uint8)), f"{where}: available"
        assert np.array_equal(got["alive"][sl], rec["dump"]["alive"]) and np.array_equal(got["arrived"][sl], rec["dump"]["arrived"]), f"{where}: alive / arrived"
        assert np.array_equal(got["done"][sl], rec["done"].astype(np.uint8)), f"{where}: done"
        r = rec["reward"].astype(np.float32)
        if multi:  # MultiObjective.compute_reward (reward_strategy.py:90-109): [gem, exit, death, done], a death zeroes the others
            dead = r[:, 2] > 0
            want = np.stack([np.where(dead, 0, r[:, 0]), np.where(dead, 0, r[:, 1]), -r[:, 2], np.where(dead, 0, r[:, 3])], axis=1).astype(np.float32)
        else:      # SingleObjective.compute_reward (reward_strategy.py:58-75)
            want = (r[:, 0] + r[:, 1] - r[:, 2] + r[:, 3])[:, None]
        assert np.array_equal(got["reward"][sl], want), f"{where}: reward"
        lo += ref.case.n


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_steps_from_set_states(monkeypatch, case):
    import torch

    from lle_amd import BatchedWorld, _capi

    name, variant = case
    tag = f"{name} {variant}"
    t_start = time.perf_counter()
    heads = variant in ("heads", "outputs-heads", "per-env-heads")
    monkeypatch.setenv("LLE_ROW_HEADS", "1" if heads else "0")
    two_maps = variant in ("outputs", "outputs-heads")
    if two_maps:
        refs = _reference_blocks(name)
    elif variant in ("per-env", "per-env-heads"):
        refs = [_reference_per_env(name)]
    elif variant == "rollout":
        refs = [_reference_rollout(name)]
    elif variant == "partial":
        refs = [_reference_partial(name)]
    else:
        refs = [_reference(name)]
    n = sum(r.case.n for r in refs)
    A, G = refs[0].case.A, refs[0].case.G
    texts = [r.case.text for r in refs]
    bw = BatchedWorld(texts if two_maps else texts[0], n, row_align=128 if heads else None, incremental_obs=(variant == "incremental"))
    if heads:
        assert bw.map.n_beam_words <= 8 and (bw.map.row_head_env_sources if variant == "per-env-heads" else bw.map.row_head)[1] != 0, tag
    if variant in ("per-env", "per-env-heads"):
        bw.set_sources(torch.from_numpy(refs[0].colours), torch.from_numpy(refs[0].enabled.astype(np.int32)))
        assert int(bw.err.max()) == 0
    bw.set_state(*_requests(refs))
    _check_set_state(bw, refs, tag)

    if variant == "rollout":
        ref = refs[0]
        R = 4
        ring = bw.make_ring(R)
        for k in range(R):  # slot 0: the enumerated joint actions; slots 1 - 3: the oracle's sampled actions of those steps
            ring["actions"][k].copy_(torch.from_numpy(ref.steps[k]["ostep"]["actions"] if k else ref.case.actions))
        bw.rollout(R, auto_reset=False, seed=ss.SEED, t=0, env_offset=ss.ENV_OFFSET, ring=ring, ring_pos=0, sample=False)
        last = ref.steps[R - 1]
        eng, bufs = _engine(bw, ref, 0, SMALL)  # (a rollout into a ring leaves the batch's own rows alone)
        obs_ring, act_ring, rew_ring = ring["obs"].cpu().numpy(), ring["actions"].cpu().numpy(), ring["reward"].cpu().numpy().astype(np.int64)
        # (a planned rollout READS its actions from the ring and leaves LLE_BUF_ACTIONS alone: the step's actions are the slot's, and
        # the slots must still hold the plan afterwards)
        eng["actions"] = act_ring[R - 1]
        assert_state_equal(eng, last["dump"], f"{tag} after the rollout of {R}")
        assert_step_equal(eng, last["ostep"], f"{tag} after the rollout of {R}")
        assert np.array_equal(bufs["done"], last["done"]), f"{tag}: done after the rollout"
        for k in range(R):
            assert np.array_equal(obs_ring[k], ref.steps[k]["ostep"]["obs"]), f"{tag}: ring observation of step {k}"
            assert np.array_equal(act_ring[k], ref.steps[k]["ostep"]["actions"]), f"{tag}: the plan in ring slot {k} was overwritten"
            assert np.array_equal(rew_ring[k], ref.steps[k]["reward"]), f"{tag}: ring reward counters of step {k}"
        ring["actions"][0].copy_(torch.from_numpy(ref.steps[R]["ostep"]["actions"]))
        bw.rollout(1, auto_reset=True, seed=ss.SEED, t=R, env_offset=ss.ENV_OFFSET, ring=ring, ring_pos=R, sample=False)
        eng, bufs = _engine(bw, ref, 0, SMALL)
        eng["actions"] = ring["actions"][0].cpu().numpy()
        assert_state_equal(eng, ref.steps[R]["dump"], f"{tag} after the auto-reset step")
        assert_step_equal(eng, ref.steps[R]["ostep"], f"{tag} after the auto-reset step")
        assert np.array_equal(bufs["done"], ref.steps[R]["done"]), f"{tag}: done after the auto-reset step"
        assert np.array_equal(ring["obs"][0].cpu().numpy(), ref.steps[R]["ostep"]["obs"]), f"{tag}: ring observation of the auto-reset step"
        assert np.array_equal(ring["reward"][0].cpu().numpy().astype(np.int64), ref.steps[R]["reward"]), f"{tag}: ring reward of the auto-reset step"
    elif two_maps:
        for norm_multi in (False, True):  # plain, then normalised state + multi-objective reward: the same states again
            if norm_multi:
                bw.reset()  # (the oracle's worlds took their requests freshly reset)
                bw.set_state(*_requests(refs))
                _check_set_state(bw, refs, tag)
            outs = _sentinel_outputs(n, A, G, norm_multi)
            env_out = bw.make_env_outputs(normalize_state=norm_multi, multi_objective=norm_multi, **outs)
            for k in range(len(refs[0].steps)):
                _take_step(bw, refs, k, env_out=env_out)
                _check_step(bw, refs, k, tag)
                _check_outputs(outs, refs, k, norm_multi, norm_multi, f"{tag} {'normalised + multi-objective' if norm_multi else 'plain'}")
    elif variant == "partial":
        ref = refs[0]
        bufs = {k: bw.partial_buffer(k) for k in (3, 5)}
        state = torch.full((n, 3 * A + G), -7.0, dtype=torch.float32, device="cuda")
        for k, rec in enumerate(ref.steps):
            pk = rec["extras"]["k"]
            bufs[pk][0].fill_(0x55)
            _take_step(bw, refs, k, env_out=bw.make_env_outputs(state=state, partial=bufs[pk][0], partial_k=pk), write_obs=False)
            _check_step(bw, refs, k, tag, check_obs=False)
            assert np.array_equal(bufs[pk][1].cpu().numpy().astype(np.float32), rec["extras"]["partial"]), f"{tag} t={rec['t']}: partial {pk} x {pk}"
            assert np.array_equal(state.cpu().numpy(), rec["extras"]["state"]), f"{tag} t={rec['t']}: state"
    else:
        for k in range(len(refs[0].steps)):
            _take_step(bw, refs, k)
            _check_step(bw, refs, k, tag)
            if variant == "incremental":
                assert bw.check_obs() == 0, f"{tag}: rows differ from the state after an incremental step"

    want = kernel_name(bw.map, MODE[variant])
    assert want in _capi.launched_kernels(), f"{tag} was meant to launch {want}"
    stepped = float(np.mean(np.concatenate([r.steps[0]["ostep"]["err"] for r in refs]) == 0))
    print(f"\n[step-states] {tag}: {want} envs={n} stepped={stepped:.3f} wall={time.perf_counter() - t_start:.2f}s")


def test_a_second_round_of_vertex_conflicts_through_stale_availability(oracle_mod, monkeypatch):
    """The one situation in which solve_vertex_conflicts needs a second round (tests/step_states.py STALE_MAP): after a set_state that is
    refused with InvalidWorldState and not rolled back, the stale availability lists let an agent walk onto the cell another one is
    sent back to.  step_kernel<4,4,0,true,1>, 21 identical envs, against the oracle."""
    import torch

    from lle_amd import BatchedWorld, _capi
    from tests.test_step_states_cpu import stale_reference

    monkeypatch.setenv("LLE_ROW_HEADS", "0")
    n = 21
    ob, d0, ostep, d1 = stale_reference(oracle_mod, n)
    bw = BatchedWorld(ss.STALE_MAP, n)
    pos, _gems, alive = ss.STALE_REQUEST
    bw.set_state(torch.tensor([pos] * n, dtype=torch.uint8), torch.zeros((n, 0), dtype=torch.bool), torch.tensor([alive] * n))
    assert bool((bw.err == 0x40).all())
    assert_state_equal(unpack_engine(bw.host_buffers(), *ob.dims), d0, "after the refused set_state")
    bw.step(torch.tensor([ss.STALE_ACTIONS] * n, dtype=torch.uint8).cuda())
    eng = unpack_engine(bw.host_buffers(), *ob.dims)
    assert_step_equal(eng, ostep, "stale availability")
    assert_state_equal(eng, d1, "stale availability")
    assert kernel_name(bw.map, 0) == "step_kernel<4,4,0,true,1>" and kernel_name(bw.map, 0) in _capi.launched_kernels()
