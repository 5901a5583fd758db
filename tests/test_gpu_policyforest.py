"""The forest of steps-to-go tables on the MI355X (liblle_policyforest.so, lle_amd.PolicyForest) against its restatement
(tests/policyforest_ref.py: tests/policy_ref.build per map): every table of every set, state by state -- steps, sentinels and action
digits -- at four piece sizes, caller batches whose environments per map are not the forest's, one forest against one OptimalPolicy per
map, capacity per map, rebuilds, expert rollouts from sampled mid-episode states, the write footprint of the lookup, refusals.

State k of map m of the restatement lies in environment m * E_c + k of a multi-map batch, reached by replaying its prefix of joint
actions (padded with all-STAY rows) or through `set_state` with the restore tests/test_gpu_policy.py uses; spare environments stay at
the reset state."""
import ctypes as C

import numpy as np
import pytest

from tests import policy_ref
from tests import policyforest_ref as R

pytestmark = pytest.mark.gpu

CASES = [(name, horizon) for name in ("A", "B", "C") for horizon in R.HORIZONS]
SIZES = (256, 64, 7, 1)
STATE = ("pos", "bits", "gems", "beams", "avail")
DEVICE = "cuda:0"


@pytest.fixture(scope="module")
def pf_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import policyforest
    return policyforest


_FORESTS, _BATCHES, _COUNTERS = {}, {}, {}


def forest_of(pf_mod, name, horizon, collect_gems=False, **options):
    """One PolicyForest per (set, horizon, options) for the whole module."""
    key = (name, horizon, collect_gems, tuple(sorted(options.items())))
    if key not in _FORESTS:
        _FORESTS[key] = pf_mod.PolicyForest(R.SETS[name].maps, horizon, collect_gems=collect_gems, **options)
    return _FORESTS[key]


def replay(maps, ts, E_c):
    """A BatchedWorld of len(maps) * E_c environments with state k of table ts[m] in environment m * E_c + k."""
    import torch

    from lle_amd import BatchedWorld
    bw = BatchedWorld(list(maps), len(maps) * E_c, device=DEVICE)
    for step, rows in enumerate(R.replay_rows(ts, E_c)):
        bw.step(torch.from_numpy(rows).to(bw.device), write_obs=False)
        assert not bw.err.any().item(), f"the step refused a replayed joint action at step {step}"
    return bw


def replayed(name, horizon, collect_gems=False, E_c=None):
    key = (name, horizon, collect_gems, E_c)
    if key not in _BATCHES:
        ts = R.tables(name, horizon, collect_gems)
        _BATCHES[key] = replay(R.SETS[name].maps, ts, R.envs_per_map(ts) if E_c is None else E_c)
    return _BATCHES[key]


def by_set_state(name, horizon):
    """The same layout through set_state; (batch, number of environments whose record differed from the replayed one: all restored)."""
    import torch

    from lle_amd import BatchedWorld
    if ("set_state", name, horizon) in _BATCHES:
        return _BATCHES[("set_state", name, horizon)]
    ts, twin = R.tables(name, horizon), replayed(name, horizon)
    E_c, A, G = R.envs_per_map(ts), ts[0].n_agents, len(ts[0].states[0].gems)
    n = len(ts) * E_c
    positions, gems = np.zeros((n, A, 2), np.uint8), np.zeros((n, G), bool)
    for m, t in enumerate(ts):
        for k in range(E_c):
            s = t.states[k if k < t.n_states else 0]
            positions[m * E_c + k], gems[m * E_c + k] = s.positions, s.gems
    bw = BatchedWorld(list(R.SETS[name].maps), n, device=DEVICE)
    bw.set_state(torch.from_numpy(positions), torch.from_numpy(gems), torch.ones((n, A), dtype=torch.bool))
    # (World.set_state derives the beams anew, agent by agent: it refuses some states that stepping reaches, where one agent shields another
    # from a beam; such an environment counts as differing and is restored with the others)
    differs = bw.err != 0
    for key in ("pos", "bits", "beams"):
        differs |= (getattr(bw, key) != getattr(twin, key)).view(n, -1).any(1)
    count = int(differs.sum().item())
    if count:
        bw.restore(twin.snapshot())
    _BATCHES[("set_state", name, horizon)] = (bw, count)
    return bw, count


def assert_answers(got_steps, got_actions, want, where):
    want_steps, want_actions = want
    got_steps = got_steps.cpu().numpy()
    assert got_steps.dtype == np.int32 and got_steps.shape == want_steps.shape, where
    bad = np.nonzero(got_steps != want_steps)[0]
    assert bad.size == 0, f"{where}: steps of environments {bad[:8].tolist()}: {got_steps[bad[:8]].tolist()}, restatement {want_steps[bad[:8]].tolist()}"
    if got_actions is not None:
        got_actions = got_actions.cpu().numpy()
        assert got_actions.dtype == np.uint8 and got_actions.shape == want_actions.shape, where
        bad = np.nonzero((got_actions != want_actions).any(1))[0]
        assert bad.size == 0, f"{where}: actions of environments {bad[:8].tolist()}: {got_actions[bad[:8]].tolist()}, restatement {want_actions[bad[:8]].tolist()}"


def assert_lookups(pf, bw, want, where, **kw):
    actions, steps = pf.actions(bw, **kw)
    assert_answers(steps, actions, want, where)
    assert_answers(pf.steps_to_go(bw, **kw), None, want, where + " (steps_to_go alone)")


def assert_tables(pf, ts, where, maps=None):
    """Per map: the counters of the build against the restatement's (`maps`: the maps that have a table; default all)."""
    for m, t in enumerate(ts):
        if maps is not None and m not in maps:
            continue
        got = (int(pf.status[m]), int(pf.n_states[m]), bool(pf.complete[m]), int(pf.depth_reached[m]), int(pf.root_steps[m]))
        assert got == (0, t.n_states, t.complete, t.depth_reached, R.root_answer(t)), (where, m, got)
        stats = pf.stats(m)
        assert stats["frontier"] == t.frontier and stats["expanded"] == t.expanded, (where, m, stats, t.frontier, t.expanded)
        assert int(pf.passes[m]) >= (1 if t.depth_reached else 0), (where, m, pf.passes[m])


# ---------------------------------------------------------------------------------------------------------------- 1. the tables
@pytest.mark.parametrize("E", SIZES)
@pytest.mark.parametrize("name, horizon", CASES)
def test_tables_equal_the_restatement(pf_mod, name, horizon, E):
    ts = R.tables(name, horizon)
    pf = forest_of(pf_mod, name, horizon, envs_per_map=E)
    print(f"{name} h={horizon} E={E}: n_states {pf.n_states.tolist()} depth {pf.depth_reached.tolist()} passes {pf.passes.tolist()} "
          f"explore {pf.explore_ms:.1f} ms relax {pf.relax_ms:.1f} ms occupancy {pf.occupancy['explore']:.2f} / {pf.occupancy['relax']:.2f}")
    assert not pf.over_capacity.any()
    assert_tables(pf, ts, f"{name} h={horizon} E={E}")
    want = R.expected(name, horizon)
    assert_lookups(pf, replayed(name, horizon), want, f"{name} h={horizon} E={E} replayed")
    bw, restored = by_set_state(name, horizon)
    print(f"{restored} of {bw.n_envs} records differed after set_state and were restored")
    assert_lookups(pf, bw, want, f"{name} h={horizon} E={E} set_state")
    # the counters do not depend on E
    mine = (pf.n_states.tolist(), pf.complete.tolist(), pf.depth_reached.tolist(), pf.root_steps.tolist(), [pf.stats(m) for m in range(pf.n_maps)])
    first = _COUNTERS.setdefault((name, horizon), mine)
    assert mine == first
    if E != 256:  # (the forest at the default size serves the tests below)
        _FORESTS.pop((name, horizon, False, (("envs_per_map", E),))).free()


# ---------------------------------------------------------------------------------------------------------------- 2. caller batches
@pytest.mark.parametrize("E_c", [211, 7, 1])
def test_straddling_and_tiny_caller_batches(pf_mod, E_c):
    """Environments per map of the caller's batch that are no multiple of a wavefront, of a workgroup or of the forest's own 256."""
    pf = forest_of(pf_mod, "A", 40, envs_per_map=256)
    assert R.envs_per_map(R.tables("A", 40)) == 211
    assert_lookups(pf, replayed("A", 40, E_c=E_c), R.expected("A", 40, E_c=E_c), f"E_c={E_c}")


def test_single_map_batches_with_map_index(pf_mod):
    from lle_amd import World
    for horizon in R.HORIZONS:
        pf, ts = forest_of(pf_mod, "A", horizon, envs_per_map=256), R.tables("A", horizon)
        for m, t in enumerate(ts):
            answers = [t.answer(s) for s in t.states]
            want = (np.array([a[0] for a in answers], np.int32), np.array([policy_ref.joint_of(a[1], t.n_agents) for a in answers], np.uint8))
            assert_lookups(pf, replay([t.text], [t], t.n_states), want, f"h={horizon} map_index={m}", map_index=m)
        world = World(ts[3].text)
        world.reset()
        assert pf.steps_to_go(world, map_index=3).cpu().tolist() == [R.root_answer(ts[3])]


# ---------------------------------------------------------------------------------------------------------------- 3. against OptimalPolicy
def test_one_forest_against_sixteen_single_policies(pf_mod):
    import torch

    from lle_amd import OptimalPolicy
    ts = R.tables("A", 6)
    pf, E_c = forest_of(pf_mod, "A", 6, envs_per_map=256), R.envs_per_map(ts)
    actions, steps = pf.actions(replayed("A", 6))
    for m, t in enumerate(ts):
        one = OptimalPolicy(t.text, 6)
        single = replay([t.text], [t], E_c)
        a, s = one.actions(single)
        assert (one.n_states, one.complete, one.depth_reached) == (int(pf.n_states[m]), bool(pf.complete[m]), int(pf.depth_reached[m]))
        assert pf.stats(m) == dict(frontier=one.stats["frontier"], expanded=one.stats["expanded"])
        assert torch.equal(s, steps[m * E_c:(m + 1) * E_c]) and torch.equal(a, actions[m * E_c:(m + 1) * E_c]), m
        if m == 2:  # a forest of one map is an OptimalPolicy; the same map twice gives twice the same table
            lone = pf_mod.PolicyForest([t.text], 6)
            b, r = lone.actions(single)
            assert torch.equal(b, a) and torch.equal(r, s) and lone.n_states.tolist() == [one.n_states]
            assert torch.equal(lone.steps_to_go(single, map_index=0), s)
            twice = pf_mod.PolicyForest([t.text, t.text], 6, envs_per_map=64)
            assert twice.n_states.tolist() == [one.n_states] * 2 and twice.stats(0) == twice.stats(1) == pf.stats(m)
            both = replay([t.text, t.text], [t, t], E_c)
            b, r = twice.actions(both)
            assert torch.equal(b[:E_c], a) and torch.equal(b[E_c:], a) and torch.equal(r[:E_c], s) and torch.equal(r[E_c:], s)
            lone.free(), twice.free()
        one.free()


# ---------------------------------------------------------------------------------------------------------------- 4. capacity
@pytest.mark.parametrize("cap, fitting", [(128, [1, 8, 13, 14]), (211, list(range(16))), (210, [m for m in range(16) if m != 5])])
def test_capacity_is_per_map(pf_mod, cap, fitting):
    ts = R.tables("A", 40)
    assert fitting == [m for m, t in enumerate(ts) if t.n_states <= cap]
    pf = pf_mod.PolicyForest(R.SET_A.maps, 40, max_states_per_map=cap)
    assert np.flatnonzero(~pf.over_capacity).tolist() == fitting
    assert (pf.status[pf.over_capacity] == pf_mod.LLE_POLICY_CAPACITY).all() and (pf.status[~pf.over_capacity] == 0).all()
    assert not pf.complete[pf.over_capacity].any() and (pf.root_steps[pf.over_capacity] == pf.UNKNOWN).all()
    assert_tables(pf, ts, f"cap={cap}", maps=fitting)
    E_c = R.envs_per_map(ts)
    steps, actions = (a.copy() for a in R.expected("A", 40))
    for m in range(16):
        if m not in fitting:  # every environment of a map over capacity reads UNKNOWN with all-STAY
            steps[m * E_c:(m + 1) * E_c], actions[m * E_c:(m + 1) * E_c] = pf.UNKNOWN, policy_ref.STAY
    assert_lookups(pf, replayed("A", 40), (steps, actions), f"cap={cap}")
    pf.free()


# ---------------------------------------------------------------------------------------------------------------- 5. rebuild
def test_rebuild(pf_mod):
    assert all(t.states[0].gems == [False] for t in R.tables("A", 6))  # one gem per map
    pf = pf_mod.PolicyForest(R.SET_A.maps, 6, envs_per_map=64)
    for horizon, collect_gems in ((6, False), (40, False), (6, True)):
        if (horizon, collect_gems) != (6, False):
            assert pf.rebuild(horizon=horizon, collect_gems=collect_gems) is pf
        where = f"rebuilt h={horizon} collect_gems={collect_gems}"
        assert (pf.horizon, pf.collect_gems) == (horizon, collect_gems)
        assert_tables(pf, R.tables("A", horizon, collect_gems), where)
        assert_lookups(pf, replayed("A", horizon, collect_gems), R.expected("A", horizon, collect_gems), where)
    assert R.tables("A", 6, True)[0].n_states != R.tables("A", 6)[0].n_states
    pf.free()


# ---------------------------------------------------------------------------------------------------------------- 6. rollouts
def alive_of(bits, A):
    import torch
    return (((bits.unsqueeze(1) >> torch.arange(A, device=bits.device)) & 1) == 1).all(1)


def arrived_of(bits, A):
    import torch
    return (((bits.unsqueeze(1) >> (16 + torch.arange(A, device=bits.device))) & 1) == 1).all(1)


@pytest.mark.parametrize("auto_reset", [False, True], ids=["BatchedWorld", "BatchedLLE-auto-reset"])
def test_expert_rollouts(pf_mod, auto_reset):
    """Every environment with an answer s >= 0 arrives after exactly s steps of act + step and its answer falls by one per step; every
    DEAD_END environment has a dead agent or a state the restatement calls a dead end.  (With auto-reset an environment is followed
    until it arrives: the step after that resets it.)"""
    import torch

    from lle_amd import BatchedLLE, BatchedWorld
    cfg = R.ROLLOUT
    name, E, A = cfg["name"], cfg["envs_per_map"], 2
    pf = forest_of(pf_mod, name, cfg["horizon"], envs_per_map=256)
    assert pf.complete.all()
    n = pf.n_maps * E
    env = BatchedLLE(list(R.SETS[name].maps), n, device=DEVICE) if auto_reset else BatchedWorld(list(R.SETS[name].maps), n, device=DEVICE)
    bw = env.world if auto_reset else env
    for t in range(cfg["steps"]):
        bw.step(sample=True, auto_reset=auto_reset, seed=cfg["seed"], t=t, write_obs=False)
    want, want_alive = R.sampled_answers(name, cfg["horizon"], cfg["seed"], cfg["steps"], E, auto_reset)
    classes = R.rollout_classes(want, want_alive, E)
    print(f"{classes[0]} environments with an answer, {classes[1]} with a dead agent, {classes[2]} dead ends with everybody alive")
    assert all(c > 0 for c in classes[:3]) and classes[3] == 0
    alive = alive_of(bw.bits, A)
    assert np.array_equal(alive.cpu().numpy(), want_alive)
    first = pf.steps_to_go(env)
    assert np.array_equal(first.cpu().numpy(), want)
    followed = first >= 0
    stay = torch.full((A,), policy_ref.STAY, dtype=torch.uint8, device=bw.device)
    solved_at = torch.full((n,), -1, dtype=torch.int64, device=bw.device)
    for k in range(int(first.max().item()) + 1):
        running = followed & (solved_at < 0)
        solved_at = torch.where(running & arrived_of(bw.bits, A), torch.full_like(solved_at, k), solved_at)
        running = followed & (solved_at < 0)
        before = {key: getattr(bw, key).clone() for key in STATE}
        steps = pf.act(env)
        for key in STATE:  # the lookup writes the action buffer and nothing else
            assert torch.equal(getattr(bw, key), before[key]), key
        assert torch.equal(steps[running], first[running] - k)
        assert (bw.actions[steps < 0] == stay).all().item() and (bw.actions[steps == 0] == stay).all().item()
        if auto_reset:
            env.step(bw.actions, auto_reset=True)
        else:
            bw.step(bw.actions, write_obs=False)
            assert torch.equal(steps[followed], torch.clamp(first[followed] - k, min=0))
            assert (steps[~followed] == pf.DEAD_END).all().item()
        assert not bw.err[running].any().item()
        assert alive_of(bw.bits, A)[running].all().item(), "an expert action killed an agent"
    assert torch.equal(solved_at[followed], first[followed].to(torch.int64)), "every environment arrives after exactly its first steps_to_go steps"


# ---------------------------------------------------------------------------------------------------------------- 7. the write footprint
def test_write_footprint(pf_mod):
    """Guard bytes around steps_out, an action pitch wider than A: only steps_out[e] and the bytes [0, A) of every row change; the
    caller batch's whole arena -- the state buffers and everything else of it -- is bit-identical before and after."""
    import torch

    pf, bw = forest_of(pf_mod, "A", 40, envs_per_map=256), replayed("A", 40)
    n, A, pitch, guard = bw.n_envs, 2, 5, 64
    L = pf_mod.lib()
    for fill in (0x00, 0xA5):
        steps = torch.full((guard + n + guard,), -1 if fill else 0x5A5A5A5A, dtype=torch.int32, device=bw.device)
        actions = torch.full((guard + n * pitch + guard,), fill, dtype=torch.uint8, device=bw.device)
        steps_before, actions_before = steps.clone(), actions.clone()
        state = {key: getattr(bw, key).clone() for key in STATE + ("actions", "err")}
        arena = bw._base.clone()  # every byte of the batch on the device
        rc = L.lle_policyforest_lookup(pf.h, bw.h, -1, steps.data_ptr() + 4 * guard, actions.data_ptr() + guard, pitch, bw._stream())
        assert rc == 0, L.lle_policyforest_last_error()
        torch.cuda.synchronize()
        assert torch.equal(steps[:guard], steps_before[:guard]) and torch.equal(steps[guard + n:], steps_before[guard + n:])
        assert torch.equal(actions[:guard], actions_before[:guard]) and torch.equal(actions[guard + n * pitch:], actions_before[guard + n * pitch:])
        rows, rows_before = actions[guard:guard + n * pitch].view(n, pitch), actions_before[guard:guard + n * pitch].view(n, pitch)
        assert torch.equal(rows[:, A:], rows_before[:, A:])
        assert_answers(steps[guard:guard + n], rows[:, :A], R.expected("A", 40), f"fill {fill:#x}")
        for key, kept in state.items():
            assert torch.equal(getattr(bw, key), kept), key
        assert torch.equal(bw._base, arena)


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals(pf_mod):
    import torch

    from lle_amd import BatchedWorld, Map
    maps = list(R.SET_A.maps)
    pf = forest_of(pf_mod, "A", 40, envs_per_map=256)
    with pytest.raises(ValueError, match="holds 15 maps, the forest 16"):
        pf.steps_to_go(BatchedWorld(maps[:15], 30, device=DEVICE))
    swapped = BatchedWorld(maps[:7] + [maps[8], maps[7]] + maps[9:], 32, device=DEVICE)
    with pytest.raises(ValueError, match="map 7 of the env is not map 7 of the forest"):
        pf.steps_to_go(swapped)
    assert pf.steps_to_go(swapped, check_map=False).shape == (32,)  # the caller vouches for the maps: the call runs
    single = BatchedWorld(maps[4], 3, device=DEVICE)
    for index in (-1, 16):
        with pytest.raises(ValueError, match="map_index must be 0 .. 15"):
            pf.steps_to_go(single, map_index=index)
    with pytest.raises(ValueError, match="fingerprint"):
        pf.steps_to_go(single, map_index=5)
    with pytest.raises(ValueError, match="of that map alone"):
        pf.steps_to_go(swapped, map_index=5)
    with pytest.raises(ValueError, match="holds 1 maps, the forest 16"):
        pf.steps_to_go(single)
    with pytest.raises(ValueError, match="agents"):
        pf.steps_to_go(BatchedWorld(["S0 . X"] * 16, 16, device=DEVICE), check_map=False)
    sourced = BatchedWorld(maps, 32, device=DEVICE)
    assert pf.steps_to_go(sourced).shape == (32,)
    sourced.set_sources(enabled=torch.zeros(32, dtype=torch.int32))
    with pytest.raises(ValueError, match="per-environment sources"):
        pf.steps_to_go(sourced)
    env = BatchedWorld(maps, 32, device=DEVICE)
    for out in (torch.zeros(32, dtype=torch.int64, device=DEVICE), torch.zeros(31, dtype=torch.int32, device=DEVICE), torch.zeros(32, dtype=torch.int32),
                torch.zeros(64, dtype=torch.int32, device=DEVICE)[::2], np.zeros(32, np.int32)):
        with pytest.raises(ValueError, match="out must be a contiguous int32 tensor"):
            pf.steps_to_go(env, out=out)
    out = torch.zeros(32, dtype=torch.int32, device=DEVICE)
    assert pf.act(env, out=out) is out and torch.equal(out, pf.steps_to_go(env))
    with pytest.raises(TypeError):
        pf.steps_to_go(object())
    with pytest.raises(ValueError, match="lle_batch_create_multi: the maps of a batch must agree"):
        pf_mod.PolicyForest([maps[0], R.SET_B.maps[0]], 4)
    with pytest.raises(ValueError, match="at most 6 agents"):
        pf_mod.PolicyForest([" ".join(f"S{k}" for k in range(7)) + " X" * 7], 4)
    freed = pf_mod.PolicyForest(maps[:2], 3, envs_per_map=8)
    freed.free()
    for call in (lambda: freed.steps_to_go(env), lambda: freed.stats(0), lambda: freed.rebuild(horizon=2)):
        with pytest.raises(RuntimeError, match="freed"):
            call()
    # the C ABI: a handle that has not been built holds no table; map_index is judged there too
    L = pf_mod.lib()
    kept = [Map(t) for t in maps[:2]]
    handles = (C.c_void_p * 2)(*[m.h for m in kept])
    h = L.lle_policyforest_create(handles, 2, None)
    assert h, L.lle_policyforest_last_error()
    two = BatchedWorld(maps[:2], 6, device=DEVICE)
    steps = torch.zeros(6, dtype=torch.int32, device=DEVICE)
    assert L.lle_policyforest_lookup(h, two.h, -1, steps.data_ptr(), None, 0, None) == -2 and b"no table" in L.lle_policyforest_last_error()
    res, args = (pf_mod.PolicyForestMapResult * 2)(), pf_mod.PolicyArgs(C.sizeof(pf_mod.PolicyArgs), 0, 3, 0)
    for horizon in (-1, 32768):
        bad = pf_mod.PolicyArgs(C.sizeof(pf_mod.PolicyArgs), 0, horizon, 0)
        assert L.lle_policyforest_build(h, C.byref(bad), res, None) == -2 and b"horizon" in L.lle_policyforest_last_error()
    assert L.lle_policyforest_build(h, C.byref(args), res, None) == 0, L.lle_policyforest_last_error()
    assert [r.n_states for r in res] == [t.n_states for t in R.tables("A", 3)[:2]]
    for index in (-2, 2):
        assert L.lle_policyforest_lookup(h, two.h, index, steps.data_ptr(), None, 0, None) == -2 and b"map_index" in L.lle_policyforest_last_error()
    assert L.lle_policyforest_lookup(h, single.h, -1, steps.data_ptr(), None, 0, None) == -2 and b"holds 1 maps" in L.lle_policyforest_last_error()
    assert L.lle_policyforest_lookup(h, two.h, 0, steps.data_ptr(), None, 0, None) == -2 and b"holds 2 maps" in L.lle_policyforest_last_error()
    assert L.lle_policyforest_lookup(h, two.h, -1, None, None, 0, None) == -1
    assert L.lle_policyforest_lookup(h, two.h, -1, None, steps.data_ptr(), 1, None) == -2 and b"action_stride" in L.lle_policyforest_last_error()
    torch.cuda.synchronize()
    assert not steps.any().item()
    assert L.lle_policyforest_lookup(h, two.h, -1, steps.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert steps.cpu().tolist() == [R.root_answer(t) for t in R.tables("A", 3)[:2] for _ in range(3)]
    L.lle_policyforest_free(h)


# ---------------------------------------------------------------------------------------------------------------- 9. the registry
def test_every_kernel_was_launched(pf_mod):
    """(last in the module.)"""
    assert sorted(pf_mod.compiled_kernels()) == sorted(pf_mod.KERNELS) == ["pf_commit", "pf_expand", "pf_insert", "pf_lookup", "pf_relax", "pf_roots", "pf_seed"]
    assert set(pf_mod.launched_kernels()) == set(pf_mod.compiled_kernels())
