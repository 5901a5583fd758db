"""The steps-to-go table on the MI355X (liblle_policy.so, lle_amd.policy.OptimalPolicy) against its restatement over the oracle
(tests/policy_ref.py): the whole table of every row, state by state -- steps, sentinels and action digits --, the same answers under
other piece sizes, the solver's lengths, expert rollouts from sampled mid-episode states, refusals and capacity.

A state of the restatement reaches the device twice: by `set_state` (positions, gems, everybody alive; `restore` from the replayed
batch where set_state derives another record than stepping does) and by replaying its prefix of joint actions from the reset state,
padded with all-STAY rows (which lead back to the same state: tests/test_policy_ref_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import policy_ref, search_ref

pytestmark = pytest.mark.gpu

ROWS = {r[0]: r for r in policy_ref.rows()}
NAMES = [r[0] for r in policy_ref.rows()]
STATE = ("pos", "bits", "gems", "beams", "avail")
SAMPLING_SEED = 3  # 1 000 one-way-detour environments after 12 sampled steps: 386 with everybody alive (one of them solved), 614 with a dead agent


@pytest.fixture(scope="module")
def policy_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import policy
    return policy


def ref_of(name):
    _, text, horizon, collect_gems = ROWS[name]
    return policy_ref.build(text, horizon, collect_gems)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(steps int32 [n_states], actions uint8 [n_states, A]) of the restatement, in the order of its states."""
    t = ref_of(name)
    answers = [t.answer(s) for s in t.states]
    return (np.array([a[0] for a in answers], np.int32), np.array([policy_ref.joint_of(a[1], t.n_agents) for a in answers], np.uint8))


_POLICIES = {}


def policy_of(policy_mod, name, **options):
    """One OptimalPolicy per (row, options) for the whole module."""
    key = (name, tuple(sorted(options.items())))
    if key not in _POLICIES:
        _, text, horizon, collect_gems = ROWS[name]
        _POLICIES[key] = policy_mod.OptimalPolicy(text, horizon, collect_gems=collect_gems, **options)
    return _POLICIES[key]


_BATCHES = {}


def replayed(name):
    """A BatchedWorld with state k of the restatement in environment k, reached by replaying its prefix."""
    import torch

    from lle_amd import BatchedWorld
    if name not in _BATCHES:
        t = ref_of(name)
        bw = BatchedWorld(t.text, t.n_states, device="cuda:0")
        longest = max(len(s.prefix) for s in t.states)
        for step in range(longest):
            rows = [list(s.prefix[step]) if step < len(s.prefix) else [policy_ref.STAY] * t.n_agents for s in t.states]
            bw.step(torch.tensor(rows, dtype=torch.uint8, device=bw.device), write_obs=False)
            assert not bw.err.any().item(), f"{name}: the step refused a replayed joint action at step {step}"
        _BATCHES[name] = bw
    return _BATCHES[name]


def by_set_state(name):
    """The same states through set_state; (batch, number of environments whose record differed from the replayed one and was restored)."""
    import torch

    from lle_amd import BatchedWorld
    t, twin = ref_of(name), replayed(name)
    bw = BatchedWorld(t.text, t.n_states, device="cuda:0")
    positions = torch.tensor([s.positions for s in t.states], dtype=torch.uint8)
    gems = torch.tensor([s.gems for s in t.states], dtype=torch.bool).view(t.n_states, -1)
    bw.set_state(positions, gems, torch.ones((t.n_states, t.n_agents), dtype=torch.bool))
    assert not bw.err.any().item(), f"{name}: set_state refused a state of the table"
    differs = torch.zeros(t.n_states, dtype=torch.bool, device=bw.device)
    for key in ("pos", "bits", "beams") + (("gems",) if t.collect_gems else ()):
        differs |= (getattr(bw, key) != getattr(twin, key)).view(t.n_states, -1).any(1)
    n = int(differs.sum().item())
    if n:
        bw.restore(twin.snapshot())
    return bw, n


def assert_lookups(pol, bw, name, where):
    want_steps, want_actions = expected(name)
    actions, steps = pol.actions(bw)
    only = pol.steps_to_go(bw)
    got_steps, got_actions = steps.cpu().numpy(), actions.cpu().numpy()
    assert got_steps.dtype == np.int32 and got_actions.dtype == np.uint8 and got_actions.shape == want_actions.shape
    bad = np.nonzero(got_steps != want_steps)[0]
    assert bad.size == 0, f"{name} {where}: steps of states {bad[:8].tolist()}: {got_steps[bad[:8]].tolist()}, restatement {want_steps[bad[:8]].tolist()}"
    bad = np.nonzero((got_actions != want_actions).any(1))[0]
    assert bad.size == 0, f"{name} {where}: actions of states {bad[:8].tolist()}: {got_actions[bad[:8]].tolist()}, restatement {want_actions[bad[:8]].tolist()}"
    assert np.array_equal(only.cpu().numpy(), want_steps)


# ---------------------------------------------------------------------------------------------------------------- the whole table
@pytest.mark.parametrize("name", NAMES)
def test_table_equals_the_restatement(policy_mod, name):
    t = ref_of(name)
    pol = policy_of(policy_mod, name)
    print(f"{name}: n_states {pol.n_states} depth {pol.depth_reached} complete {pol.complete} root {pol.root_steps} passes {pol.passes} "
          f"explore {pol.stats['explore_ms']:.1f} ms relax {pol.stats['relax_ms']:.1f} ms")
    assert (pol.n_states, pol.complete, pol.depth_reached, pol.root_steps) == (t.n_states, t.complete, t.depth_reached, t.root_steps)
    assert pol.stats["frontier"] == t.frontier and pol.stats["expanded"] == t.expanded
    assert pol.passes >= (1 if t.depth_reached else 0)
    twin = replayed(name)
    assert_lookups(pol, twin, name, "replayed")
    assert pol.steps_to_go(twin)[0].item() == (t.root_steps if t.root_steps is not None else (pol.DEAD_END if t.complete else pol.UNKNOWN))  # the reset state
    assert t.states[0].prefix == () and expected(name)[0][0] == pol.steps_to_go(twin)[0].item()
    bw, restored = by_set_state(name)
    print(f"{name}: {restored} of {t.n_states} records differed after set_state and were restored")
    assert_lookups(pol, bw, name, "set_state")
    want_steps, _ = expected(name)
    kinds = {k: int((want_steps == k).sum()) for k in (pol.UNKNOWN, pol.DEAD_END)}
    if name in ("one-way-detour-h7", "long-beam"):  # a table cut at the horizon: exact and UNKNOWN answers
        assert kinds[pol.UNKNOWN] > 0 and kinds[pol.DEAD_END] == 0 and (want_steps >= 0).any() and not pol.complete
    if name in ("single-laser-asymmetric", "gems-collect"):  # a complete table with dead ends beside exact answers
        assert kinds[pol.DEAD_END] > 0 and kinds[pol.UNKNOWN] == 0 and (want_steps >= 0).any() and pol.complete


# ---------------------------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("name", ["one-way-detour", "five-lanes"])
def test_pieces_do_not_matter(policy_mod, name):
    """chunk=64, max_states=1024: many pieces per level, a table of 2 048 slots."""
    t = ref_of(name)
    small = policy_of(policy_mod, name, chunk=64, max_states=1024)
    print(f"{name}: passes {small.passes} (defaults: {policy_of(policy_mod, name).passes})")
    assert (small.n_states, small.complete, small.depth_reached, small.root_steps) == (t.n_states, t.complete, t.depth_reached, t.root_steps)
    assert small.stats["frontier"] == t.frontier and small.stats["expanded"] == t.expanded
    assert_lookups(small, replayed(name), name, "chunk=64")
    a, s = small.actions(replayed(name))
    b, r = policy_of(policy_mod, name).actions(replayed(name))
    assert (a == b).all().item() and (s == r).all().item()


def test_one_item_per_piece(policy_mod):
    one = policy_of(policy_mod, "line", chunk=1, max_states=16)
    assert_lookups(one, replayed("line"), "line", "chunk=1")
    assert one.stats["frontier"] == ref_of("line").frontier and one.stats["expanded"] == ref_of("line").expanded


# ---------------------------------------------------------------------------------------------------------------- the solver
ROOTED = ["line", "single-laser-asymmetric", "one-way-detour", "one-way-detour-h7", "five-lanes", "long-beam", "gems-collect", "gems", "open-two-agent"]


@pytest.mark.parametrize("name", ROOTED)
def test_consistency_with_the_solver(policy_mod, name):
    """root_steps is the length of the solver's shortest plan; following `actions` from the reset state on a World is a plan of that
    length, and steps_to_go falls by exactly one per step."""
    from lle_amd import Action, Solver, World
    t = ref_of(name)
    pol = policy_of(policy_mod, name)
    solver = Solver(t.text, t.horizon)
    plan = solver.find_shortest(collect_gems=t.collect_gems)
    solver.free()
    assert t.root_steps is not None and sorted(ROOTED) == sorted(n for n in NAMES if ref_of(n).root_steps is not None)
    assert plan is not None and pol.root_steps == len(plan)
    world = World(t.text)
    world.reset()
    taken = []
    for k in range(pol.root_steps):
        actions, steps = pol.actions(world)
        assert steps.shape == (1,) and steps.item() == pol.root_steps - k
        taken.append(actions[0].cpu().tolist())
        world.step([Action(v) for v in taken[-1]])
    assert pol.steps_to_go(world).item() == 0
    search_ref.check_plan(t.text, taken, "standard", t.collect_gems, length=pol.root_steps)


# ---------------------------------------------------------------------------------------------------------------- rollouts
def test_expert_rollouts_from_sampled_states(policy_mod):
    import torch

    from lle_amd import BatchedWorld
    from oracle import oracle
    name, n = "one-way-detour", 1000
    t, pol = ref_of(name), policy_of(policy_mod, name)
    assert pol.complete
    bw = BatchedWorld(t.text, n, device="cuda:0")
    ob = oracle.OracleBatch(t.text, n)
    for step in range(12):
        bw.step(sample=True, seed=SAMPLING_SEED, t=step, write_obs=False)
        ob.step(None, auto_reset=False, seed=SAMPLING_SEED, t=step, want_obs=False)
    A = t.n_agents
    alive = (((bw.bits.unsqueeze(1) >> torch.arange(A, device=bw.device)) & 1) == 1).all(1)
    assert alive.any().item() and (~alive).any().item(), "the seed must leave environments of both kinds"
    assert np.array_equal(alive.cpu().numpy(), ob.dump()["alive"].all(1))
    table = t.table
    want = np.array([table[search_ref.identity(ob.world(e), False)][0] if ok else pol.DEAD_END for e, ok in enumerate(alive.cpu().tolist())], np.int32)
    first = pol.steps_to_go(bw)
    assert np.array_equal(first.cpu().numpy(), want)
    assert (first[alive] >= 0).all().item(), "a complete table has no UNKNOWN: every state with everybody alive was reached by the exploration"
    assert (first[~alive] == pol.DEAD_END).all().item()
    stay = torch.full((A,), policy_ref.STAY, dtype=torch.uint8, device=bw.device)
    solved_at = torch.full((n,), -1, dtype=torch.int64, device=bw.device)
    horizon = int(first.max().item())
    for k in range(horizon + 1):
        arrived = (((bw.bits.unsqueeze(1) >> (16 + torch.arange(A, device=bw.device))) & 1) == 1).all(1)
        solved_at = torch.where((solved_at < 0) & arrived & alive, torch.full_like(solved_at, k), solved_at)
        before = {key: getattr(bw, key).clone() for key in STATE}
        steps = pol.act(bw)
        for key in STATE:  # the lookup writes the action buffer and nothing else
            assert torch.equal(getattr(bw, key), before[key]), key
        assert torch.equal(steps[alive], torch.clamp(first[alive] - k, min=0))
        assert (steps[~alive] == pol.DEAD_END).all().item() and (bw.actions[~alive] == stay).all().item()
        assert (bw.actions[alive & (steps == 0)] == stay).all().item()
        bw.step(bw.actions, write_obs=False)
        assert not bw.err[alive].any().item()
        still = (((bw.bits.unsqueeze(1) >> torch.arange(A, device=bw.device)) & 1) == 1).all(1)
        assert torch.equal(still & alive, alive), "an expert action killed an agent"
    assert torch.equal(solved_at[alive], first[alive].to(torch.int64)), "every environment is solved after exactly its first steps_to_go steps"
    print(f"{int(alive.sum())} environments solved in at most {horizon} steps, {int((~alive).sum())} dead ends")


# ---------------------------------------------------------------------------------------------------------------- refusals and capacity
def test_capacity_and_neighbours(policy_mod):
    import torch

    from lle_amd import BatchedWorld, Map
    text = ROWS["one-way-detour"][1]
    bw = BatchedWorld(text, 64, device="cuda:0")
    bw.step(sample=True, seed=5, t=0)
    for _ in range(2):  # nothing is cached: the second constructor fails the same way
        with pytest.raises(policy_mod.PolicyCapacityError, match="max_states"):
            policy_mod.OptimalPolicy(text, 40, max_states=64)
    pol = policy_mod.OptimalPolicy(text, 40, chunk=512, max_states=4096)  # a second build beside the stepped batch
    bw.step(sample=True, seed=5, t=1)
    after = bw.host_buffers()
    twin = BatchedWorld(text, 64, device="cuda:0")
    twin.step(sample=True, seed=5, t=0)
    twin.step(sample=True, seed=5, t=1)
    want = twin.host_buffers()
    for key in STATE:
        assert torch.equal(torch.as_tensor(after[key]), torch.as_tensor(want[key])), key
    assert_lookups(pol, replayed("one-way-detour"), "one-way-detour", "chunk=512")
    pol.free()
    # the C ABI: a handle whose build overflowed holds no table, and says so at every lookup
    L, m = policy_mod.lib(), Map(text)
    opt = policy_mod.PolicyOptions(C.sizeof(policy_mod.PolicyOptions), -1, 0, 64, None)
    h = L.lle_policy_create(m.h, C.byref(opt))
    assert h
    steps = torch.zeros(64, dtype=torch.int32, device=bw.device)
    assert L.lle_policy_lookup(h, bw.h, steps.data_ptr(), None, 0, None) == -2 and b"no table" in L.lle_policy_last_error()  # never built
    res = policy_mod.PolicyResult(C.sizeof(policy_mod.PolicyResult))
    for horizon in (-1, 32768):
        args = policy_mod.PolicyArgs(C.sizeof(policy_mod.PolicyArgs), 0, horizon, 0)
        assert L.lle_policy_build(h, C.byref(args), C.byref(res)) == -2 and b"horizon" in L.lle_policy_last_error()
    bad = policy_mod.PolicyArgs(4, 0, 40, 0)
    assert L.lle_policy_build(h, C.byref(bad), C.byref(res)) == -2 and b"struct_bytes" in L.lle_policy_last_error()
    args = policy_mod.PolicyArgs(C.sizeof(policy_mod.PolicyArgs), 0, 40, 0)
    assert L.lle_policy_build(h, C.byref(args), C.byref(res)) == policy_mod.LLE_POLICY_CAPACITY and b"max_states = 64" in L.lle_policy_last_error()
    assert L.lle_policy_lookup(h, bw.h, steps.data_ptr(), None, 0, None) == -2 and b"no table" in L.lle_policy_last_error()
    torch.cuda.synchronize()
    assert not steps.any().item()
    L.lle_policy_free(h)


def test_refusals(policy_mod):
    import torch

    from lle_amd import BatchedWorld
    text = ROWS["open-two-agent"][1]
    pol = policy_of(policy_mod, "open-two-agent")
    other = BatchedWorld(ROWS["exit-freezes"][1], 5, device="cuda:0")  # two agents, no source, other dimensions
    with pytest.raises(ValueError, match="fingerprint"):
        pol.steps_to_go(other)
    steps = pol.steps_to_go(other, check_map=False)  # the caller vouches for the map: the call runs (and finds states it does not know)
    assert steps.shape == (5,) and steps.dtype == torch.int32
    with pytest.raises(ValueError, match="beam words"):  # ... but not over records of another layout
        pol.steps_to_go(BatchedWorld(ROWS["single-laser-asymmetric"][1], 5, device="cuda:0"), check_map=False)
    with pytest.raises(ValueError, match="agents"):
        pol.steps_to_go(BatchedWorld("S0 . X", 5, device="cuda:0"), check_map=False)
    with pytest.raises(ValueError, match="maps"):
        pol.steps_to_go(BatchedWorld([text, text], 4, device="cuda:0"))
    sourced = BatchedWorld(ROWS["single-laser-asymmetric"][1], 4, device="cuda:0")
    lasers = policy_of(policy_mod, "single-laser-asymmetric")
    assert lasers.steps_to_go(sourced).shape == (4,)
    sourced.set_sources(enabled=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="per-environment sources"):
        lasers.steps_to_go(sourced)
    with pytest.raises(ValueError, match="at most 6 agents"):
        policy_mod.OptimalPolicy(" ".join(f"S{k}" for k in range(7)) + " X" * 7, 4)
    with pytest.raises(TypeError):
        pol.steps_to_go(object())
    none = policy_mod.OptimalPolicy("S0 . X", 0)  # a horizon of no levels: the reset state alone, and nothing known about it
    assert (none.n_states, none.depth_reached, none.complete, none.passes, none.root_steps) == (1, 0, False, 0, None)
    assert none.stats["frontier"] == [1] and none.stats["expanded"] == []
    assert none.steps_to_go(BatchedWorld("S0 . X", 3, device="cuda:0")).cpu().tolist() == [none.UNKNOWN] * 3
    arrived = policy_mod.OptimalPolicy("S0 X", 3)
    assert arrived.root_steps == 1 and arrived.complete


def test_every_kernel_was_launched(policy_mod):
    """(last in the module.)"""
    assert sorted(policy_mod.compiled_kernels()) == ["policy_commit", "policy_expand", "policy_insert", "policy_lookup", "policy_relax"]
    assert set(policy_mod.launched_kernels()) == set(policy_mod.compiled_kernels())
