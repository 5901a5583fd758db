"""The four search libraries on the MI355X (liblle_search.so, liblle_forest.so, liblle_policy.so, liblle_helpgraph.so) over the parts of
their written contract that the suites of the features do not execute, against the same three restatements over the oracle
(tests/search_ref.py, policy_ref.py, helpgraph_ref.py), exactly -- lengths, per-depth counters, state counts, steps and action digits;
every plan is replayed on the oracle.  tests/test_search_edges_cpu.py holds the restatements to every number used here.

  A  six agents outside the help-graph library: three position words, the second availability word, 15 625 joint codes
  B  a pool that is exactly full, one record short, one record spare (tables of 32 to 128 slots: linear probing wraps)
  C  a handle that goes on after LLE_*_CAPACITY, and one lle_policy handle built five times
  D  the `stream` and `device` options of the four option structs and the stream of lle_policy_lookup
  E  lookups on batches as a training loop has them, and the fields that are not part of a state's identity
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import forest_ref, helpgraph_ref, policy_ref, search_ref
from tests import search_edges_inputs as inp

pytestmark = pytest.mark.gpu

U, D, STAY = policy_ref.UNKNOWN, policy_ref.DEAD_END, policy_ref.STAY
MODES = ("standard", "no-cooperation")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def values(plan):
    return None if plan is None else [[a.value for a in row] for row in plan]


# ---------------------------------------------------------------------------------------------------------------- comparisons
def assert_search(s, text, mode="standard"):
    """One mode of the Solver `s` against search_ref: length, counters, state count, the plan replayed."""
    ref = search_ref.search(text, s.t_max, mode)
    plan = values(s.find_shortest(mode))
    stats = s.last_stats
    print(f"{mode}: length {stats['length']} (ref {ref.length}), frontier {stats['frontier']}, expanded {stats['expanded']}")
    assert stats["length"] == ref.length and (plan is None) == (ref.length is None)
    assert stats["frontier"] == ref.frontier and stats["expanded"] == ref.expanded and stats["n_states"] == ref.n_states
    if plan is not None:
        search_ref.check_plan(text, plan, mode, length=ref.length)
    return stats


def mode_text(mode, param=2):
    return f"{mode}-{param}" if mode in ("no-convergence", "no-divergence") else mode


def assert_helpgraph(s, text, mode="standard", param=2):
    """One mode of the HelpGraphSolver `s` against helpgraph_ref."""
    ref = helpgraph_ref.search(text, s.t_max, mode, param)
    plan = values(s.find_shortest(mode_text(mode, param)))
    stats = s.last_stats
    print(f"{mode}-{param}: length {stats['length']} (ref {ref.length}), frontier {stats['frontier']}, expanded {stats['expanded']}")
    assert stats["length"] == ref.length and (plan is None) == (ref.length is None)
    assert stats["frontier"] == ref.frontier and stats["expanded"] == ref.expanded and stats["n_states"] == ref.n_states
    if plan is None:
        assert stats["help_edges"] is None
    else:
        assert stats["help_edges"] == helpgraph_ref.check_plan(text, plan, mode, param, length=ref.length)
    return stats


def expected(t):
    """(steps int32 [n_states], actions uint8 [n_states, A]) of the restatement's Table, in the order of its states."""
    answers = [t.answer(s) for s in t.states]
    return np.array([a[0] for a in answers], np.int32), np.array([policy_ref.joint_of(a[1], t.n_agents) for a in answers], np.uint8)


def replayed(torch, t, device="cuda:0"):
    """A BatchedWorld with state k of the Table `t` in environment k, reached by replaying its prefix padded with all-STAY rows."""
    from lle_amd import BatchedWorld
    bw = BatchedWorld(t.text, t.n_states, device=device)
    for step in range(max(len(s.prefix) for s in t.states)):
        rows = [list(s.prefix[step]) if step < len(s.prefix) else [STAY] * t.n_agents for s in t.states]
        bw.step(torch.tensor(rows, dtype=torch.uint8, device=bw.device), write_obs=False)
        assert not bw.err.any().item(), f"the step refused a replayed joint action at step {step}"
    return bw


def assert_answers(got_steps, got_actions, want_steps, want_actions, where):
    got_steps, got_actions = got_steps.cpu().numpy(), got_actions.cpu().numpy()
    assert got_steps.dtype == np.int32 and got_actions.dtype == np.uint8 and got_actions.shape == want_actions.shape
    bad = np.nonzero(got_steps != want_steps)[0]
    assert bad.size == 0, f"{where}: steps of states {bad[:8].tolist()}: {got_steps[bad[:8]].tolist()}, restatement {want_steps[bad[:8]].tolist()}"
    bad = np.nonzero((got_actions != want_actions).any(1))[0]
    assert bad.size == 0, f"{where}: actions of states {bad[:8].tolist()}: {got_actions[bad[:8]].tolist()}, restatement {want_actions[bad[:8]].tolist()}"


def assert_policy(pol, t, bw, where):
    """An OptimalPolicy against the restatement's Table: the build's numbers and the whole table over the replayed batch `bw`."""
    assert (pol.n_states, pol.complete, pol.depth_reached, pol.root_steps) == (t.n_states, t.complete, t.depth_reached, t.root_steps), where
    assert pol.stats["frontier"] == t.frontier and pol.stats["expanded"] == t.expanded, where
    actions, steps = pol.actions(bw)
    assert_answers(steps, actions, *expected(t), where)
    assert np.array_equal(pol.steps_to_go(bw).cpu().numpy(), expected(t)[0])


class CPolicy:
    """An lle_policy handle through the C ABI alone (OptimalPolicy builds once, in its constructor, on the NULL stream)."""

    def __init__(self, text, *, device=-1, chunk=0, max_states=0, stream=None):
        from lle_amd import Map, policy
        self.pm, self.L, self.map = policy, policy.lib(), Map(text)
        opt = policy.PolicyOptions(C.sizeof(policy.PolicyOptions), device, chunk, max_states, stream)
        self.h = self.L.lle_policy_create(self.map.h, C.byref(opt))
        self.A = self.map.n_agents

    def build(self, horizon, collect_gems=False):
        """(return code, lle_policy_result, frontier, expanded)"""
        args = self.pm.PolicyArgs(C.sizeof(self.pm.PolicyArgs), int(collect_gems), horizon, 0)
        res = self.pm.PolicyResult(C.sizeof(self.pm.PolicyResult))
        rc = self.L.lle_policy_build(self.h, C.byref(args), C.byref(res))
        cap = res.depth_reached + 2
        frontier, expanded = (C.c_int64 * cap)(), (C.c_int64 * cap)()
        n = self.L.lle_policy_stats(self.h, frontier, expanded, cap)
        return rc, res, [int(frontier[d]) for d in range(n)], [int(expanded[d]) for d in range(res.depth_reached)]

    def assert_built(self, t, horizon, collect_gems=False):
        rc, res, frontier, expanded = self.build(horizon, collect_gems)
        assert rc == 0, self.L.lle_policy_last_error()
        root = res.root_steps if res.root_steps >= 0 else None
        assert (res.n_states, bool(res.complete), res.depth_reached, root) == (t.n_states, t.complete, t.depth_reached, t.root_steps)
        assert frontier == t.frontier and expanded == t.expanded and res.step_errors == 0

    def lookup(self, torch, bw, stream=None):
        """(return code, steps, actions); on the batch's current torch stream unless `stream` is given."""
        steps = torch.full((bw.n_envs,), -77, dtype=torch.int32, device=bw.device)
        actions = torch.full((bw.n_envs, self.A), 77, dtype=torch.uint8, device=bw.device)
        rc = self.L.lle_policy_lookup(self.h, bw.h, steps.data_ptr(), actions.data_ptr(), self.A, bw._stream() if stream is None else stream)
        return rc, steps, actions

    def free(self):
        if self.h:
            self.L.lle_policy_free(self.h)
            self.h = None


# ================================================================================================ A. six agents
@pytest.mark.parametrize("options", [{}, dict(chunk=4096)], ids=["defaults", "chunk4096"])
def test_six_agents_solver(torch, options):
    """Three position words, two availability words and 15 625 codes per state in the u16 action of a stored state; with chunk=4096 a
    state's codes span four pieces, so a piece boundary falls inside the digits of agent 5."""
    from lle_amd import Map, Solver
    assert Map(inp.SIX).n_agents == 6 == Map(inp.LANES6).n_agents
    s = Solver(inp.SIX, 4, **options)
    try:
        std = assert_search(s, inp.SIX, "standard")
        alone = assert_search(s, inp.SIX, "no-cooperation")
        assert (std["length"], std["frontier"], alone["length"], alone["n_states"]) == (2, [1, 47, 436], None, 840)
    finally:
        s.free()
    lanes = Solver(inp.LANES6, 4, **options)
    try:
        assert assert_search(lanes, inp.LANES6) == dict(frontier=[1, 63], expanded=[64], n_states=64, length=1)
    finally:
        lanes.free()


@pytest.mark.parametrize("mode", MODES)
def test_six_agents_forest(torch, mode):
    """Two six-agent maps of one shape with different answers, 16 384 environments each: level 1 is 45 pieces per map."""
    from lle_amd import ForestSolver
    maps, E = [inp.SIX, inp.SIX_VARIANT], 16384
    refs = forest_ref.oracle(maps, 2, mode)
    f = ForestSolver(maps, 2, envs_per_map=E)
    try:
        res = f.run(mode)
        print(f"{mode}: lengths {res.length.tolist()}, states {res.n_states.tolist()}, pieces {res.pieces}, occupancy {res.valid_items}/{res.launched_lanes}")
        for m, (text, ref) in enumerate(zip(maps, refs)):
            forest_ref.assert_map_equals_oracle(text, ref, res, m, mode)
        want_pieces = sum(max(-(-r.frontier[d] * 5 ** 6 // E) for r in refs) for d in range(2))
        assert res.pieces == want_pieces and res.pieces >= 30
        assert res.valid_items == 5 ** 6 * sum(r.frontier[0] + r.frontier[1] for r in refs)
    finally:
        f.free()


def test_six_agents_table(torch):
    """The whole table of OptimalPolicy(SIX, 12), state by state over replayed states: steps, sentinels and all six action digits --
    the codes reach 15 624 in the 16-bit code field of a value, stay_code(6) included."""
    from lle_amd import OptimalPolicy
    t = policy_ref.build(inp.SIX, 12, False)
    t0 = time.perf_counter()
    pol = OptimalPolicy(inp.SIX, 12)
    print(f"OptimalPolicy(SIX, 12): {time.perf_counter() - t0:.2f} s, passes {pol.passes}, explore {pol.stats['explore_ms']:.0f} ms, relax {pol.stats['relax_ms']:.0f} ms")
    try:
        bw = replayed(torch, t)
        assert_policy(pol, t, bw, "SIX horizon 12")
        want_steps, want_actions = expected(t)
        assert (want_steps == D).sum() == 676 and sorted(set(want_steps[want_steps >= 0].tolist())) == [0, 1, 2, 3, 4] and not (want_steps == U).any()
        assert (want_actions[:, 4] != STAY).any() and (want_actions[:, 5] != STAY).any()
    finally:
        pol.free()


def test_six_agents_table_cut_at_the_horizon(torch):
    """Horizon 4: 1 344 states, incomplete; UNKNOWN exactly where the restatement says, exact answers elsewhere."""
    from lle_amd import OptimalPolicy
    t = policy_ref.build(inp.SIX, 4, False)
    pol = OptimalPolicy(inp.SIX, 4)
    try:
        assert_policy(pol, t, replayed(torch, t), "SIX horizon 4")
        want_steps, _ = expected(t)
        assert (want_steps == U).any() and (want_steps >= 0).any() and not (want_steps == D).any() and not pol.complete
    finally:
        pol.free()


# ================================================================================================ B. exact fit
def no_partial_answer(L, prefix, h):
    """After a capacity failure the handle holds no plan and no counters beyond the reset state."""
    buf = (C.c_uint8 * 64)()
    frontier, expanded = (C.c_int64 * 8)(), (C.c_int64 * 8)()
    assert getattr(L, prefix + "_plan")(h, buf, 64) == -2 and b"no plan" in getattr(L, prefix + "_last_error")()
    assert getattr(L, prefix + "_stats")(h, frontier, expanded, 8) == 1 and frontier[0] == 1


@pytest.mark.parametrize("chunk", [1, 64])
@pytest.mark.parametrize("mode", MODES)
def test_exact_fit_search(torch, mode, chunk):
    """max_states = the states the search stores: the last winner takes the last record (`idx >= max_states` is false for it and
    `counters[CNT_STATES] > max_states` too), in a table of 32 (chunk 1) or 128 slots."""
    from lle_amd import Solver, SolverCapacityError, solver
    text = inp.text(inp.EXACT_MAP)
    n = search_ref.search(text, inp.EXACT_T_MAX, mode).n_states
    assert n == {"standard": 11, "no-cooperation": 10}[mode]
    for cap in (n, n + 1):
        s = Solver(text, inp.EXACT_T_MAX, chunk=chunk, max_states=cap)
        try:
            assert assert_search(s, text, mode)["n_states"] == n
        finally:
            s.free()
    short = Solver(text, inp.EXACT_T_MAX, chunk=chunk, max_states=n - 1)
    try:
        for _ in range(2):
            with pytest.raises(SolverCapacityError, match=f"max_states = {n - 1}"):
                short.find_shortest(mode)
            assert short._cache == {}
            no_partial_answer(solver.lib(), "lle_search", short.h)
    finally:
        short.free()


@pytest.mark.parametrize("chunk", [1, 64])
def test_exact_fit_helpgraph(torch, chunk):
    """14 records at t_max 6 where the plain search stores 11 states: the help words are part of the identity."""
    from lle_amd import HelpGraphSolver, SolverCapacityError, helpgraph
    text = inp.text(inp.EXACT_MAP)
    n = helpgraph_ref.search(text, inp.EXACT_T_MAX).n_states
    assert n == 14
    for cap in (n, n + 1):
        s = HelpGraphSolver(text, inp.EXACT_T_MAX, chunk=chunk, max_states=cap)
        try:
            assert assert_helpgraph(s, text)["n_states"] == n
        finally:
            s.free()
    short = HelpGraphSolver(text, inp.EXACT_T_MAX, chunk=chunk, max_states=n - 1)
    try:
        for _ in range(2):
            with pytest.raises(SolverCapacityError, match=f"max_states = {n - 1}"):
                short.find_shortest("standard")
            assert short._cache == {}
            no_partial_answer(helpgraph.lib(), "lle_helpgraph", short.h)
    finally:
        short.free()


@pytest.mark.parametrize("chunk", [1, 64])
def test_exact_fit_policy(torch, chunk):
    """A complete table of 16 states in a pool of 16, 17 and 15 records."""
    from lle_amd import OptimalPolicy, PolicyCapacityError
    text = inp.text(inp.EXACT_MAP)
    t = policy_ref.build(text, inp.EXACT_HORIZON, False)
    n = t.n_states
    assert n == 16
    bw = replayed(torch, t)
    for cap in (n, n + 1):
        pol = OptimalPolicy(text, inp.EXACT_HORIZON, chunk=chunk, max_states=cap)
        try:
            assert_policy(pol, t, bw, f"max_states {cap}")
        finally:
            pol.free()
    for _ in range(2):
        with pytest.raises(PolicyCapacityError, match=f"max_states = {n - 1}"):
            OptimalPolicy(text, inp.EXACT_HORIZON, chunk=chunk, max_states=n - 1)
    # ... and through the C ABI: the handle that failed holds no table, twice
    c = CPolicy(text, chunk=chunk, max_states=n - 1)
    try:
        for _ in range(2):
            rc, res, frontier, expanded = c.build(inp.EXACT_HORIZON)
            assert rc == c.pm.LLE_POLICY_CAPACITY and (frontier, res.n_states) == ([1], n - 1)
            rc, steps, _ = c.lookup(torch, bw)
            assert rc == -2 and b"no table" in c.L.lle_policy_last_error()
            torch.cuda.synchronize()
            assert (steps == -77).all().item(), "a refused lookup writes nothing"
    finally:
        c.free()


# ================================================================================================ C. a handle that goes on
def test_search_handle_goes_on_after_capacity(torch):
    """After LLE_SEARCH_CAPACITY the pool is full and the table holds the tags of the piece that failed; the next run on the SAME handle
    starts from an empty table and its own counters."""
    from lle_amd import Solver, SolverCapacityError
    text = inp.text(inp.CAPACITY_MAP)
    s = Solver(text, inp.CAPACITY_T_MAX, max_states=inp.SEARCH_POOL)
    try:
        for _ in range(2):
            with pytest.raises(SolverCapacityError, match="max_states = 128"):
                s.find_shortest()
            h = s.h
            stats = assert_search(s, text, "no-cooperation")
            assert s.h == h and (stats["n_states"], stats["length"]) == (55, None)
            s._cache.clear()  # (ask the device again, not the Python cache)
        with pytest.raises(SolverCapacityError):
            s.find_shortest("standard")
    finally:
        s.free()


def test_helpgraph_handle_goes_on_after_capacity(torch):
    from lle_amd import HelpGraphSolver, SolverCapacityError
    text = inp.text(inp.CAPACITY_MAP)
    s = HelpGraphSolver(text, inp.CAPACITY_T_MAX, max_states=inp.HELPGRAPH_POOL)
    try:
        for _ in range(2):
            with pytest.raises(SolverCapacityError, match="max_states = 256"):
                s.find_shortest(mode_text(*inp.HELPGRAPH_OVER))
            h = s.h
            stats = assert_helpgraph(s, text, *inp.HELPGRAPH_FITS)
            assert s.h == h and (stats["n_states"], stats["length"]) == (245, None)
            s._cache.clear()
        with pytest.raises(SolverCapacityError):
            s.find_shortest(mode_text(*inp.HELPGRAPH_OVER))
    finally:
        s.free()


def test_one_policy_handle_built_again(torch):
    """One lle_policy handle, five builds (inp.REBUILDS): another horizon, the gem word in and out of the identity, a smaller table
    after a larger one.  After each build lle_policy_stats is that configuration's frontier and a lookup over ONE batch -- the 44
    states of the collect_gems table, replayed -- answers what that configuration's restatement holds for each state's identity,
    UNKNOWN where it holds none.  (The build also drops the handle's cache of callers' batches: the same batch is bound again.)"""
    big = policy_ref.build(inp.GEMS, 12, True)
    bw = replayed(torch, big)
    stay = policy_ref.code_of([STAY])
    c = CPolicy(inp.GEMS)
    assert c.h, c.L.lle_policy_last_error()
    seen = []
    try:
        for horizon, collect in inp.REBUILDS:
            t = policy_ref.build(inp.GEMS, horizon, collect)
            c.assert_built(t, horizon, collect)
            table = t.table
            answers = [table.get(s.key if collect else s.key[:-1], (U, stay))[:2] for s in big.states]
            want_steps = np.array([a[0] for a in answers], np.int32)
            want_actions = np.array([policy_ref.joint_of(a[1], 1) for a in answers], np.uint8)
            rc, steps, actions = c.lookup(torch, bw)
            assert rc == 0, c.L.lle_policy_last_error()
            assert_answers(steps, actions, want_steps, want_actions, f"horizon {horizon} collect_gems {collect}")
            seen.append(want_steps.tolist())
        assert seen[0] == seen[1] == seen[4] and seen[2] != seen[1] and U in seen[3] and U not in seen[2]
    finally:
        c.free()


# ================================================================================================ D. streams and devices
def with_handle(solver_obj, create, map_handles, options):
    """Put a handle made through ctypes with `options` into a Solver-like object, whose own would be made with stream = NULL."""
    solver_obj.h = create(*map_handles, C.byref(options))
    assert solver_obj.h
    return solver_obj


def four_libraries(torch, device, stream):
    """One small search through each of the four libraries on handles created with `device` and `stream`; everything equals the
    restatements.  The current device of the caller is the same after every call."""
    from lle_amd import ForestSolver, HelpGraphSolver, Solver, forest, helpgraph, solver
    text = inp.text("one-way-detour")
    current = torch.cuda.current_device()
    s = Solver(text, 11)
    with_handle(s, solver.lib().lle_search_create, (s._map.h,), solver.SearchOptions(C.sizeof(solver.SearchOptions), device, s.chunk, s.max_states, stream))
    try:
        for mode in MODES:
            assert_search(s, text, mode)
            assert torch.cuda.current_device() == current
    finally:
        s.free()
    g = HelpGraphSolver(text, 7)
    with_handle(g, helpgraph.lib().lle_helpgraph_create, (g._map.h,), helpgraph.HelpGraphOptions(C.sizeof(helpgraph.HelpGraphOptions), device, g.chunk, g.max_states, stream))
    try:
        assert assert_helpgraph(g, text)["length"] == 6
        assert torch.cuda.current_device() == current
    finally:
        g.free()
    maps = list(forest_ref.SET_A.maps[:4])
    f = ForestSolver(maps, forest_ref.SET_A.t_max)
    handles = (C.c_void_p * len(maps))(*[m.h for m in f._maps])
    with_handle(f, forest.lib().lle_forest_create, (handles, len(maps)), forest.ForestOptions(C.sizeof(forest.ForestOptions), device, f.envs_per_map, f.max_states_per_map, stream))
    try:
        for mode in MODES:
            res = f.run(mode)
            for m, ref in enumerate(forest_ref.oracle(maps, forest_ref.SET_A.t_max, mode)):
                forest_ref.assert_map_equals_oracle(maps[m], ref, res, m, mode)
            assert torch.cuda.current_device() == current
    finally:
        f.free()
    t = policy_ref.build(text, 40, False)
    c = CPolicy(text, device=device, stream=stream)
    assert c.h, c.L.lle_policy_last_error()
    try:
        c.assert_built(t, 40)
        assert torch.cuda.current_device() == current
        if device <= 0:  # (a batch on another device: the caller's to make)
            rc, steps, actions = c.lookup(torch, replayed(torch, t))
            assert rc == 0, c.L.lle_policy_last_error()
            assert_answers(steps, actions, *expected(t), f"device {device}")
            assert torch.cuda.current_device() == current
    finally:
        c.free()


def test_handles_on_a_stream_of_their_own(torch):
    """Every option struct carries a `stream`; here it is a torch.cuda.Stream instead of NULL, once per library.  A test like this
    cannot prove that every enqueue of a library uses the handle's stream -- a misplaced launch on the NULL stream is still ordered
    against the blocking streams torch makes --; it executes the contract once and checks the results."""
    stream = torch.cuda.Stream()
    four_libraries(torch, -1, stream.cuda_stream)
    stream.synchronize()


def test_lookup_on_a_second_stream(torch):
    """The table is built on one stream; the batch is created and stepped, and the lookups are launched, on another.  The answers equal
    those of the same steps and lookups on the default stream.  (Executes the contract once: see the test above.)"""
    from lle_amd import BatchedWorld
    text = inp.text("one-way-detour")
    lived = inp.lived_in(text, 40)
    build_stream, other = torch.cuda.Stream(), torch.cuda.Stream()
    c = CPolicy(text, stream=build_stream.cuda_stream)
    assert c.h, c.L.lle_policy_last_error()
    try:
        c.assert_built(policy_ref.build(text, 40, False), 40)
        default = BatchedWorld(text, inp.LIVED_ENVS, device="cuda:0")
        got_default = []
        for t in range(8):
            default.step(sample=True, auto_reset=True, seed=inp.LIVED_SEED, t=t)
            rc, steps, actions = c.lookup(torch, default)
            assert rc == 0
            got_default.append((steps.cpu(), actions.cpu()))
        with torch.cuda.stream(other):
            bw = BatchedWorld(text, inp.LIVED_ENVS, device="cuda:0")
            assert bw._stream().value == other.cuda_stream
            for t in range(8):
                bw.step(sample=True, auto_reset=True, seed=inp.LIVED_SEED, t=t)
                rc, steps, actions = c.lookup(torch, bw, other.cuda_stream)
                assert rc == 0, c.L.lle_policy_last_error()
                steps, actions = steps.cpu(), actions.cpu()  # (on `other`: behind the lookup)
                assert torch.equal(steps, got_default[t][0]) and torch.equal(actions, got_default[t][1]), t
                assert np.array_equal(steps.numpy(), lived.want[t]), t
        other.synchronize()
    finally:
        c.free()


def test_device_option(torch):
    """device = 0 gives what -1 gives; device = the number of devices is refused by all four libraries; the caller's device stays."""
    from lle_amd import Map, forest, helpgraph, policy, solver
    four_libraries(torch, 0, None)
    n, current = torch.cuda.device_count(), torch.cuda.current_device()
    map_ = Map(inp.text("one-way-detour"))
    one = (C.c_void_p * 1)(map_.h)
    for lib, create, args, options in (
            (solver.lib(), "lle_search_create", (map_.h,), solver.SearchOptions(C.sizeof(solver.SearchOptions), n, 0, 0, None)),
            (helpgraph.lib(), "lle_helpgraph_create", (map_.h,), helpgraph.HelpGraphOptions(C.sizeof(helpgraph.HelpGraphOptions), n, 0, 0, None)),
            (forest.lib(), "lle_forest_create", (one, 1), forest.ForestOptions(C.sizeof(forest.ForestOptions), n, 0, 0, None)),
            (policy.lib(), "lle_policy_create", (map_.h,), policy.PolicyOptions(C.sizeof(policy.PolicyOptions), n, 0, 0, None))):
        assert not getattr(lib, create)(*args, C.byref(options)), create
        assert b"no such HIP device" in getattr(lib, create.replace("_create", "_last_error"))(), create
        assert torch.cuda.current_device() == current


def test_handles_on_the_second_device(torch):
    """Handles on device 1 while device 0 is current: equal results, device 0 still current, and a lookup of a batch that lives on
    device 0 is refused."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two HIP devices")
    from lle_amd import BatchedWorld
    torch.cuda.set_device(0)
    four_libraries(torch, 1, None)
    assert torch.cuda.current_device() == 0
    text = inp.text("one-way-detour")
    t = policy_ref.build(text, 40, False)
    c = CPolicy(text, device=1)
    assert c.h, c.L.lle_policy_last_error()
    try:
        c.assert_built(t, 40)
        here = BatchedWorld(text, 8, device="cuda:0")
        rc, steps, _ = c.lookup(torch, here)
        assert rc == -2 and b"lives on HIP device 0" in c.L.lle_policy_last_error()
        assert (steps == -77).all().item() and torch.cuda.current_device() == 0
        with torch.cuda.device(1):
            there = replayed(torch, t, "cuda:1")
        rc, steps, actions = c.lookup(torch, there)  # (device 0 is current again: the DeviceGuard of the lookup)
        assert rc == 0, c.L.lle_policy_last_error()
        torch.cuda.synchronize(1)
        assert_answers(steps, actions, *expected(t), "device 1")
        assert torch.cuda.current_device() == 0
    finally:
        c.free()


# ================================================================================================ E. lived-in batches
_POLICIES = {}


def policy_of(text, horizon, collect_gems=False):
    from lle_amd import OptimalPolicy
    key = (text, horizon, collect_gems)
    if key not in _POLICIES:
        _POLICIES[key] = OptimalPolicy(text, horizon, collect_gems=collect_gems)
    return _POLICIES[key]


def assert_steps(pol, env, want, where):
    got = pol.steps_to_go(env).cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{where}: environments {bad[:8].tolist()}: {got[bad[:8]].tolist()}, expected {want[bad[:8]].tolist()}"


@pytest.mark.parametrize("row_align", [None, 128])
@pytest.mark.parametrize("name", sorted(inp.LIVED))
def test_lookups_while_a_batch_lives(torch, name, row_align):
    """1 000 environments (a ragged last workgroup), 30 sampled steps with auto-reset and observations written, a lookup after every
    step: table[identity] where everybody is alive, DEAD_END elsewhere, from the OracleBatch that mirrors the batch.  Solved, dead and
    freshly reset environments all occur (tests/test_search_edges_cpu.py); a masked reset at the end answers root_steps."""
    from lle_amd import BatchedWorld
    text, horizon = inp.text(name), inp.LIVED[name]
    lived, pol = inp.lived_in(text, horizon), policy_of(text, horizon)
    assert pol.complete and pol.root_steps == lived.root_steps
    bw = BatchedWorld(text, inp.LIVED_ENVS, device="cuda:0", row_align=row_align)
    if row_align:
        assert bw.map.obs_stride % row_align == 0
    assert_steps(pol, bw, np.full(inp.LIVED_ENVS, lived.root_steps, np.int32), "the reset state")
    for t in range(inp.LIVED_STEPS):
        bw.step(sample=True, auto_reset=True, seed=inp.LIVED_SEED, t=t)
        assert np.array_equal(bw.actions.cpu().numpy(), lived.actions[t]), f"the batch and the oracle sampled other actions at step {t}"
        assert np.array_equal((bw.evcount.cpu().numpy() & 128) != 0, lived.was_reset[t])
        assert_steps(pol, bw, lived.want[t], f"step {t}")
    mask = torch.arange(inp.LIVED_ENVS) % 3 == 0
    bw.reset(mask)
    want = np.where(mask.numpy(), lived.root_steps, lived.want[-1]).astype(np.int32)
    assert (want != lived.want[-1]).any()
    assert_steps(pol, bw, want, "after a masked reset")


@pytest.mark.parametrize("name", sorted(inp.LIVED))
def test_lookups_between_rollout_chunks(torch, name):
    """The same 30 steps through rollout() in fused chunks of 7, 11 and 12 steps, a lookup after every chunk."""
    from lle_amd import BatchedWorld
    text, horizon = inp.text(name), inp.LIVED[name]
    lived, pol = inp.lived_in(text, horizon), policy_of(text, horizon)
    bw = BatchedWorld(text, inp.LIVED_ENVS, device="cuda:0")
    t = 0
    for chunk in inp.ROLLOUT_CHUNKS:
        bw.rollout(chunk, auto_reset=True, seed=inp.LIVED_SEED, t=t)
        t += chunk
        want = lived.want[t - 1]
        assert (want == 0).any() or (want == D).any()
        assert_steps(pol, bw, want, f"after {t} fused steps")
    assert t == inp.LIVED_STEPS


@pytest.mark.parametrize("name", sorted(inp.LIVED))
def test_lookups_on_a_batched_lle(torch, name):
    """_batched() accepts a BatchedLLE: stepped through LLE.step with the oracle's joint actions and auto-reset, steps_to_go(env) is
    steps_to_go(env.world) and the expected value."""
    from lle_amd.env import BatchedLLE
    text, horizon = inp.text(name), inp.LIVED[name]
    lived, pol = inp.lived_in(text, horizon), policy_of(text, horizon)
    env = BatchedLLE(text, inp.LIVED_ENVS, device="cuda:0")
    for t in range(inp.LIVED_STEPS):
        out = env.step(torch.from_numpy(lived.actions[t]), auto_reset=True)
        assert not out["err"].any().item()
        assert_steps(pol, env, lived.want[t], f"BatchedLLE step {t}")
        assert torch.equal(pol.steps_to_go(env), pol.steps_to_go(env.world))
    a, s = pol.actions(env)
    b, r = pol.actions(env.world)
    assert torch.equal(a, b) and torch.equal(s, r)


def raw_rows(torch, bw, name):
    """(the bytes of buffer `name` of the batch as one flat uint8 view, bytes per environment row)"""
    offset, nbytes, _shape, elem_bytes, stride = bw._desc[name]
    return bw._base[offset:offset + nbytes], stride[0] * elem_bytes


def fill_padding(torch, bw, name, used):
    """0xFF into every byte of the rows of `name` past the first `used` bytes; returns the number of bytes written."""
    raw, row = raw_rows(torch, bw, name)
    pad = (torch.arange(raw.numel(), device=raw.device) % row) >= used
    raw[pad] = 0xFF
    return int(pad.sum().item())


def test_fields_outside_the_identity_change_nothing(torch):
    """Three agents: a position row of 8 bytes for 6, an availability row of 4 for 3.  After 12 sampled steps the lookups equal the
    expectation; then the availability bytes are filled with random bytes, the padding of the position and availability rows with
    0xFF and the gem word with random bits: every answer and every action is unchanged (collect_gems is off: n_key ends before the gem
    word, and env_word never reads past 2 A position bytes).  pol.act writes the first A bytes of each action row and no other."""
    from lle_amd import BatchedWorld
    text = inp.text(inp.PADDED_MAP)
    lived, pol = inp.lived_in(text, inp.PADDED_HORIZON, False, inp.PADDED_STEPS), policy_of(text, inp.PADDED_HORIZON)
    A, n = 3, inp.LIVED_ENVS
    bw = BatchedWorld(text, n, device="cuda:0")
    assert bw.n_agents == A and bw.pos.stride(0) > 2 * A and bw.avail.stride(0) >= A and bw.actions.stride(0) >= A
    for t in range(inp.PADDED_STEPS):
        bw.step(sample=True, auto_reset=True, seed=inp.LIVED_SEED, t=t)
    want = lived.want[-1]
    assert_steps(pol, bw, want, "before")
    actions, steps = pol.actions(bw)
    assert_answers(steps, actions, want, np.array([policy_ref.joint_of(c, A) for c in lived.last_codes], np.uint8), "before")
    pos, bits, beams = bw.pos.clone(), bw.bits.clone(), bw.beams.clone()
    gen = torch.Generator(device=bw.device).manual_seed(7)
    bw.avail.copy_(torch.randint(0, 256, (n, A), dtype=torch.uint8, device=bw.device, generator=gen))
    assert fill_padding(torch, bw, "pos", 2 * A) >= (n - 1) * (bw.pos.stride(0) - 2 * A) > 0
    assert fill_padding(torch, bw, "avail", A) >= (n - 1) * (bw.avail.stride(0) - A)
    bw.gems.copy_(torch.randint(-2 ** 31, 2 ** 31, (n,), dtype=torch.int64, device=bw.device, generator=gen).to(torch.int32))
    assert torch.equal(bw.pos, pos) and torch.equal(bw.bits, bits) and torch.equal(bw.beams, beams), "the identity itself is untouched"
    assert_steps(pol, bw, want, "after")
    after_actions, after_steps = pol.actions(bw)
    assert torch.equal(after_actions, actions) and torch.equal(after_steps, steps)
    # act: the first A bytes of every action row, nothing else of it
    raw, row = raw_rows(torch, bw, "actions")
    raw.fill_(0xEE)
    got = pol.act(bw)
    torch.cuda.synchronize()
    assert torch.equal(got, steps) and torch.equal(bw.actions, actions)
    padding = (torch.arange(raw.numel(), device=raw.device) % row) >= A
    assert int(padding.sum().item()) >= (n - 1) * (bw.actions.stride(0) - A) and (raw[padding] == 0xEE).all().item()


def test_the_gem_word_counts_when_gems_are_collected(torch):
    """GEMS, two gems.  The gem word of every environment is replaced by another one: the plain table answers as before; the
    collect_gems table answers what the restatement's dictionary holds for the perturbed identity, UNKNOWN where it holds none (a state
    nobody can reach, or a bit beyond the map's gems).  At least one answer changes."""
    from lle_amd import BatchedWorld
    n, G = inp.LIVED_ENVS, 2
    lived = inp.lived_in(inp.GEMS, 12, True, inp.PADDED_STEPS)
    plain_lived = inp.lived_in(inp.GEMS, 12, False, inp.PADDED_STEPS)
    with_gems, plain = policy_of(inp.GEMS, 12, True), policy_of(inp.GEMS, 12, False)
    table = policy_ref.build(inp.GEMS, 12, True).table
    bw = BatchedWorld(inp.GEMS, n, device="cuda:0")
    for t in range(inp.PADDED_STEPS):
        bw.step(sample=True, auto_reset=True, seed=inp.LIVED_SEED, t=t)
    words = np.array([inp.gem_word(row) for row in lived.gems[-1]], np.int32)
    assert np.array_equal(bw.gems.cpu().numpy(), words), "bit g of the gem word is gem g of the oracle"
    assert_steps(with_gems, bw, lived.want[-1], "collect_gems, before")
    assert_steps(plain, bw, plain_lived.want[-1], "plain, before")
    flips = np.array([(1 + e % 3) if e % 10 else (1 << 7) for e in range(n)], np.int32)  # a gem, the other, both; every tenth a bit no gem has
    bw.gems.copy_(torch.from_numpy(words ^ flips).to(bw.device))
    want = np.array([inp.answer_with_gems(table, lived.keys[e], int(words[e] ^ flips[e]), G) for e in range(n)], np.int32)
    assert (want != lived.want[-1]).any() and (want == U).any() and (want >= 0).any()
    assert_steps(with_gems, bw, want, "collect_gems, perturbed")
    assert_steps(plain, bw, plain_lived.want[-1], "plain, perturbed")
    actions, steps = with_gems.actions(bw)
    assert (actions[steps < 0] == STAY).all().item()
