"""The shortest-plan search on the MI355X (liblle_search.so, lle_amd.solver, lle_amd.characterization.WorldCharacterizer) against the
reference's own expectations (tests/golden/kat_solver.json) and against the restatement of the search over the oracle
(tests/search_ref.py): answers, plans replayed on the oracle, and the per-depth counters, which pin the state identity, the
enumeration of available joint actions and the piece boundaries."""
import pytest

from oracle.levels import LEVELS
from tests import search_ref

pytestmark = pytest.mark.gpu

CASES = search_ref.load_cases()
CATALOGUE = {c["name"]: c for c in CASES["catalogue"]}
# the layouts the oracle restatement does not finish quickly (tests/test_search_ref_cpu.py says why): checked against the fixtures only
NO_REF = ("level-2", "level-3", "level-4")
N, S, E, W, STAY = range(5)

TERMINATION_EXHAUSTED = "S0 S1 S2\n. . .\nL1E . .\nX X X"
FIVE_LANES = " @ ".join(f"S{k} . X" for k in range(5))
# a beam of 39 cells (two beam words) of colour 1 over a short lane: agent 1 can walk into it and cut both words
LONG_BEAM = "L1E" + " ." * 39 + "\nS1 S0 . X X" + " @" * 35
GEMS = "S0 . G .\n.  . . .\nX  . . G"
MODES = ("standard", "no-cooperation")


@pytest.fixture(scope="module")
def solver_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import solver
    return solver


def values(plan):
    return None if plan is None else [[a.value for a in row] for row in plan]


def run(solver_mod, text, t_max, mode="standard", collect_gems=False, **options):
    """(plan as rows of action values or None, last_stats) of one fresh Solver."""
    s = solver_mod.Solver(text, t_max, **options)
    plan = values(s.find_shortest(mode, collect_gems=collect_gems))
    stats = s.last_stats
    s.free()
    return plan, stats


def assert_equals_ref(solver_mod, text, t_max, mode="standard", collect_gems=False, **options):
    ref = search_ref.search(text, t_max, mode, collect_gems)
    plan, stats = run(solver_mod, text, t_max, mode, collect_gems, **options)
    print(f"{mode} collect_gems={collect_gems} {options}: length {stats['length']} (ref {ref.length}), frontier {stats['frontier']}, expanded {stats['expanded']}")
    assert stats["length"] == ref.length and (plan is None) == (ref.length is None)
    assert stats["frontier"] == ref.frontier and stats["expanded"] == ref.expanded
    assert stats["n_states"] == ref.n_states
    if plan is not None:
        search_ref.check_plan(text, plan, mode, collect_gems, length=ref.length)
    return plan, stats


# ---------------------------------------------------------------------------------------------------------------- catalogue
def characterize(text, t_max):
    """(solvable, cooperative, independent, shortest plan, shortest independent plan) of a fresh WorldCharacterizer."""
    from lle_amd import World, WorldCharacterizer
    c = WorldCharacterizer(World(text), t_max)
    out = (c.is_solvable(), c.is_cooperative(), c.is_independent(), values(c.shortest_path), values(c.shortest_independent_path))
    assert c.is_solvable() is out[0] and values(c.shortest_path) == out[3], "results are cached"
    c._solver.free()
    return out


@pytest.mark.parametrize("name", sorted(CATALOGUE))
def test_catalogue(solver_mod, name):
    """WorldCharacterizer gives what python/tests/world_layouts.py states for the layout at every stated t_max, and every plan it
    returns replays on the oracle.  Every stated horizon gets a characterizer of its own, the twenty of level-3 included (the ten below
    the lower bound are answered without a launch, the others are searches of a few thousand states)."""
    case = CATALOGUE[name]
    text = search_ref.map_text(case)
    horizons = sorted(int(t) for t in case["expect"])
    t_top = max(horizons)
    answers = {}
    for t in horizons:
        solvable, cooperative, independent, plan, independent_plan = characterize(text, t)
        answers[t] = dict(solvable=solvable, cooperative=cooperative, independent=independent)
        print(f"{name} t_max={t}: {answers[t]} shortest {None if plan is None else len(plan)} independent {None if independent_plan is None else len(independent_plan)}")
        for mode, p in (("standard", plan), ("no-cooperation", independent_plan)):
            if p is not None:
                assert len(p) <= t
                search_ref.check_plan(text, p, mode)
                if name not in NO_REF:
                    assert len(p) == search_ref.search(text, t_top, mode).length
        if t == t_top:
            lengths = (None if plan is None else len(plan), None if independent_plan is None else len(independent_plan))
    for t in horizons:
        for key, want in case["expect"][str(t)].items():
            assert answers[t][key] is want, (name, t, key, want, answers[t])
    if name in ("level-3", "level-4"):  # optimal because it equals the lower bound
        from lle_amd import Map
        assert lengths[0] == 10 == solver_mod.lower_bound(Map(text))


# ---------------------------------------------------------------------------------------------------------------- the solver's interface
@pytest.mark.parametrize("case", CASES["solver"]["lengths"], ids=[c["name"] for c in CASES["solver"]["lengths"]])
def test_solver_lengths(solver_mod, case):
    from lle_amd import Action, World
    world = World(case["map"])
    if case["call"] == "solve":
        plan = solver_mod.solve(world, case["t_max"], path_length=case["path_length"])
    else:
        plan = solver_mod.Solver(world, case["t_max"]).find_shortest(t_min=case["t_min"])
    assert plan is not None and len(plan) == case["length"]
    assert all(isinstance(row, tuple) for row in plan) and all(isinstance(a, Action) for row in plan for a in row)
    search_ref.check_plan(case["map"], values(plan), length=case["length"])  # a padded plan ends solved at the requested length
    world.reset()  # ... and runs on the World facade like the reference's test_solve_plan_is_executable
    for joint in plan:
        world.step(list(joint))
    assert all(a.has_arrived for a in world.agents)


@pytest.mark.parametrize("case", CASES["solver"]["solvable"], ids=[c["name"] for c in CASES["solver"]["solvable"]])
def test_solver_solvable_maps(solver_mod, case):
    plan = solver_mod.solve(case["map"], case["t_max"])
    assert (plan is not None) is case["solvable"]
    ref = search_ref.search(case["map"], case["t_max"])
    assert (ref.length is not None) is case["solvable"]
    if plan is not None:
        search_ref.check_plan(case["map"], values(plan), length=case["t_max"])
        assert len(values(solver_mod.Solver(case["map"], case["t_max"]).find_shortest())) == ref.length


def test_solver_collect_gems_fixture(solver_mod):
    case = CASES["solver"]["collect_gems"][0]
    s = solver_mod.Solver(case["map"], case["t_max"])
    assert (s.solve(collect_gems=False) is not None) is case["solvable"]
    with_gems = s.solve(collect_gems=True)
    assert (with_gems is not None) is case["solvable_with_gems"]
    search_ref.check_plan(case["map"], values(with_gems), collect_gems=True, length=case["t_max"])
    assert s.solve(1) is None and s.solve(0) is None  # below the lower bound


def test_padding_and_modes(solver_mod):
    text = CATALOGUE["one-way-detour"]["map"]
    s = solver_mod.Solver(text, 11)
    assert len(s.find_shortest()) == 6 and len(s.find_shortest("no-cooperation")) == 10
    assert len(s.find_shortest(t_min=9)) == 9 and len(s.find_shortest(solver_mod.SolveMode.no_cooperation(), t_min=11, shuffle=True)) == 11
    assert s.find_shortest("no-cooperation", t_min=3) is not None and len(s.solve(7)) == 7 and s.solve(7, mode="no-cooperation") is None
    search_ref.check_plan(text, values(s.solve(11, mode="no-cooperation")), "no-cooperation", length=11)
    search_ref.check_plan(text, values(s.find_shortest(t_min=9)), length=9)
    assert solver_mod.Solver(text, 9).find_shortest("no-cooperation") is None  # the detour opens at 10
    with pytest.raises(NotImplementedError, match="no-asymmetric"):
        s.find_shortest("no-asymmetric")


# ---------------------------------------------------------------------------------------------------------------- counters
FAST = ["level-1", "open-two-agent", "open-two-agent-wide", "one-way-detour", "single-laser-asymmetric", "convergent-2-tight", "divergent-2-with-detour",
        "paper-sequence-2", "paper-convergent-2", "two-agent-mutual-with-detours", "paper-interdependent-3", "unsolvable-4agents", "blocked-unsolvable"]
CONFIGS = {"defaults": {}, "small": dict(chunk=64, max_states=4096)}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FAST)
def test_counters_equal_the_restatement(solver_mod, name, mode, config):
    """frontier and expanded by depth, exactly: with the default sizes (one piece per level) and with chunk=64, max_states=4096 (many
    pieces per level, a table of 8 192 slots)."""
    case = CATALOGUE[name]
    assert_equals_ref(solver_mod, search_ref.map_text(case), max(int(t) for t in case["expect"]), mode, **CONFIGS[config])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["open-two-agent", "single-laser-asymmetric", "blocked-unsolvable", "paper-sequence-2", "convergent-2-tight"])
def test_counters_one_item_per_piece(solver_mod, name, mode):
    """chunk=1 is four launches per work item, all 5^A codes of every state: the layouts are the small ones -- two agents, an
    unsolvable one, two three-agent layouts (pitch 4; at most 363 states x 125 codes), and in single-laser-asymmetric and
    convergent-2-tight a no-cooperation search that rejects states the standard search keeps."""
    case = CATALOGUE[name]
    assert_equals_ref(solver_mod, search_ref.map_text(case), max(int(t) for t in case["expect"]), mode, chunk=1, max_states=512)


# ---------------------------------------------------------------------------------------------------------------- termination
def test_exhausted_state_space_returns_none(solver_mod):
    """Agent 0 cannot pass the beam of colour 1 and agent 1 cannot hold it off for long enough: every state is reached by depth 9."""
    for options in ({}, dict(chunk=64, max_states=4096)):
        plan, stats = assert_equals_ref(solver_mod, TERMINATION_EXHAUSTED, 30, **options)
        assert plan is None and stats["n_states"] == 350 and len(stats["frontier"]) == 10 and stats["frontier"][-1] == 0


def test_level_3_stops_at_the_horizon(solver_mod):
    """t_max = 9 is below the lower bound of 10, so find_shortest answers without a search; the search itself, asked all the same,
    expands nine levels and stops with a frontier that is not empty."""
    s = solver_mod.Solver(LEVELS[3], 9)
    assert s.find_shortest() is None and s.last_stats is None and s.solve() is None
    assert s._shortest(solver_mod.SolveMode.standard(), False) is None
    stats = s.last_stats
    print(stats)
    assert stats["length"] is None and len(stats["expanded"]) == 9 and len(stats["frontier"]) == 10 and stats["frontier"][-1] > 0
    s.free()


def test_an_exit_freezes_the_agent_that_reaches_it(solver_mod):
    plan, stats = assert_equals_ref(solver_mod, "S0 . S1 . X X", 12)
    assert plan is None


# ---------------------------------------------------------------------------------------------------------------- capacity
def test_capacity_and_neighbours(solver_mod):
    import torch

    from lle_amd import BatchedWorld
    text = CATALOGUE["paper-fully-coupled"]["map"]
    ref = search_ref.search(text, 10)
    small = solver_mod.Solver(text, 10, max_states=64)
    with pytest.raises(solver_mod.SolverCapacityError, match="max_states"):
        small.find_shortest()
    with pytest.raises(solver_mod.SolverCapacityError):
        small.find_shortest()  # no answer is cached
    second = solver_mod.Solver(text, 10, chunk=512, max_states=4096)  # a second handle beside the first
    bw = BatchedWorld(text, 64, device="cuda:0")
    bw.step(sample=True, seed=5, t=0)
    first = values(second.find_shortest())
    stats = second.last_stats
    bw.step(sample=True, seed=5, t=1)
    after = bw.host_buffers()
    rebuilt = solver_mod.Solver(text, 10)  # the same world, now with the default capacity
    plan = values(rebuilt.find_shortest())
    assert len(plan) == len(first) == ref.length
    assert rebuilt.last_stats["frontier"] == stats["frontier"] == ref.frontier and rebuilt.last_stats["expanded"] == stats["expanded"] == ref.expanded
    search_ref.check_plan(text, plan, length=ref.length)
    search_ref.check_plan(text, first, length=ref.length)
    # the searches beside it did not touch the stepped batch
    twin = BatchedWorld(text, 64, device="cuda:0")
    twin.step(sample=True, seed=5, t=0)
    twin.step(sample=True, seed=5, t=1)
    want = twin.host_buffers()
    for key in ("pos", "bits", "gems", "beams", "avail"):
        assert torch.equal(torch.as_tensor(after[key]), torch.as_tensor(want[key])), key
    with pytest.raises(solver_mod.SolverCapacityError):
        small.find_shortest("standard")
    for s in (small, second, rebuilt):
        s.free()


# ---------------------------------------------------------------------------------------------------------------- pitches, beam words, gems
def test_agent_pitches_and_beam_words(solver_mod):
    from lle_amd import Map
    three = CATALOGUE["three-agent-temporal-cycle"]
    assert Map(three["map"]).n_agents == 3  # pitch 4
    for mode in MODES:
        assert_equals_ref(solver_mod, three["map"], 15, mode)
        assert_equals_ref(solver_mod, three["map"], 15, mode, chunk=100, max_states=1000)
    assert Map(FIVE_LANES).n_agents == 5  # pitch 8, 3 125 joint actions per state
    for options in ({}, dict(chunk=1000, max_states=512)):
        plan, _ = assert_equals_ref(solver_mod, FIVE_LANES, 4, **options)
        assert len(plan) == 2
    assert_equals_ref(solver_mod, CATALOGUE["unsolvable-4agents"]["map"], 10)
    long_map = Map(LONG_BEAM)
    assert long_map.max_beam_len == 39 and long_map.n_beam_words >= 2 and long_map.n_agents == 2  # (maps with a long beam are padded to 5 words)
    for mode in MODES:
        for options in ({}, dict(chunk=64, max_states=4096)):
            assert_equals_ref(solver_mod, LONG_BEAM, 8, mode, **options)


def test_collect_gems(solver_mod):
    plain, _ = assert_equals_ref(solver_mod, GEMS, 12)
    for options in ({}, dict(chunk=64, max_states=4096)):
        with_gems, _ = assert_equals_ref(solver_mod, GEMS, 12, collect_gems=True, **options)
        assert len(plain) < len(with_gems)
    assert_equals_ref(solver_mod, GEMS, 12, "no-cooperation", collect_gems=True)


def test_refusals_on_the_device(solver_mod):
    with pytest.raises(ValueError, match="at most 6 agents"):
        solver_mod.Solver(" ".join(f"S{k}" for k in range(7)) + " X" * 7, 4)
    s = solver_mod.Solver("S0 . X", 0)  # a horizon of no steps: the search itself answers with the start state alone
    assert s._shortest(solver_mod.SolveMode.standard(), False) is None and s.last_stats == dict(frontier=[1], expanded=[], n_states=1, length=None)
    assert s.find_shortest() is None
    arrived = solver_mod.Solver("S0 X", 3)  # nothing to do is not this map: one step
    assert len(arrived.find_shortest()) == 1


def test_every_kernel_was_launched(solver_mod):
    """(last in the module: the tests above launch both insert kernels.)"""
    assert sorted(solver_mod.compiled_kernels()) == ["search_commit", "search_expand", "search_insert<false>", "search_insert<true>"]
    assert set(solver_mod.launched_kernels()) == set(solver_mod.compiled_kernels())
