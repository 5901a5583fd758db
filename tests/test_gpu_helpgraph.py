"""The help-graph search on the MI355X (liblle_helpgraph.so, lle_amd.helpgraph) against the reference's stated values
(tests/golden/kat_helpgraph.json: `catalogue`) and against the restatement of the search over the oracle (tests/helpgraph_ref.py), whose
per-depth counters for every listed search are recorded in the same file (`searches`; tests/test_helpgraph_cpu.py holds the
restatement to every one of them, so no test here walks a search in Python).  The counters pin the identity of a record -- help words
included -- the edge rule, the enumeration of joint actions and the piece boundaries; every plan is replayed on the oracle."""
import ctypes as C

import pytest

from tests import helpgraph_ref

pytestmark = pytest.mark.gpu

CASES = helpgraph_ref.load_cases()
CATALOGUE = {c["name"]: c for c in CASES["catalogue"]}
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"]}, **CASES["maps"])
SEARCHES = CASES["searches"]
# many pieces per level: candidates with equal key words meet as tags inside a piece and as pool records across pieces
CONFIGS = {"defaults": {}, "chunk64": dict(chunk=64, max_states=16384)}


def search_id(s):
    return f"{s['map']}-t{s['t_max']}-{s['mode']}-{s['param']}" + ("-gems" if s["collect_gems"] else "") + helpgraph_ref.changes_label(s.get("changes"))


def mode_text(mode, param=2):
    return f"{mode}-{param}" if mode in ("no-convergence", "no-divergence") else mode


@pytest.fixture(scope="module")
def hg():
    import torch
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from lle_amd import helpgraph
    return helpgraph


def values(plan):
    return None if plan is None else [[a.value for a in row] for row in plan]


def run(hg, text, t_max, mode="standard", param=2, collect_gems=False, changes=None, **options):
    """(plan as rows of action values or None, last_stats) of one fresh HelpGraphSolver, over a World that `changes` was applied to
    (tests/helpgraph_ref.py: apply_changes) when there are any."""
    if changes is not None:
        from lle_amd import World
        text = helpgraph_ref.apply_changes(World(text), changes)
    s = hg.HelpGraphSolver(text, t_max, **options)
    try:
        plan = values(s.find_shortest(mode_text(mode, param), collect_gems=collect_gems))
        return plan, s.last_stats
    finally:
        s.free()


def assert_recorded(hg, s, text=None, **options):
    """One search of the golden file: length, counters and state count equal the restatement's; the plan replays on the oracle under the mode
    (and under the entry's `changes`, if it has any)."""
    text, changes = MAPS[s["map"]] if text is None else text, s.get("changes")
    plan, stats = run(hg, text, s["t_max"], s["mode"], s["param"], s["collect_gems"], changes, **options)
    print(f"{search_id(s)} {options}: length {stats['length']} (ref {s['length']}), states {stats['n_states']} (ref {s['states']}), frontier {stats['frontier']}, "
          f"expanded {stats['expanded']}")
    assert stats["length"] == s["length"] and (plan is None) == (s["length"] is None)
    assert stats["frontier"] == s["frontier"] and stats["expanded"] == s["expanded"] and stats["n_states"] == s["states"]
    if plan is None:
        assert stats["help_edges"] is None
    else:
        edges = helpgraph_ref.check_plan(text, plan, s["mode"], s["param"], s["collect_gems"], length=s["length"], changes=changes)
        assert stats["help_edges"] == edges, "the goal's help words are the flattened edges of the plan's replay"
    return plan, stats


# (a six-agent map has 15 625 joint actions per state: in pieces of 64 no piece ever holds two states, at half a million launches;
# test_six_agents_reach_the_second_help_word and tests/test_gpu_helpgraph_maps.py run them with the default chunk and with 4 096)
LISTED = [s for s in SEARCHES if helpgraph_ref.n_agents_of(MAPS[s["map"]]) < 6]


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("s", LISTED, ids=[search_id(s) for s in LISTED])
def test_counters_and_plans(hg, s, config):
    assert_recorded(hg, s, **CONFIGS[config])


def test_the_table_of_the_issue_is_listed():
    """Every (layout, t_max, mode) row the feature was specified with, by length and states stored."""
    N = None
    rows = [("single-laser-asymmetric", 6, "standard", 2, 2, 14), ("single-laser-asymmetric", 6, "no-asymmetric", 2, N, 26),
            ("divergent-2-tight", 8, "no-asymmetric", 2, N, 480), ("divergent-2-tight", 8, "no-divergence", 2, N, 252), ("divergent-2-tight", 8, "no-divergence", 3, 2, 73),
            ("divergent-2-with-detour", 5, "no-divergence", 2, N, 963), ("divergent-2-with-detour", 6, "no-divergence", 2, 6, 1408),
            ("convergent-2-tight", 5, "no-convergence", 2, N, 245), ("convergent-2-tight", 5, "no-convergence", 3, 5, 505),
            ("two-agent-mutual-compact", 6, "standard", 2, 5, 123), ("two-agent-mutual-compact", 6, "no-asymmetric", 2, 5, 123),
            ("two-agent-mutual-compact", 6, "no-mutual", 2, N, 100), ("two-agent-mutual-with-detours", 7, "no-mutual", 2, N, 924),
            ("two-agent-mutual-with-detours", 8, "no-mutual", 2, 8, 1225),
            ("paper-fully-coupled", 10, "standard", 2, 8, 3965), ("paper-fully-coupled", 10, "no-asymmetric", 2, 8, 3965), ("paper-fully-coupled", 10, "no-mutual", 2, N, 4617),
            ("paper-fully-coupled", 10, "no-fully-coupled", 2, N, 6509), ("paper-fully-coupled", 10, "no-convergence", 2, N, 4016),
            ("paper-fully-coupled", 10, "no-divergence", 2, N, 1199),
            ("paper-convergent-2", 10, "no-asymmetric", 2, N, 4492), ("paper-convergent-2", 10, "no-convergence", 2, N, 2797), ("paper-convergent-2", 10, "no-divergence", 2, 5, 1003),
            ("paper-fully-coupled-legacy", 10, "standard", 2, 6, 4375), ("paper-fully-coupled-legacy", 10, "no-asymmetric", 2, 6, 4375),
            ("paper-fully-coupled-legacy", 10, "no-mutual", 2, N, 2064), ("paper-fully-coupled-legacy", 10, "no-fully-coupled", 2, N, 7599),
            ("paper-fully-coupled-legacy", 10, "no-convergence", 2, N, 1744), ("paper-fully-coupled-legacy", 10, "no-convergence", 3, 6, 4375),
            ("paper-fully-coupled-legacy", 10, "no-divergence", 2, N, 930), ("paper-fully-coupled-legacy", 10, "no-divergence", 3, 6, 4375),
            ("six-agents", 4, "standard", 2, 2, 616), ("six-agents", 4, "no-asymmetric", 2, N, 2184)]
    listed = {(s["map"], s["t_max"], s["mode"], s["param"], s["length"], s["states"]) for s in SEARCHES if not s["collect_gems"]}
    assert set(rows) <= listed


# ---------------------------------------------------------------------------------------------------------------- characterizer
# fully-coupled-4agents is beyond the restatement (84 128 records within t_max 8; tests/golden/make_kat_helpgraph.py): the searches through
# World.step find no plan of 8 steps on it, so the stated fully_coupled and interdependent[2] are not reproduced and not asserted here;
# test_standard_mode_has_the_length_of_the_plain_search covers the layout.
RESTATED = sorted(set(CATALOGUE) - {"fully-coupled-4agents"})


@pytest.mark.parametrize("name", sorted(CATALOGUE))
def test_standard_mode_has_the_length_of_the_plain_search(hg, name):
    """`standard` through the new library against Solver.find_shortest() (liblle_search.so), on every layout at every stated t_max."""
    from lle_amd import Solver
    case = CATALOGUE[name]
    for t in sorted(int(t) for t in case["expect"]):
        ours, plain = hg.HelpGraphSolver(case["map"], t), Solver(case["map"], t)
        try:
            a, b = ours.find_shortest("standard"), plain.find_shortest()
            print(name, t, None if a is None else len(a), ours.last_stats["n_states"], plain.last_stats and plain.last_stats["n_states"])
            assert (a is None) == (b is None) and (a is None or len(a) == len(b))
            if a is not None:
                helpgraph_ref.check_plan(case["map"], values(a))
        finally:
            ours.free()
            plain.free()


@pytest.mark.parametrize("name", RESTATED)
def test_characterizer(hg, name):
    """HelpGraphCharacterizer gives what python/tests/world_layouts.py states for the layout at every stated t_max, and the generator's
    Asymmetric() atom over it agrees."""
    from lle_amd import Asymmetric, Constraint, Solver, World
    case = CATALOGUE[name]
    for t, expect in sorted(case["expect"].items(), key=lambda kv: int(kv[0])):
        c = hg.HelpGraphCharacterizer(World(case["map"]), int(t))
        plain = Solver(case["map"], int(t))
        try:
            got = {}
            for key, want in expect.items():
                if key == "asymmetric":
                    got[key] = c.is_asymmetric()
                    assert Constraint(int(t), Asymmetric()).is_satisfied_by(World(case["map"]), characterizer=hg.HelpGraphCharacterizer) is want
                elif key == "fully_coupled":
                    got[key] = c.is_fully_coupled()
                elif key == "interdependent":
                    got[key] = {k: c.is_interdependent(int(k)) for k in want}
                    assert c.is_mutual() is got[key]["2"]
                else:
                    got[key] = {k: (c.is_convergent if key == "convergent" else c.is_divergent)(int(k)) for k in want}
            print(name, t, got)
            assert got == expect
            ours, theirs = c.shortest_path, plain.find_shortest()
            assert (ours is None) == (theirs is None) and (ours is None or len(ours) == len(theirs))
        finally:
            c._solver.free()
            plain.free()


def test_constraint_with_two_atoms(hg):
    from lle_amd import Asymmetric, Constraint, Convergent, Divergent, World
    w = World(MAPS["divergent-2-tight"])
    assert Constraint(8, Asymmetric() & ~Convergent(2)).is_satisfied_by(w, characterizer=hg.HelpGraphCharacterizer) is True
    assert Constraint(8, Asymmetric() & ~Divergent(2)).is_satisfied_by(w, characterizer=hg.HelpGraphCharacterizer, chunk=4096) is False
    with pytest.raises(NotImplementedError):  # the default characterizer is unchanged
        Constraint(8, Asymmetric()).is_satisfied_by(w)


# ---------------------------------------------------------------------------------------------------------------- shapes
def test_six_agents_reach_the_second_help_word(hg):
    """Helper 5's byte lies in the second help word: the goal edges of the standard plan are {(5, 4)}."""
    standard = next(s for s in SEARCHES if s["map"] == "six-agents" and s["mode"] == "standard")
    _plan, stats = assert_recorded(hg, standard)
    assert (stats["length"], stats["n_states"], stats["help_edges"]) == (2, 616, {(5, 4)})
    none = next(s for s in SEARCHES if s["map"] == "six-agents" and s["mode"] == "no-asymmetric")
    assert (none["length"], none["states"]) == (None, 2184)
    assert_recorded(hg, none, chunk=4096)


def test_cell_table_in_global_memory(hg):
    """single-laser-asymmetric in the top-left corner of a 65 x 66 map of walls: 4 290 cells are more than 16 KB of table, so the
    insert kernel reads it from global memory; the counters are the 3 x 3 layout's."""
    rows = [line.split() for line in MAPS["single-laser-asymmetric"].strip().splitlines()]
    big = "\n".join(" ".join((rows[i][j] if i < 3 and j < 3 else "@") for j in range(66)) for i in range(65))
    for s in SEARCHES:
        if s["map"] == "single-laser-asymmetric":
            assert_recorded(hg, s, text=big, chunk=256, max_states=1024)
    assert "hg_insert<false>" in hg.launched_kernels()


def test_collect_gems_changes_the_length(hg):
    without, with_gems = [s for s in SEARCHES if s["map"] == "gem-detour"]
    assert (without["mode"], with_gems["mode"]) == ("no-asymmetric", "no-asymmetric") and not without["collect_gems"] and with_gems["collect_gems"]
    assert without["length"] == 5 and with_gems["length"] == 7
    s = hg.HelpGraphSolver(MAPS["gem-detour"], 8)  # one handle, both searches: the gem word joins the identity per run
    try:
        assert len(s.find_shortest("no-asymmetric")) == 5 and s.last_stats["frontier"] == without["frontier"]
        plan = values(s.find_shortest("no-asymmetric", collect_gems=True))
        assert len(plan) == 7 and s.last_stats["frontier"] == with_gems["frontier"] and s.last_stats["expanded"] == with_gems["expanded"]
        helpgraph_ref.check_plan(MAPS["gem-detour"], plan, "no-asymmetric", collect_gems=True)
        assert len(s.find_shortest("no-asymmetric")) == 5 and s.last_stats["n_states"] == without["states"]  # (cached per mode and collect_gems)
    finally:
        s.free()


def test_interface_on_the_device(hg):
    """STAY padding, solve(path_length), the delegated no-cooperation, and the cache."""
    from lle_amd import Action, Solver
    text = MAPS["two-agent-mutual-compact"]
    s, plain = hg.HelpGraphSolver(text, 8), Solver(text, 8)
    try:
        plan = s.find_shortest("no-asymmetric", t_min=7)
        assert len(plan) == 7 and plan[5:] == [(Action.STAY, Action.STAY)] * 2 and s.last_stats["help_edges"] == {(0, 1), (1, 0)}
        assert len(s.solve(8, mode="no-asymmetric")) == 8 and s.solve(4, mode="no-asymmetric") is None
        assert s.find_shortest("no-mutual") is None and s.find_shortest("no-interdependence-2") is None and s.last_stats["length"] is None
        assert values(s.find_shortest("no-cooperation")) == values(plain.find_shortest("no-cooperation"))
        assert s.last_stats == plain.last_stats
    finally:
        s.free()
        plain.free()


def test_capacity(hg):
    """A pool of 16 records overflows on paper-convergent-2: SolverCapacityError, no partial plan, and the solver object still answers."""
    from lle_amd import SolverCapacityError
    s = hg.HelpGraphSolver(MAPS["paper-convergent-2"], 10, max_states=16)
    try:
        for mode in ("standard", "no-divergence"):
            with pytest.raises(SolverCapacityError, match="max_states = 16"):
                s.find_shortest(mode)
        assert s.solution_lower_bound == 4 and s._cache == {}
    finally:
        s.free()


def test_run_refusals_on_a_handle(hg):
    """Wrong struct_bytes, unknown mode, param < 2, negative t_max; lle_helpgraph_plan after a run without a plan."""
    from lle_amd import Map
    L = hg.lib()
    map_ = Map(MAPS["single-laser-asymmetric"])  # (kept: the handle of a temporary would be freed before the call)
    h = L.lle_helpgraph_create(map_.h, None)
    assert h, L.lle_helpgraph_last_error()
    try:
        A, R = hg.HelpGraphArgs, hg.HelpGraphResult
        res = R(C.sizeof(R))
        for args, result, word in ((A(4, 0, 2, 0, 5), res, b"lle_helpgraph_args.struct_bytes"), (A(C.sizeof(A), 0, 2, 0, 5), R(8), b"lle_helpgraph_result.struct_bytes"),
                                   (A(C.sizeof(A), 6, 2, 0, 5), res, b"unknown mode"), (A(C.sizeof(A), -1, 2, 0, 5), res, b"unknown mode"),
                                   (A(C.sizeof(A), hg.LLE_HELPGRAPH_NO_CONVERGENCE, 1, 0, 5), res, b"param"),
                                   (A(C.sizeof(A), hg.LLE_HELPGRAPH_NO_DIVERGENCE, 0, 0, 5), res, b"param"), (A(C.sizeof(A), 0, 2, 0, -1), res, b"t_max")):
            assert L.lle_helpgraph_run(h, C.byref(args), C.byref(result)) == -2 and word in L.lle_helpgraph_last_error()
        assert L.lle_helpgraph_run(h, None, C.byref(res)) == -1 and L.lle_helpgraph_run(h, C.byref(A(C.sizeof(A), 0, 2, 0, 5)), None) == -1
        assert L.lle_helpgraph_run(h, C.byref(A(C.sizeof(A), hg.LLE_HELPGRAPH_NO_MUTUAL, 0, 0, 6)), C.byref(res)) == 0  # (param is ignored by the other modes)
        assert (res.length, res.n_states, res.help_lo, res.help_hi) == (2, 14, 1 << 1, 0)
        buf = (C.c_uint8 * 4)()
        assert L.lle_helpgraph_plan(h, buf, 3) == -2 and L.lle_helpgraph_plan(h, None, 4) == -2 and L.lle_helpgraph_plan(h, buf, 4) == 2
        assert L.lle_helpgraph_run(h, C.byref(A(C.sizeof(A), hg.LLE_HELPGRAPH_NO_ASYMMETRIC, 0, 0, 6)), C.byref(res)) == 0
        assert (res.length, res.n_states, res.depth_reached, res.help_lo, res.help_hi) == (-1, 26, 5, 0, 0)
        assert L.lle_helpgraph_plan(h, buf, 4) == -2 and b"no plan" in L.lle_helpgraph_last_error()
        frontier, expanded = (C.c_int64 * 8)(), (C.c_int64 * 8)()
        assert L.lle_helpgraph_stats(h, frontier, expanded, 8) == 6 and list(frontier[:6]) == [1, 2, 11, 9, 3, 0] and list(expanded[:5]) == [4, 21, 57, 43, 10]
        assert L.lle_helpgraph_stats(h, None, None, 0) == 6
    finally:
        L.lle_helpgraph_free(h)


def test_root_states(hg):
    """The reset state carries its own edges: all three agents start on the beam agent 0 blocks, so every record holds (0, 1) and
    (0, 2).  A reset state the mode rejects gives no plan, one record and no level."""
    text = "L0E S0 S1 S2\n @  X  X  X"
    for mode, param, length in (("standard", 2, 1), ("no-divergence", 3, 1), ("no-divergence", 2, None), ("no-asymmetric", 2, None), ("no-mutual", 2, 1)):
        ref = helpgraph_ref.search(text, 3, mode, param)
        plan, stats = run(hg, text, 3, mode, param)
        assert ref.length == length == stats["length"] and stats["frontier"] == ref.frontier and stats["expanded"] == ref.expanded
        assert stats["help_edges"] == (None if length is None else {(0, 1), (0, 2)})
        if mode == "no-divergence" and param == 2:
            assert (stats["n_states"], stats["frontier"], stats["expanded"]) == (1, [1], [])


def test_every_kernel_was_launched(hg):
    """At the end of this file: the searches above have gone through every kernel the library holds."""
    assert sorted(hg.launched_kernels()) == sorted(hg.compiled_kernels()) == ["hg_commit", "hg_expand", "hg_insert<false>", "hg_insert<true>"]
