"""The help forest without a GPU: header / exports / binding of liblle_helpforest.so, every host-side refusal, HelpForestSolver's
argument errors and mode wording, ManyHelpCharacterization over hand-made answers, the generator's new keyword, the fixed input sets
against the figures the issue states and the golden file against the restatements, and lle_amd/helpforest/helpforest_logic.hpp under
AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program (tests/hostsim/helpforest_pieces.cpp).  The search itself
runs on the MI355X (tests/test_gpu_helpforest.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lle_amd
from lle_amd import Map, World, forest, generator, helpforest, helpgraph, solver, trails
from lle_amd.generator import Asymmetric, Constraint, Convergent, Cooperative, Divergent, Interdependent, Sequential, Solvable
from tests import helpforest_ref
from tests.helpforest_ref import SET_C, SET_G, SET_L, SET_P, SET_R, SET_S, SET_X, SETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
GOLDEN = helpforest_ref.load_golden()


def handles(maps):
    return (C.c_void_p * len(maps))(*[m.h for m in maps])


def options(envs_per_map=0, max_states_per_map=0, struct_bytes=None, device=-1):
    return helpforest.HelpForestOptions(C.sizeof(helpforest.HelpForestOptions) if struct_bytes is None else struct_bytes, device, envs_per_map,
                                        max_states_per_map, None)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_exports_sizes_and_constants():
    """liblle_helpforest.so exports every function include/lle_helpforest.h declares, and the binding knows exactly those; the header
    is plain C; struct sizes, field offsets and constants of the binding are the header's."""
    L = helpforest.lib()
    header = open(os.path.join(ROOT, "include", "lle_helpforest.h")).read()
    declared = set(re.findall(r"\b(lle_helpforest_[a-z_0-9]+)\s*\(", header))
    assert declared == set(helpforest.EXPORTS) and len(helpforest.EXPORTS) == 9
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "helpforest", "helpforest.hip")).read()
    assert '#include "../../include/lle_helpforest.h"' in source and '#include "helpforest_logic.hpp"' in source
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    for foreign in ("lle_helpgraph_create", "lle_trails_create", "lle_forest_create", "lle_search_create"):
        assert foreign not in source  # no symbol of the single-map libraries or of the plain forest
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "lle_helpforest.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d", '
            'sizeof(lle_helpforest_options), sizeof(lle_helpforest_args), sizeof(lle_helpforest_result), offsetof(lle_helpforest_options, stream), '
            'offsetof(lle_helpforest_args, t_max), offsetof(lle_helpforest_result, n_states), offsetof(lle_helpforest_result, depth_reached), '
            'offsetof(lle_helpforest_result, help_lo), offsetof(lle_helpforest_result, trail), (int)LLE_HELPFOREST_NO_SEQUENCE, (int)LLE_HELPFOREST_MAX_AGENTS, '
            '(int)LLE_HELPFOREST_MAX_SOURCES, (int)LLE_HELPGRAPH_NO_DIVERGENCE, (int)LLE_HELPGRAPH_CAPACITY, (int)LLE_TRAILS_DENSE, (int)LLE_TRAILS_WALK_BUDGET); '
            'return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    R = helpforest.HelpForestMapResult
    assert got == [C.sizeof(helpforest.HelpForestOptions), C.sizeof(helpforest.HelpForestArgs), C.sizeof(R), helpforest.HelpForestOptions.stream.offset,
                   helpforest.HelpForestArgs.t_max.offset, R.n_states.offset, R.depth_reached.offset, R.help_lo.offset, R.trail.offset,
                   helpforest.LLE_HELPFOREST_NO_SEQUENCE, helpforest.LLE_HELPFOREST_MAX_AGENTS, helpforest.LLE_HELPFOREST_MAX_SOURCES,
                   helpgraph.LLE_HELPGRAPH_NO_DIVERGENCE, helpgraph.LLE_HELPGRAPH_CAPACITY, trails.LLE_TRAILS_DENSE, trails.LLE_TRAILS_WALK_BUDGET]
    assert helpforest.LLE_HELPFOREST_NO_SEQUENCE == len(helpgraph._NATIVE) == 6 and solver.LLE_SEARCH_CAPACITY == helpgraph.LLE_HELPGRAPH_CAPACITY
    # what the library static_asserts against the logic headers
    logic = open(os.path.join(ROOT, "lle_amd", "helpforest", "helpforest_logic.hpp")).read()
    forest_logic = open(os.path.join(ROOT, "lle_amd", "forest", "forest_logic.hpp")).read()  # (the dense counter lies beside the forest's others)
    assert "NO_SEQUENCE = hl::N_MODES" in logic and "CNT_DENSE = 5" in forest_logic and "LLE_HELPFOREST_NO_SEQUENCE == hfl::NO_SEQUENCE" in source
    assert sorted(helpforest.compiled_kernels()) == sorted(helpforest.KERNELS) and len(helpforest.KERNELS) == 9
    assert helpforest.launched_kernels() == []


def test_build_knows_the_library():
    from lle_amd import build
    assert '("helpforest", "liblle_helpforest.so")' in open(build.__file__).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "helpforest.EXPORTS" in entry and "liblle_helpforest.so does not export" in entry
    assert os.path.exists(helpforest.LIB_PATH)
    ignored = subprocess.run(["git", "check-ignore", "-q", helpforest.LIB_PATH], cwd=ROOT)
    assert ignored.returncode in (0, 128)  # ignored (128: not a git checkout)


def test_lazy_names():
    assert lle_amd.HelpForestSolver is helpforest.HelpForestSolver and lle_amd.HelpForestResult is helpforest.HelpForestResult
    assert lle_amd.ManyHelpCharacterization is helpforest.ManyHelpCharacterization
    assert {"HelpForestSolver", "HelpForestResult", "ManyHelpCharacterization"} <= set(lle_amd.__all__)
    assert lle_amd.solve_many is forest.solve_many and lle_amd.characterize_many is forest.characterize_many  # the plain forest keeps its names


def test_host_side_refusals():
    L = helpforest.lib()
    line, other = Map(LINE), Map("S0 . X .")

    def refused(maps, n, opt, word):
        got = L.lle_helpforest_create(maps, n, None if opt is None else C.byref(opt))
        message = L.lle_helpforest_last_error()
        assert got is None and word in message, (word, message)

    two = handles([line, other])
    refused(None, 1, None, b"NULL maps")
    refused(two, 0, None, b"n_maps must be at least 1")
    refused((C.c_void_p * 2)(line.h, None), 2, None, b"NULL map (entry 1)")
    refused(two, 2, options(struct_bytes=4), b"struct_bytes")
    for E, cap, word in ((-1, 0, b"envs_per_map must be"), ((1 << 30) + 1, 0, b"envs_per_map must be"), (0, -1, b"max_states_per_map"),
                         (0, (1 << 30) + 1, b"max_states_per_map"), (1 << 30, 0, b"n_maps * envs_per_map")):
        refused(two, 2, options(E, cap), word)
    refused(handles([line]), 1, options(1 << 30, 1 << 30), b"must be below 2^31")
    narrow, laser, no_laser, aligned, seven = Map("S0 . X"), Map("S0 . X .\nL0E . . ."), Map("S0 . X .\n. . . ."), Map(LINE, row_align=256), Map(SEVEN)
    refused(handles([line, narrow]), 2, None, b"lle_batch_create_multi: the maps of a batch must agree on height, width")
    refused(handles([laser, no_laser]), 2, None, b"lle_batch_create_multi: the maps of a batch must agree")
    refused(handles([line, aligned]), 2, None, b"row alignment")
    refused(handles([seven]), 1, None, b"more than 6 agents")
    # nothing wrong with the arguments: where they are refused all the same, what is missing is the device
    for maps, n, opt in ((two, 2, None), (two, 2, options(1, 1)), (handles([line]), 1, options(7, 128))):
        got = L.lle_helpforest_create(maps, n, None if opt is None else C.byref(opt))
        assert got is not None or b"no HIP device" in L.lle_helpforest_last_error(), L.lle_helpforest_last_error()
        L.lle_helpforest_free(got)
    # the arguments of a run are judged before the handle is looked at
    res = (helpforest.HelpForestMapResult * 2)()

    def run_refused(word, mode=0, param=2, t_max=3, struct_bytes=None):
        args = helpforest.HelpForestArgs(C.sizeof(helpforest.HelpForestArgs) if struct_bytes is None else struct_bytes, mode, param, 0, t_max)
        assert L.lle_helpforest_run(None, C.byref(args), None, res) < 0 and word in L.lle_helpforest_last_error(), (word, L.lle_helpforest_last_error())

    run_refused(b"struct_bytes", struct_bytes=8)
    run_refused(b"unknown mode", mode=7)
    run_refused(b"unknown mode", mode=-1)
    run_refused(b"param must be at least 2", mode=helpgraph.LLE_HELPGRAPH_NO_CONVERGENCE, param=1)
    run_refused(b"param must be 2 .. 16", mode=helpforest.LLE_HELPFOREST_NO_SEQUENCE, param=17)
    run_refused(b"param must be 2 .. 16", mode=helpforest.LLE_HELPFOREST_NO_SEQUENCE, param=1)
    run_refused(b"t_max must not be negative", t_max=-1)
    run_refused(b"NULL handle")
    assert L.lle_helpforest_plan(None, 0, None, 0) == -1
    assert L.lle_helpforest_stats(None, 0, None, None, 0) == -1
    assert L.lle_helpforest_occupancy(None, None, None) == -1
    L.lle_helpforest_free(None)


# ---------------------------------------------------------------------------------------------------------------- HelpForestSolver
def test_solver_forms_freezing_and_refusals(monkeypatch):
    """Refusals come before any device work: nothing here makes a handle."""
    w = World("S0 . X X")
    f = helpforest.HelpForestSolver([w, Map(LINE), "S0 X . ."], 7, envs_per_map=3, max_states_per_map=5)
    assert isinstance(f, forest.ForestSolver) and (f.t_max, f.envs_per_map, f.max_states_per_map, f.n_maps, f.n_agents, f.h) == (7, 3, 5, 3, 1, None)
    w.exit_pos = [(0, 3)]  # frozen at construction
    assert f._maps[0].positions(1) == [(0, 2), (0, 3)]
    assert helpforest.HelpForestSolver([LINE]).t_max == 2 and helpforest.HelpForestSolver([LINE]).envs_per_map == 256
    with pytest.raises(ValueError, match="at least one world"):
        helpforest.HelpForestSolver([], 5)
    with pytest.raises(ValueError, match="non-negative"):
        helpforest.HelpForestSolver([LINE], -1)
    with pytest.raises(ValueError, match="at least 1"):
        helpforest.HelpForestSolver([LINE], 5, envs_per_map=0)
    with pytest.raises(ValueError, match=r"map 2 does not match map 0 in width \(3, map 0 has 4\)"):
        helpforest.HelpForestSolver([LINE, LINE, "S0 . X"], 5)
    with pytest.raises(ValueError, match="at most 6 agents"):
        helpforest.HelpForestSolver([SEVEN], 4)
    with pytest.raises(ValueError, match="at most 6 agents"):
        helpforest.solve_many([SEVEN, SEVEN], 4, mode="no-mutual")
    # (a map text of more than 32 sources does not parse -- its beams would take more than 32 words -- so the limit is lowered to meet it)
    two_sources = "S0 . X .\nL0E . . .\nL0E . . ."
    assert helpforest.HelpForestSolver([LINE, LINE], 4).n_maps == 2 and helpforest.LLE_HELPFOREST_MAX_SOURCES == 32
    monkeypatch.setattr(helpforest, "LLE_HELPFOREST_MAX_SOURCES", 1)
    with pytest.raises(ValueError, match=r"at most 1 laser sources.*map 0 has 2"):
        helpforest.HelpForestSolver([two_sources, two_sources], 4)
    f = helpforest.HelpForestSolver([LINE, LINE], 5)
    with pytest.raises(ValueError, match="one entry per map"):
        f.run("no-mutual", only=[True])
    assert f.h is None


@pytest.mark.parametrize("text", ["no-interdependence-3", "no-interdependence-5", "no-sequence-17"])
def test_unserved_modes_have_the_single_solvers_wording(text):
    for asked in (text, solver.SolveMode.from_str(text)):
        with pytest.raises(NotImplementedError) as single:
            trails.TrailSolver(LINE, 5).find_shortest(asked)
        for call in (lambda: helpforest.HelpForestSolver([LINE, LINE], 5).run(asked), lambda: helpforest.solve_many([LINE], 5, mode=asked)):
            with pytest.raises(NotImplementedError) as many:
                call()
            assert str(many.value) == str(single.value) and f"'{asked}'" in str(many.value)
    with pytest.raises(ValueError, match="nonsense|Unknown solve mode"):
        helpforest.HelpForestSolver([LINE], 5).run("nonsense")


def test_mode_parsing_is_the_single_solvers():
    M = solver.SolveMode
    table = {"standard": (0, 2), "no-asymmetric": (1, 2), "no-mutual": (2, 2), "no-interdependence": (2, 2), "no-interdependence-2": (2, 2),
             "no-fully-coupled": (3, 2), "no-convergence": (4, 2), "no-convergence-3": (4, 3), "no-divergence-4": (5, 4), "no-sequence": (6, 2),
             "no-sequence-2": (6, 2), "no-sequence-16": (6, 16)}
    for text, want in table.items():
        mode = trails._served_mode(text)
        assert helpforest.native_mode(mode) == want, text
        if mode.kind != "no-sequence":  # the help kind's constants and parameters are HelpGraphSolver's own
            assert helpforest.native_mode(mode) == (helpgraph._NATIVE[mode.kind], mode.n or 2)
    assert trails._served_mode("no-cooperation").kind == "no-cooperation" and trails._served_mode(M.no_mutual()) == M.no_interdependence(2)


# ---------------------------------------------------------------------------------------------------------------- ManyHelpCharacterization
def hand_made(sequential=True):
    """Five worlds of three agents with known answers: 0 unsolvable, 1 independent, 2 and 3 cooperative, 4 cooperative with a plan in
    every restricted mode.  `asked` records (mode, the worlds asked for)."""
    plan = [("a",)] * 4
    plans = {"standard": [None, plan, plan, plan, plan], "no-cooperation": [None, plan[:3], None, None, None],
             "no-asymmetric": [None, None, None, plan, plan], "no-sequence-3": [None, None, plan, None, plan], "no-divergence": [None, None, None, None, plan],
             "no-interdependence": [None, None, plan, plan, plan], "no-fully-coupled": [None, None, plan, plan, plan], "no-convergence": [None] * 5}
    asked = []

    def runner(mode, only):
        asked.append((str(mode), [int(i) for i in np.flatnonzero(only)]))
        return [p if keep else None for p, keep in zip(plans[str(mode)], only)]

    return helpforest.ManyHelpCharacterization(9, [3, 3, 3, 3, 2], runner, sequential=sequential), asked


def test_many_help_characterization_over_hand_made_answers():
    many, asked = hand_made()
    assert len(many) == 5 and asked == []  # nothing runs before it is asked for
    assert many.solvable.tolist() == [False, True, True, True, True] and many.solvable.dtype == bool
    assert many.independent.tolist() == [False, True, False, False, False] and many.cooperative.tolist() == [False, False, True, True, True]
    assert asked == [("standard", [0, 1, 2, 3, 4]), ("no-cooperation", [1, 2, 3, 4])]  # the unsolvable map is not asked again
    assert many.is_asymmetric().tolist() == [False, False, True, False, False]
    assert asked[-1] == ("no-asymmetric", [2, 3, 4])  # only the cooperative maps: an independent plan avoids every shape
    assert many.is_sequential(3).tolist() == [False, False, False, True, False] and asked[-1] == ("no-sequence-3", [2, 3, 4])
    assert many.is_divergent(2).tolist() == [False, False, True, True, False]
    assert asked[-1] == ("no-divergence", [2, 3])  # map 4 has two agents: nobody helps two others
    assert many.is_divergent(3).tolist() == [False] * 5 and many.is_convergent(3).tolist() == [False] * 5  # k >= n_agents everywhere: no run at all
    assert [a[0] for a in asked].count("no-divergence-3") == 0 and "no-convergence-3" not in [a[0] for a in asked]
    assert many.is_convergent(2).tolist() == [False, False, True, True, False] and asked[-1] == ("no-convergence", [2, 3])
    assert many.is_mutual().tolist() == [False] * 5 and many.is_interdependent(2).tolist() == [False] * 5 and many.is_fully_coupled().tolist() == [False] * 5
    n = len(asked)
    many.is_asymmetric(), many.is_sequential(3), many.is_mutual(), many.solvable, many.cooperative
    assert len(asked) == n and len({a[0] for a in asked}) == n  # at most one run per mode
    for bad, word in ((lambda: many.is_sequential(1), "Sequence length must be >= 2"), (lambda: many.is_convergent(1), "at least 2 distinct helpers"),
                      (lambda: many.is_divergent(1), "at least 2 distinct beneficiaries"), (lambda: many.is_interdependent(1), ">= 2 agents")):
        with pytest.raises(ValueError, match=word):
            bad()
    with pytest.raises(NotImplementedError, match="no-interdependence-3"):
        many.is_interdependent(3)
    with pytest.raises(NotImplementedError, match="at most 16"):
        many.is_sequential(17)
    with many as same:  # a context manager; free() may be called again
        assert same is many
    many.free()


def test_entries_answer_and_short_circuit():
    many, asked = hand_made()
    e = many.entry(2)
    assert isinstance(e, lle_amd.WorldCharacterizer) and e.t_max == 9 and asked == []
    assert e.is_solvable() and asked == [("standard", [0, 1, 2, 3, 4])]
    assert e.is_cooperative() and not e.is_independent() and e.is_asymmetric() and not e.is_sequential(3) and e.is_divergent() and e.is_convergent(2)
    assert not e.is_mutual() and not e.is_interdependent(2) and not e.is_fully_coupled()
    assert len(e.shortest_path) == 4 and e.shortest_independent_path is None and len(many.entry(1).shortest_independent_path) == 3
    with pytest.raises(NotImplementedError, match="no-interdependence-3"):
        e.is_interdependent(3)
    with pytest.raises(IndexError):
        many.entry(5)
    # a constraint asks the cheapest atom first and stops when it is settled: an unbuilt or costly atom behind it never runs
    many, asked = hand_made()
    c = Constraint(9, Cooperative() & Asymmetric() & ~Sequential(3), min_solution_length=4)
    assert [c._accepts(many.entry(i)) for i in range(5)] == [False, False, True, False, False]
    assert [a[0] for a in asked] == ["standard", "no-cooperation", "no-asymmetric", "no-sequence-3"]
    many, asked = hand_made()
    assert [Constraint(9, Solvable() | Divergent(2))._accepts(many.entry(i)) for i in range(5)] == [False, True, True, True, True]
    assert [a[0] for a in asked] == ["standard", "no-cooperation", "no-divergence"]  # asked for world 0 alone, which Solvable did not settle
    assert Constraint(9, min_solution_length=5)._accepts(many.entry(2)) is False
    # under HelpGraphCharacterizer Sequential raises as it does for one world
    many, asked = hand_made(sequential=False)
    with pytest.raises(NotImplementedError, match="needs the solve mode 'no-sequence-3'"):
        Sequential(3).holds(many.entry(2))
    assert many.entry(2).is_asymmetric() is True
    with pytest.raises(NotImplementedError, match="needs the solve mode 'no-interdependence-3'"):
        Interdependent(3).holds(many.entry(2))
    assert Convergent(2).holds(many.entry(3)) is True


# ---------------------------------------------------------------------------------------------------------------- the generator
def test_satisfied_by_many_paths(monkeypatch):
    """characterizer=None still goes through forest.characterize_many; HelpGraphCharacterizer / TrailCharacterizer through
    helpforest.characterize_many; any other class through one characterizer per world."""
    calls = []
    plan = [("a",)] * 3

    def plain(worlds, t_max, **options):
        calls.append(("forest", len(worlds), t_max, options))
        return forest.ManyCharacterization(t_max, [plan, None], [None, None])

    def helped(worlds, t_max, **options):
        calls.append(("helpforest", len(worlds), t_max, options))
        many, _asked = hand_made(options.get("sequential", True))
        return many

    monkeypatch.setattr(forest, "characterize_many", plain)
    monkeypatch.setattr(helpforest, "characterize_many", helped)
    got = Constraint(7, Cooperative()).satisfied_by_many([LINE, LINE], envs_per_map=64)
    assert got.tolist() == [True, False] and got.dtype == bool and calls == [("forest", 2, 7, dict(envs_per_map=64))]
    got = Constraint(7, Cooperative()).satisfied_by_many([LINE, LINE], characterizer=None)
    assert got.tolist() == [True, False] and calls[-1] == ("forest", 2, 7, {})
    with pytest.raises(NotImplementedError, match="no-asymmetric"):  # today's path keeps today's errors
        Constraint(7, Asymmetric()).satisfied_by_many([LINE, LINE])
    five = [LINE] * 5
    got = Constraint(9, Asymmetric() & ~Sequential(3)).satisfied_by_many(five, characterizer=lle_amd.TrailCharacterizer, envs_per_map=64)
    assert got.tolist() == [False, False, True, False, False] and calls[-1] == ("helpforest", 5, 9, dict(sequential=True, envs_per_map=64))
    got = Constraint(9, Asymmetric()).satisfied_by_many(five, characterizer=lle_amd.HelpGraphCharacterizer)
    assert got.tolist() == [False, False, True, False, False] and calls[-1] == ("helpforest", 5, 9, dict(sequential=False))
    with pytest.raises(NotImplementedError, match="needs the solve mode 'no-sequence-3'"):
        Constraint(9, Cooperative() & Sequential(3)).satisfied_by_many(five, characterizer=lle_amd.HelpGraphCharacterizer)

    class Other:
        made = []

        def __init__(self, world, t_max, **solver_options):
            Other.made.append((world, t_max, solver_options))
            self.shortest_path = plan

        def is_solvable(self):
            return True

    n = len(calls)
    assert Constraint(4).satisfied_by_many(["a", "b"], characterizer=Other, chunk=8).tolist() == [True, True]
    assert Other.made == [("a", 4, dict(chunk=8)), ("b", 4, dict(chunk=8))] and len(calls) == n
    for text in ("characterizer", "TrailCharacterizer"):
        assert text in Constraint.satisfied_by_many.__doc__
    assert "characterizer=" in generator.generate_n.__doc__
    for atom in (Asymmetric, Convergent, Divergent, Sequential):
        assert "not built" not in atom.__doc__ and "satisfied_by_many" in atom.__doc__


# ---------------------------------------------------------------------------------------------------------------- the fixed input sets
def test_sets_have_the_stated_shapes():
    shapes = {"S": (4, 6, 3, 1, 0, 8, 6), "P": (5, 9, 2, 2, 0, 8, 8), "R": (6, 6, 3, 2, 0, 5, 5), "Q": (6, 6, 3, 3, 0, 2, 10), "X": (4, 8, 6, 2, 0, 2, 3),
              "G": (4, 5, 2, 2, 1, 2, 8), "L": (4, 6, 2, 2, 0, 3, 24), "C": (4, 4, 2, 2, 0, 4, 8)}
    assert set(shapes) == set(SETS)
    for name, (h, w, agents, sources, gems, count, t_max) in shapes.items():
        s = SETS[name]
        assert len(s.maps) == count == len(s.names) == len(s.changes) and s.t_max == t_max
        assert {forest.shape_key(Map(t)) for t in s.maps} == {forest.shape_key(Map(s.maps[0]))}, name
        m = Map(s.maps[0])
        assert (m.height, m.width, m.n_agents, m.n_sources, m.n_gems) == (h, w, agents, sources, gems), name
    assert SET_G.collect_gems and not SET_S.collect_gems
    assert all(s.changes == (None,) * len(s.maps) for name, s in SETS.items() if name not in "LC")
    assert SET_L.modes == (("no-sequence", 8), ("no-sequence", 15), ("no-sequence", 16), ("standard", 2)) and SET_X.modes[-2:] == (("no-sequence", 2), ("no-sequence", 3))
    assert SET_C.modes == (("standard", 2), ("no-mutual", 2), ("no-sequence", 2), ("no-sequence", 3))


def test_sets_l_and_c_differ_where_the_device_could_confuse_their_maps():
    """Set C is ONE layout four times: the texts are equal, the worlds are not, and every map has its own (length, records) under
    no-sequence-2 -- a forest that reads another map's edge rule gives another map's answer.  Set L's first two maps are one layout too,
    and its third is another one: a wrong cell-table offset reads other tiles."""
    assert len(set(SET_C.maps)) == 1 and SET_C.changes == (None, helpforest_ref.OFF1, helpforest_ref.OFF0, helpforest_ref.RECOLOUR1)
    assert SET_C.names == ("two-agent-mutual-compact", "two-agent-mutual-compact-source1-off", "two-agent-mutual-compact-source0-off",
                           "two-agent-mutual-compact-source1-colour0")
    rows = GOLDEN["C"]["no-sequence/2"]
    assert [(r["length"], r["states"]) for r in rows] == [(None, 100), (5, 164), (5, 130), (None, 107)] and GOLDEN["C"]["no-mutual/2"] == rows
    assert [(r["length"], r["states"]) for r in GOLDEN["C"]["no-sequence/3"]] == [(5, 119), (5, 164), (5, 130), (None, 107)]
    for key in GOLDEN["C"]:
        assert len({(r["length"], r["states"]) for r in GOLDEN["C"][key]}) == 4, key
    # the worlds the device is given: the sources as the changes leave them
    worlds = SET_C.worlds
    assert worlds[0] == SET_C.maps[0] and all(isinstance(w, World) for w in worlds[1:])
    assert [[(s.is_enabled, s.agent_id) for s in sorted(w.laser_sources, key=lambda s: s.laser_id)] for w in worlds[1:]] == \
        [[(True, 0), (False, 1)], [(False, 0), (True, 1)], [(True, 0), (True, 0)]]
    assert SET_L.maps[0] == SET_L.maps[1] != SET_L.maps[2] and SET_L.changes == (None, helpforest_ref.OFF1, None)
    for n in (8, 15, 16):
        first, second, third = GOLDEN["L"][f"no-sequence/{n}"]
        assert (first["length"], first["states"], len(first["expanded"]), first["frontier"][-1]) == (None, 100 + 76 * (n - 2), n + 5, 0)
        assert (second["length"], second["states"], len(second["expanded"])) == (None, 198, 8)
        assert (third["length"], third["states"], len(third["expanded"])) == (5, 126, 5)  # solved at depth 5 while the first map walks N + 5 levels
    assert [(r["length"], r["states"]) for r in GOLDEN["L"]["standard/2"]] == [(None, 203), (None, 198), (5, 123)]
    # the embedding gives the small layout's counters: set L's third map is set C's first at every depth both walk, set P's first too
    for key in ("standard/2",):
        assert GOLDEN["L"][key][2] == GOLDEN["C"][key][0] == GOLDEN["P"][key][0]
    assert GOLDEN["C"]["no-sequence/3"][0] == GOLDEN["P"]["no-sequence/3"][0] and GOLDEN["C"]["no-sequence/2"][0] == GOLDEN["P"]["no-sequence/2"][0]
    # six agents under no-sequence-3: the single solver's recorded searches, in a frame of walls
    from tests import trails_ref
    single = {(c["map"], c["n"]): c for c in trails_ref.load_cases()["searches"] if "changes" not in c}
    for m, name in enumerate(SET_X.names):
        row, want = GOLDEN["X"]["no-sequence/3"][m], single[(name, 3)]
        assert (row["length"], row["states"], row["frontier"], row["expanded"]) == (want["length"], want["states"], want["frontier"], want["expanded"])


def test_golden_file_holds_what_the_issue_states():
    assert set(GOLDEN) == set(SETS)
    for name, s in SETS.items():
        assert set(GOLDEN[name]) == {helpforest_ref.golden_key(*mp) for mp in s.modes} and all(len(rows) == len(s.maps) for rows in GOLDEN[name].values())
    for s, stated in ((SET_S, helpforest_ref.S_STATED), (SET_P, helpforest_ref.P_STATED)):
        for (mode, param), pairs in stated.items():
            rows = GOLDEN[s.name][helpforest_ref.golden_key(mode, param)]
            assert [(rows[m]["length"], rows[m]["states"]) for m in (0, 1)] == list(pairs), (s.name, mode, param)
    standard, asym = GOLDEN["S"]["standard/2"], GOLDEN["S"]["no-asymmetric/2"]
    assert sum(r["length"] is None for r in standard) == 2  # two generated maps have no plan at all
    assert [(standard[m]["length"], standard[m]["states"], asym[m]["length"], asym[m]["states"]) for m in range(2, 8)].count((4, 576, None, 1641)) == 1
    assert GOLDEN["P"]["no-mutual/2"] == GOLDEN["P"]["no-sequence/2"]  # two agents: a mutual pair is a trail of two edges and the other way round
    at_reset = SET_R.names.index("chain-at-reset")
    assert GOLDEN["R"]["no-sequence/2"][at_reset] == dict(length=None, frontier=[1], expanded=[], states=1)  # the reset state holds the trail already
    assert all(r["states"] < 8000 for r in GOLDEN["Q"]["no-fully-coupled/2"])
    assert any(r["states"] > 256 for r in asym) and any(r["states"] <= 256 for r in asym)  # capacity isolation has both kinds of map


@pytest.mark.parametrize("name, m", [("S", 0), ("S", 1), ("P", 0), ("R", 3), ("R", 2), ("G", 0), ("G", 1), ("L", 0), ("L", 1), ("L", 2), ("C", 0), ("C", 1), ("C", 2),
                                     ("C", 3)])
def test_the_restatements_still_give_the_golden_file(name, m):
    """A subset (the whole file takes minutes): every mode of seven maps, the catalogue maps of S and P among them, and every map of
    L and C under its changes."""
    s = SETS[name]
    for mode, param in s.modes:
        r = helpforest_ref.search(s.maps[m], s.t_max, mode, param, s.collect_gems, changes=s.changes[m])
        got = dict(length=r.length, frontier=list(r.frontier), expanded=list(r.expanded), states=r.n_states)
        assert got == GOLDEN[name][helpforest_ref.golden_key(mode, param)][m], (name, m, mode, param)


@pytest.mark.parametrize("name, m, size, mode, param", [("L", 2, (20, 20), "standard", 2), ("L", 2, (6, 255), "no-sequence", 16), ("R", 3, (255, 6), "no-sequence", 3),
                                                        ("R", 3, (20, 20), "no-convergence", 2)], ids=str)
def test_a_layout_in_either_corner_is_the_same_world(name, m, size, mode, param):
    """What the far-corner tests of tests/test_gpu_helpforest_edges.py lean on: a set's map in the top-left corner (`embed_top_left`) or in
    the bottom-right corner (`helpgraph_ref.embed`) of a big map of walls has the counters recorded for the small one."""
    from tests import helpgraph_ref
    s, want = SETS[name], GOLDEN[name][helpforest_ref.golden_key(mode, param)][m]
    for text in (helpforest_ref.embed_top_left(helpforest_ref.MAPS[s.names[m]], *size), helpgraph_ref.embed(s.maps[m], *size)):
        r = helpforest_ref.search(text, s.t_max, mode, param, changes=s.changes[m])
        assert dict(length=r.length, frontier=list(r.frontier), expanded=list(r.expanded), states=r.n_states) == want


@pytest.mark.parametrize("m", [0, 1])
def test_the_restatement_gives_set_x_under_no_sequence_3(m):
    """Six agents, trails of two edges stored: the one mode of set X added after the file was first made (its other modes take a minute)."""
    r = helpforest_ref.search(SET_X.maps[m], SET_X.t_max, "no-sequence", 3)
    assert dict(length=r.length, frontier=list(r.frontier), expanded=list(r.expanded), states=r.n_states) == GOLDEN["X"]["no-sequence/3"][m]
    assert r.trails[5] > 0 and max(r.trails) == 2  # the sixth field, bits 20-23, under an N that stores trails of two edges


# ---------------------------------------------------------------------------------------------------------------- helpforest_logic.hpp
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_piece_logic_under_sanitizers(tmp_path):
    """tests/hostsim/helpforest_pieces.cpp: its own main over helpforest_logic.hpp, built with g++ -fsanitize=address,undefined and run
    as a child process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "helpforest_pieces")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "helpforest_pieces.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["lanes"]) > 5000 and int(out["records"]) > 100
        assert int(out["tag_matches"]) > 100 and int(out["pool_matches"]) > 100  # duplicates met inside a piece and across pieces
