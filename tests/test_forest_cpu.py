"""The forest search without a GPU: header / exports / binding of liblle_forest.so, every host-side refusal, ForestSolver's argument
errors, the predicate algebra and generate_n's argument errors of lle_amd.generator, the fixed input sets against the figures their
oracle is known to give, and lle_amd/forest/forest_logic.hpp under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone
program (tests/hostsim/forest_pieces.cpp).  The search itself runs on the MI355X (tests/test_gpu_forest.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, characterization, forest, generator, solver
from lle_amd.generator import (And, Asymmetric, Constraint, Convergent, Cooperative, Divergent, Independent, Interdependent, Not, Or, Predicate, Sequential,
                               Solvable, WorldRequirements)
from tests import forest_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
KERNELS = ["forest_commit", "forest_expand", "forest_insert<false>", "forest_insert<true>", "forest_plans", "forest_roots", "forest_seed"]


def handles(maps):
    return (C.c_void_p * len(maps))(*[m.h for m in maps])


def options(envs_per_map=0, max_states_per_map=0, struct_bytes=None, device=-1):
    return forest.ForestOptions(C.sizeof(forest.ForestOptions) if struct_bytes is None else struct_bytes, device, envs_per_map, max_states_per_map, None)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_exports():
    """liblle_forest.so exports every function include/lle_forest.h declares, and the binding knows exactly those; the header is plain
    C and the one the library is compiled against; struct sizes of the binding are the header's; the library adds nothing to
    liblle_search.so."""
    L = forest.lib()
    header = open(os.path.join(ROOT, "include", "lle_forest.h")).read()
    declared = set(re.findall(r"\b(lle_forest_[a-z_0-9]+)\s*\(", header))
    assert declared == set(forest.EXPORTS) and len(forest.EXPORTS) == 9
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "forest", "forest.hip")).read()
    assert '#include "../../include/lle_forest.h"' in source and '#include "forest_logic.hpp"' in source
    assert '#include "../search/search_logic.hpp"' in open(os.path.join(ROOT, "lle_amd", "forest", "forest_logic.hpp")).read()
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    assert "lle_search_create" not in source and "lle_search_run" not in source.replace("lle_search_run's", "")  # no symbol of liblle_search.so
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "lle_forest.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu", sizeof(lle_forest_options), '
            'sizeof(lle_forest_result), offsetof(lle_forest_options, max_states_per_map), offsetof(lle_forest_options, stream), '
            'offsetof(lle_forest_result, n_states), offsetof(lle_forest_result, depth_reached)); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(forest.ForestOptions), C.sizeof(forest.ForestMapResult), forest.ForestOptions.max_states_per_map.offset,
                   forest.ForestOptions.stream.offset, forest.ForestMapResult.n_states.offset, forest.ForestMapResult.depth_reached.offset]
    assert sorted(forest.compiled_kernels()) == KERNELS == sorted(forest.KERNELS)
    assert forest.launched_kernels() == []


def test_build_knows_the_library():
    from lle_amd import build
    assert '("forest", "liblle_forest.so")' in open(build.__file__).read()
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "forest.EXPORTS" in entry and "liblle_forest.so does not export" in entry
    assert os.path.exists(forest.LIB_PATH)


def test_lazy_names():
    assert lle_amd.ForestSolver is forest.ForestSolver and lle_amd.ForestResult is forest.ForestResult
    assert lle_amd.solve_many is forest.solve_many and lle_amd.characterize_many is forest.characterize_many
    for name in generator.__all__:
        assert getattr(lle_amd, name) is getattr(generator, name)
    assert lle_amd.WorldFilter is lle_amd.Constraint
    assert {"ForestSolver", "solve_many", "characterize_many", "Constraint", "generate_n"} <= set(lle_amd.__all__)
    assert "out of scope" in generator.generate_n.__doc__ and "placement strategies" in generator.generate_n.__doc__


def test_host_side_refusals():
    L = forest.lib()
    line, other = Map(LINE), Map("S0 . X .")

    def refused(maps, n, opt, word):
        got = L.lle_forest_create(maps, n, None if opt is None else C.byref(opt))
        message = L.lle_forest_last_error()
        assert got is None and word in message, (word, message)

    two = handles([line, other])
    refused(None, 1, None, b"NULL maps")
    refused(two, 0, None, b"n_maps must be at least 1")
    refused(two, -3, None, b"n_maps must be at least 1")
    refused((C.c_void_p * 2)(line.h, None), 2, None, b"NULL map (entry 1)")
    refused(two, 2, options(struct_bytes=4), b"struct_bytes")
    refused(two, 2, options(struct_bytes=C.sizeof(forest.ForestOptions) + 8), b"struct_bytes")
    for E, cap, word in ((-1, 0, b"envs_per_map must be"), ((1 << 30) + 1, 0, b"envs_per_map must be"), (0, -1, b"max_states_per_map"),
                         (0, (1 << 30) + 1, b"max_states_per_map"), (0, 1 << 31, b"max_states_per_map"), (1 << 30, 0, b"n_maps * envs_per_map")):
        refused(two, 2, options(E, cap), word)
    refused(handles([line]), 1, options(1 << 30, 1 << 30), b"must be below 2^31")
    # the step library's own refusal, with its message: a map of another width, another number of sources, another row alignment
    # (the Maps are named: an array of handles does not keep them alive)
    narrow, laser, no_laser, aligned, seven = Map("S0 . X"), Map("S0 . X .\nL0E . . ."), Map("S0 . X .\n. . . ."), Map(LINE, row_align=256), Map(SEVEN)
    refused(handles([line, narrow]), 2, None, b"lle_batch_create_multi: the maps of a batch must agree on height, width")
    refused(handles([laser, no_laser]), 2, None, b"lle_batch_create_multi: the maps of a batch must agree")
    refused(handles([line, aligned]), 2, None, b"row alignment")
    refused(handles([seven]), 1, None, b"more than 6 agents")
    # nothing wrong with the arguments: where they are refused all the same, what is missing is the device
    for maps, n, opt in ((two, 2, None), (two, 2, options(1, 1)), (handles([line]), 1, options(7, 128))):
        got = L.lle_forest_create(maps, n, None if opt is None else C.byref(opt))
        assert got is not None or b"no HIP device" in L.lle_forest_last_error(), L.lle_forest_last_error()
        L.lle_forest_free(got)
    args, res = solver.SearchArgs(C.sizeof(solver.SearchArgs), 0, 0, 3), (forest.ForestMapResult * 2)()
    assert L.lle_forest_run(None, C.byref(args), res) == -1 and b"NULL" in L.lle_forest_last_error()
    assert L.lle_forest_plan(None, 0, None, 0) == -1
    assert L.lle_forest_stats(None, 0, None, None, 0) == -1
    assert L.lle_forest_occupancy(None, None, None) == -1
    L.lle_forest_free(None)


# ---------------------------------------------------------------------------------------------------------------- ForestSolver
def test_forest_solver_forms_and_freezing():
    w = World("S0 . X X")
    f = forest.ForestSolver([w, Map(LINE), "S0 X . ."], 7, envs_per_map=3, max_states_per_map=5)
    assert f.worlds[0] is w and all(isinstance(x, World) for x in f.worlds)
    assert (f.t_max, f.envs_per_map, f.max_states_per_map, f.n_maps, f.n_agents, f.h) == (7, 3, 5, 3, 1, None)
    w.exit_pos = [(0, 3)]  # frozen at construction, like Solver
    assert f._maps[0].positions(1) == [(0, 2), (0, 3)] and w._map.positions(1) == [(0, 3)]
    assert forest.ForestSolver([LINE]).t_max == 2 and forest.ForestSolver([LINE, LINE], "auto").envs_per_map == 256
    assert forest.ForestSolver([LINE]).max_states_per_map == 1 << 16


def test_forest_solver_argument_errors():
    with pytest.raises(ValueError, match="at least one world"):
        forest.ForestSolver([], 5)
    with pytest.raises(ValueError, match="non-negative"):
        forest.ForestSolver([LINE], -1)
    with pytest.raises(ValueError, match="at least 1"):
        forest.ForestSolver([LINE], 5, envs_per_map=0)
    with pytest.raises(ValueError, match="at least 1"):
        forest.ForestSolver([LINE], 5, max_states_per_map=0)
    with pytest.raises(ValueError, match="nonsense|Unknown solve mode"):
        forest.ForestSolver([LINE], 5).run("nonsense")


@pytest.mark.parametrize("other, what", [
    ("S0 . X", r"width \(3, map 0 has 4\)"),
    ("S0 . . X\n. . . .", r"height \(2, map 0 has 1\)"),
    ("S0 S1 X X", r"number of agents \(2, map 0 has 1\)"),
    ("S0 G . X", r"number of gems \(1, map 0 has 0\)"),
])
def test_shape_mismatches_name_the_map(other, what):
    with pytest.raises(ValueError, match=r"map 2 does not match map 0 in " + what):
        forest.ForestSolver([LINE, LINE, other, "S0 X"], 5)


def test_shape_mismatches_of_sources_beam_words_and_alignment():
    base = "S0 . X .\nL0E . . ."
    with pytest.raises(ValueError, match=r"map 1 does not match map 0 in number of laser sources \(0, map 0 has 1\)"):
        forest.ForestSolver([base, "S0 . X .\n. . . ."], 5)
    long_beam = "L0E" + " ." * 39 + "\nS0 X" + " ." * 38
    short_beam = "L0E . . @" + " ." * 36 + "\nS0 X" + " ." * 38
    with pytest.raises(ValueError, match=r"map 1 does not match map 0 in layout of the beam words"):
        forest.ForestSolver([long_beam, short_beam], 5)
    with pytest.raises(ValueError, match=r"map 1 does not match map 0 in row alignment"):
        forest.ForestSolver([Map(LINE), Map(LINE, row_align=256)], 5)
    with pytest.raises(ValueError, match=r"map 3 does not match map 0 in height \(5, map 0 has 4\)"):
        forest.ForestSolver(list(forest_ref.SET_A.maps[:3]) + [forest_ref.SET_B.maps[0]], 10)
    assert len({forest.shape_key(Map(t)) for t in forest_ref.SET_A.maps}) == 1
    keys = [forest.shape_key(Map(s.maps[0])) for s in forest_ref.SETS.values()]
    assert len(set(keys)) == 3


def test_seven_agents_are_refused():
    with pytest.raises(ValueError, match="at most 6 agents"):
        forest.ForestSolver([SEVEN], 4)
    with pytest.raises(ValueError, match="at most 6 agents"):
        forest.solve_many([SEVEN, SEVEN], 4)
    assert forest.ForestSolver([" ".join(f"S{k}" for k in range(6)) + " X" * 6], 4).n_agents == 6


@pytest.mark.parametrize("text", ["no-asymmetric", "no-mutual", "no-fully-coupled", "no-sequence-2", "no-sequence-3", "no-interdependence-3", "no-convergence",
                                  "no-divergence-4"])
def test_mode_wording_is_the_solvers(text):
    for asked in (text, solver.SolveMode.from_str(text)):
        with pytest.raises(NotImplementedError) as single:
            solver.Solver(LINE, 5).find_shortest(asked)
        for call in (lambda: forest.ForestSolver([LINE, LINE], 5).run(asked), lambda: forest.solve_many([LINE], 5, mode=asked)):
            with pytest.raises(NotImplementedError) as many:
                call()
            assert str(many.value) == str(single.value) and f"'{asked}'" in str(many.value)


# ---------------------------------------------------------------------------------------------------------------- the predicate algebra
def test_operators_and_flattening():
    s, i, c = Solvable(), Independent(), Cooperative()
    assert (s & i) == And(s, i) and (s | i) == Or(s, i) and ~s == Not(s)
    assert s.and_(i) == s & i and s.or_(i) == s | i and s.not_() == ~s and s.and_not(c) == And(s, Not(c))
    assert ((s & i) & c).children == (s, i, c) == (s & (i & c)).children == And(And(s), And(i, And(c))).children
    assert ((s | i) | c).children == (s, i, c) == Or(Or(s, i), c).children
    assert ((s | i) & c).children == (Or(s, i), c) and ((s & i) | c).children == (And(s, i), c)  # only the same kind is flattened
    assert Not(Not(s)).inner == Not(s)
    assert And().children == () and Or().children == ()
    assert hash(s & i) == hash(And(s, i)) and {s & i, And(s, i)} == {And(s, i)} and Sequential(3) != Sequential(2) and Divergent() == Divergent(2)
    for bad in (lambda: And(s, 3), lambda: Or("x"), lambda: Not(None), lambda: s & 1, lambda: Constraint(5, "cooperative")):
        with pytest.raises(TypeError, match="Expected Predicate"):
            bad()
    with pytest.raises(Exception):
        s.anything = 1  # value objects
    with pytest.raises(Exception):
        (s & i).children = ()


def test_costs_and_the_order_of_evaluation():
    assert [p.cost for p in (Solvable(), Independent(), Cooperative(), Asymmetric(), Sequential(), Sequential(4), Convergent(2), Convergent(3), Divergent(),
                             Divergent(5), Interdependent(), Interdependent(3))] == [0, 1, 2, 3, 12, 14, 22, 23, 22, 25, 22, 23]
    assert (Cooperative() & Independent()).cost == 3 and (Cooperative() | Sequential(3)).cost == 15 and (~Sequential(3)).cost == 13
    assert And(Sequential(3), Cooperative(), Solvable(), Independent()).ordered() == (Solvable(), Independent(), Cooperative(), Sequential(3))
    assert Or(Convergent(2), Divergent(2), Asymmetric()).ordered() == (Asymmetric(), Convergent(2), Divergent(2))  # ties keep their order

    class Probe:
        def __init__(self, **answers):
            self.answers, self.asked = answers, []

        def __getattr__(self, name):
            def ask(*_args):
                self.asked.append(name)
                return self.answers[name]
            return ask

    p = Probe(is_solvable=True, is_independent=False, is_cooperative=True)
    assert And(Cooperative(), Independent(), Solvable()).holds(p) is False and p.asked == ["is_solvable", "is_independent"]  # cheapest first, then stop
    p = Probe(is_solvable=False, is_independent=False, is_cooperative=True)
    assert Or(Cooperative(), Independent(), Solvable()).holds(p) is True and p.asked == ["is_solvable", "is_independent", "is_cooperative"]
    p = Probe(is_cooperative=False, is_solvable=True)
    assert (~Cooperative() & Solvable()).holds(p) is True and p.asked == ["is_solvable", "is_cooperative"]
    assert And().holds(p) is True and Or().holds(p) is False
    p = Probe(is_cooperative=True)  # a cheap child that settles the answer keeps the unbuilt one from being asked
    assert Or(Sequential(3), Cooperative()).holds(p) is True and p.asked == ["is_cooperative"]


def test_requirements():
    R = WorldRequirements
    assert Solvable().requirements == R() == R(0, 1) == Independent().requirements
    assert Cooperative().requirements == R(1, 2) == Asymmetric().requirements
    assert Sequential(4).requirements == R(4, 2) and Convergent(3).requirements == R(3, 4) and Divergent(3).requirements == R(1, 4)
    assert Interdependent(3).requirements == R(3, 3)
    assert (Cooperative() & Convergent(3) & Solvable()).requirements == R(3, 4)       # And: the largest of each
    assert (Cooperative() | Convergent(3)).requirements == R(1, 2)                    # Or: the smallest of each
    assert (Cooperative() | Solvable()).requirements == R()
    assert (~Convergent(3)).requirements == R()                                       # Not: nothing is required
    assert (Cooperative() & ~Convergent(3)).requirements == R(1, 2)
    assert And().requirements == R() == Or().requirements and R.all([]) == R() == R.any([])
    assert R.all([R(2, 1), R(0, 5)]) == R(2, 5) and R.any([R(2, 1), R(0, 5)]) == R(0, 1)
    assert Constraint(10, Cooperative() & Sequential(3)).requirements == R(3, 2) and Constraint(10).requirements == R()
    for bad in (lambda: R(-1, 1), lambda: R(0, 0)):
        with pytest.raises(ValueError):
            bad()


def test_argument_checks_of_the_atoms():
    for bad, word in ((lambda: Sequential(1), "Sequence length must be >= 2, got 1"), (lambda: Convergent(1), "at least 2 distinct helpers, got 1"),
                      (lambda: Divergent(0), "at least 2 distinct beneficiaries, got 0"), (lambda: Interdependent(1), "Dependency order must be >= 2, got 1")):
        with pytest.raises(ValueError, match=word):
            bad()
    with pytest.raises(TypeError):
        Convergent()  # k has no default, as in the reference
    assert Sequential().length == 2 and Divergent().k == 2 and Interdependent().order == 2


def test_unbuilt_atoms_raise_the_characterizers_error():
    c = characterization.WorldCharacterizer(World("S0 L1S X\n. . .\n. . X\nS1 . L0N"), 6)
    for predicate, mode in ((Asymmetric(), "no-asymmetric"), (Sequential(), "no-sequence-2"), (Sequential(3), "no-sequence-3"), (Convergent(2), "no-convergence-2"),
                            (Divergent(4), "no-divergence-4"), (Interdependent(3), "no-interdependence-3")):
        with pytest.raises(NotImplementedError, match=f"needs the solve mode '{mode}'"):
            predicate.holds(c)
        with pytest.raises(NotImplementedError, match=mode):
            (~predicate).holds(c)
    # ... and behind the answers of a forest as well
    many = forest.ManyCharacterization(6, [None, [()]], [None, None])
    row = generator._Answered(many, 1)
    assert row.is_solvable() and row.is_cooperative() and not row.is_independent() and not generator._Answered(many, 0).is_cooperative()
    with pytest.raises(NotImplementedError, match="needs the solve mode 'no-sequence-3'"):
        Sequential(3).holds(row)


def test_constraint_over_given_answers():
    """Constraint._accepts on answers that need no search: what satisfied_by_many does per entry."""
    plan = [("a",)] * 5
    many = forest.ManyCharacterization(10, [plan, plan, None, plan[:2]], [plan, None, None, plan[:2]])
    assert list(many.solvable) == [True, True, False, True] and list(many.cooperative) == [False, True, False, False]
    assert list(many.independent) == [True, False, False, True] and list(many.shortest_length) == [5, 5, -1, 2]
    assert list(many.shortest_independent_length) == [5, -1, -1, 2] and len(many) == 4

    def accepts(constraint):
        return [constraint._accepts(generator._Answered(many, i)) for i in range(4)]

    assert accepts(Constraint(10)) == [True, True, False, True]
    assert accepts(Constraint(10, Cooperative())) == [False, True, False, False]
    assert accepts(Constraint(10, ~Cooperative())) == [True, False, True, True]  # (an unsolvable world is not cooperative)
    assert accepts(Constraint(10, ~Cooperative() & Solvable())) == [True, False, False, True]
    assert accepts(Constraint(10, ~Cooperative(), min_solution_length=3)) == [True, False, False, False]
    assert accepts(Constraint(10, Independent() | Cooperative(), min_solution_length=6)) == [False] * 4
    assert lle_amd.WorldFilter(10, Independent()).t_max == 10 and Constraint(3).predicate == Solvable() and Constraint(3).min_solution_length is None
    with pytest.raises(ValueError, match="non-negative"):
        Constraint(-1)


def test_generate_n_argument_errors():
    shape = dict(height=4, width=5, n_agents=2, n_lasers=1)
    for bad, error, word in (
            (lambda: generator.generate_n(3, Cooperative(), **shape), TypeError, "Expected Constraint"),
            (lambda: generator.generate_n(-1, Constraint(10), **shape), ValueError, "n must be non-negative"),
            (lambda: generator.generate_n(3, Constraint(10), batch=0, **shape), ValueError, "batch must be at least 1"),
            (lambda: generator.generate_n(3, Constraint(10), max_attempts=-1, **shape), ValueError, "max_attempts must be non-negative"),
            (lambda: generator.generate_n(3, Constraint(10, Cooperative()), height=4, width=5, n_agents=1, n_lasers=1), ValueError, "at least 2 agents, got n_agents=1"),
            (lambda: generator.generate_n(3, Constraint(10, Cooperative()), height=4, width=5, n_agents=2), ValueError, "at least 1 lasers, got n_lasers=0"),
            (lambda: generator.generate_n(3, Constraint(10, Convergent(3)), height=4, width=5, n_agents=3, n_lasers=3), ValueError, "at least 4 agents")):
        with pytest.raises(error, match=word):
            bad()  # (refused by the call itself, before the first candidate is drawn)
    with pytest.raises(TypeError):
        generator.generate_n(3, Constraint(10))  # height, width and n_agents have no default
    assert list(generator.generate_n(0, Constraint(10), **shape)) == []                 # nothing asked: no candidate, no device
    assert list(generator.generate_n(5, Constraint(10), max_attempts=0, **shape)) == []


# ---------------------------------------------------------------------------------------------------------------- the fixed input sets
def test_set_a_is_what_the_issue_states():
    A = forest_ref.SET_A
    standard = forest_ref.oracle(A.maps, A.t_max, "standard")
    alone = forest_ref.oracle(A.maps, A.t_max, "no-cooperation")
    assert [r.length for r in standard] == forest_ref.A_STANDARD_LENGTHS
    assert sorted({r.length for r in standard} - {None}) == [1, 2, 3, 4, 5, 6, 7, 9]  # maps stop at many different depths of one run
    assert [len(standard[s].expanded) for s in (8, 13)] == [10, 9] and [standard[s].frontier[-1] for s in (8, 13)] == [0, 0]  # run empty
    assert [s for s in range(16) if standard[s].length is not None and alone[s].length is None] == forest_ref.A_COOPERATIVE_SEEDS
    assert [s for s in range(16) if standard[s].n_states > 128] == forest_ref.A_OVER_128_STATES
    assert len(A.maps) == 16 and len(forest_ref.SET_B.maps) == 16 and len(forest_ref.SET_C.maps) == 6
    assert Map(forest_ref.SET_C.maps[0]).n_agents == 3 and (forest_ref.SET_B.t_max, forest_ref.SET_C.t_max) == (12, 8)


# ---------------------------------------------------------------------------------------------------------------- forest_logic.hpp
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_piece_logic_under_sanitizers(tmp_path):
    """tests/hostsim/forest_pieces.cpp: its own main over forest_logic.hpp, built with g++ -fsanitize=address,undefined and run as a child
    process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "forest_pieces")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "forest_pieces.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["levels"]) == 96 and int(out["served"]) > 10000 and int(out["lanes"]) > int(out["served"])
