"""The solver without a GPU: header / exports / binding of liblle_search.so, the lower bound, every argument error and refusal, the solve
modes, and the table code and the record I/O of lle_amd/search/search_logic.hpp under AddressSanitizer + UndefinedBehaviorSanitizer in
stand-alone programs (tests/hostsim/search_table.cpp, tests/hostsim/record_io.cpp).  The search itself runs on the MI355X
(tests/test_gpu_solver.py)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, characterization, solver
from tests import search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = search_ref.load_cases()
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7


def test_kat_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location("make_kat_solver", os.path.join(ROOT, "tests", "golden", "make_kat_solver.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CATALOGUE == CASES["catalogue"] and mod.SOLVER_CASES == CASES["solver"] and mod.LOWER_BOUNDS == CASES["lower_bounds"]
    every = CASES["catalogue"] + CASES["lower_bounds"] + [c for group in CASES["solver"].values() for c in group]
    assert all(c["ref"].startswith(("python/tests/", "src/unit_tests/")) for c in every)
    for c in CASES["catalogue"]:
        assert c["expect"] and all(set(e) <= {"solvable", "cooperative", "independent"} for e in c["expect"].values())
        assert all(e["cooperative"] is not e["independent"] for e in c["expect"].values() if "cooperative" in e)


def test_library_exports():
    """liblle_search.so exports every function include/lle_search.h declares, and the binding knows exactly those; the header is plain
    C and the one the library is compiled against; struct sizes and enum values of the binding are the header's."""
    L = solver.lib()
    header = open(os.path.join(ROOT, "include", "lle_search.h")).read()
    declared = set(re.findall(r"\b(lle_search_[a-z_0-9]+)\s*\(", header))
    assert declared == set(solver.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "search", "search.hip")).read()
    assert '#include "../../include/lle_search.h"' in source and '#include "search_logic.hpp"' in source
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    prog = ('#include <stdio.h>\n#include "lle_search.h"\nint main(void) { printf("%zu %zu %zu %d %d %d %d", sizeof(lle_search_options), '
            'sizeof(lle_search_args), sizeof(lle_search_result), LLE_SEARCH_CAPACITY, LLE_SEARCH_STANDARD, LLE_SEARCH_NO_COOPERATION, '
            'LLE_SEARCH_MAX_AGENTS); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(solver.SearchOptions), C.sizeof(solver.SearchArgs), C.sizeof(solver.SearchResult), solver.LLE_SEARCH_CAPACITY,
                   solver.LLE_SEARCH_STANDARD, solver.LLE_SEARCH_NO_COOPERATION, solver.LLE_SEARCH_MAX_AGENTS]
    assert sorted(solver.compiled_kernels()) == ["search_commit", "search_expand", "search_insert<false>", "search_insert<true>"]
    assert solver.launched_kernels() == []


def test_lazy_names():
    assert lle_amd.Solver is solver.Solver and lle_amd.solve is solver.solve and lle_amd.SolveMode is solver.SolveMode
    assert lle_amd.WorldCharacterizer is characterization.WorldCharacterizer
    assert issubclass(lle_amd.SolverCapacityError, RuntimeError)
    assert {"Solver", "solve", "SolveMode", "WorldCharacterizer"} <= set(lle_amd.__all__)
    assert "out of scope" not in characterization.__doc__.split("WorldCharacterizer")[0]


@pytest.mark.parametrize("case", CASES["lower_bounds"], ids=[c["name"] for c in CASES["lower_bounds"]])
def test_lower_bounds_of_the_reference(case):
    assert solver.lower_bound(Map(case["map"])) == case["bound"]
    assert solver.Solver(case["map"], 20).solution_lower_bound == case["bound"]


def test_lower_bounds_of_the_levels_and_the_rules():
    for level in (1, 2, 3, 4):
        assert solver.lower_bound(Map(level=level)) == 10
        assert solver.Solver(World.level(level), 10).solution_lower_bound == 10
    assert solver.lower_bound(Map("S0 @ X")) == 0            # an agent with no reachable exit counts 0
    assert solver.lower_bound(Map("S0 X . X")) == 1           # the nearest exit
    assert solver.lower_bound(Map("S0 X . S1 X")) == 1        # the maximum over agents
    assert solver.lower_bound(Map("S0 . X S1 . . X")) == 2    # (a path to the nearest exit never runs through another exit)
    assert solver.lower_bound(Map("S0 V X\n. . .")) == 4      # voids are not walkable
    assert solver.lower_bound(Map("S0 L0S X\n. . .")) == 4    # nor are sources; beams are
    assert solver.lower_bound(Map("S0 . X\nL0N . .")) == 2


def test_t_max_and_world_forms():
    assert solver.Solver(LINE).t_max == 2 and solver.Solver("S0 .\n.  X").t_max == 2 and solver.Solver(Map(level=6)).t_max == 78
    w = World(LINE)
    s = solver.Solver(w, 7, chunk=3, max_states=5)
    assert s.world is w and s.t_max == 7 and (s.chunk, s.max_states) == (3, 5) and s.last_stats is None
    assert isinstance(solver.Solver(Map(LINE), 3).world, World) and isinstance(solver.Solver(LINE, 3).world, World)


def test_argument_errors():
    s = solver.Solver(LINE, 5)
    for case in CASES["solver"]["value_errors"]:
        s = solver.Solver(case["map"], case["t_max"])
        with pytest.raises(ValueError, match=case["match"]):
            s.find_shortest(t_min=case["t_min"]) if case["call"] == "find_shortest" else s.solve(case["path_length"])
    with pytest.raises(ValueError, match="exceeds this solver's t_max"):
        s.find_shortest(t_min=6)
    with pytest.raises(ValueError, match="exceeds this solver's t_max=5"):
        s.solve(6)
    with pytest.raises(ValueError, match="non-negative"):
        s.solve(-1)
    with pytest.raises(ValueError, match="exceeds"):
        solver.solve(LINE, 5, path_length=6)
    assert s.solve(2) is None and s.solve(0) is None  # below the lower bound: no search, no device
    assert solver.Solver("S0 . . . . X", 3).find_shortest() is None  # the lower bound exceeds t_max: no length to try
    with pytest.raises(ValueError):
        solver.Solver(LINE, -1)
    with pytest.raises(ValueError):
        solver.Solver(LINE, 5, chunk=0)
    with pytest.raises(ValueError):
        solver.Solver(LINE, 5, max_states=0)


def test_seven_agents_are_refused():
    with pytest.raises(ValueError, match="at most 6 agents"):
        solver.Solver(SEVEN, 4)
    with pytest.raises(ValueError, match="at most 6 agents"):
        characterization.WorldCharacterizer(World(SEVEN), 4)
    L, seven = solver.lib(), Map(SEVEN)
    assert L.lle_search_create(seven.h, None) is None and b"more than 6 agents" in L.lle_search_last_error()
    assert solver.Solver(" ".join(f"S{k}" for k in range(6)) + " X" * 6, 4).world.n_agents == 6


def test_host_side_refusals():
    L, line = solver.lib(), Map(LINE)
    assert L.lle_search_create(None, None) is None and b"NULL" in L.lle_search_last_error()
    bad = solver.SearchOptions(4, -1, 0, 0, None)
    assert L.lle_search_create(line.h, C.byref(bad)) is None and b"struct_bytes" in L.lle_search_last_error()
    for chunk, max_states, word in ((-1, 0, b"chunk"), ((1 << 30) + 1, 0, b"chunk"), (0, -1, b"max_states"), (0, 1 << 31, b"max_states"), (0, (1 << 30) + 1, b"max_states")):
        opt = solver.SearchOptions(C.sizeof(solver.SearchOptions), -1, chunk, max_states, None)
        assert L.lle_search_create(line.h, C.byref(opt)) is None and word in L.lle_search_last_error()
    assert L.lle_search_run(None, None, None) == -1
    assert L.lle_search_plan(None, None, 0) == -1
    assert L.lle_search_stats(None, None, None, 0) == -1
    assert L.lle_search_lower_bound(None) == -1
    L.lle_search_free(None)


REFERENCE_MODES = ["standard", "no-cooperation", "no-asymmetric", "no-mutual", "no-fully-coupled", "no-sequence", "no-sequence-2", "no-sequence-3",
                   "no-interdependence", "no-interdependence-3", "no-interdependence-4", "no-convergence", "no-convergence-2", "no-convergence-3",
                   "no-divergence", "no-divergence-2", "no-divergence-3"]


@pytest.mark.parametrize("text", REFERENCE_MODES)
def test_every_mode_of_the_reference_parses(text):
    mode = solver.SolveMode.from_str(text)
    assert solver.SolveMode.from_str(str(mode)) == mode and hash(solver.SolveMode.from_str(str(mode))) == hash(mode)
    s = solver.Solver(LINE, 5)
    if text in ("standard", "no-cooperation"):
        assert mode.is_built and mode == (solver.SolveMode.standard() if text == "standard" else solver.SolveMode.no_cooperation())
        return
    for call in (lambda: s.find_shortest(text), lambda: s.find_shortest(mode), lambda: s.solve(mode=text), lambda: solver.solve(LINE, 5, mode=text)):
        with pytest.raises(NotImplementedError, match=re.escape(str(mode))):
            call()


def test_the_error_names_the_mode_the_caller_wrote():
    s = solver.Solver(LINE, 5)
    with pytest.raises(NotImplementedError, match="'no-mutual'"):
        s.find_shortest("no-mutual")
    with pytest.raises(NotImplementedError, match="'no-sequence-2'"):
        s.solve(mode="no-sequence-2")


def test_a_solver_is_frozen_at_construction():
    w = World("S0 . X X")
    s = solver.Solver(w, 5)
    w.exit_pos = [(0, 3)]
    assert s.solution_lower_bound == 2 and s._map.positions(1) == [(0, 2), (0, 3)] and w._map.positions(1) == [(0, 3)]
    assert solver.Solver(w, 5).solution_lower_bound == 3


def test_mode_strings():
    M = solver.SolveMode
    assert str(M.from_str("no-sequence-2")) == "no-sequence" and str(M.no_sequence(3)) == "no-sequence-3"  # solve_mode.rs:195-206
    assert M.from_str("no-mutual") == M.no_interdependence(2) and M.from_str("no-divergence") == M.no_divergence(2) != M.no_convergence(2)
    for bad in ("no-sequence-1", "no-sequence-0", "no-sequence-x", "no-interdependence-1", "no-divergence-", "no-divergence2", "cooperative", ""):
        with pytest.raises(ValueError):
            M.from_str(bad)
    with pytest.raises(ValueError):
        solver.Solver(LINE, 5).find_shortest("nonsense")


def test_characterizer_without_a_search():
    w = World("S0 L1S X\n. . .\n. . X\nS1 . L0N")
    c = characterization.WorldCharacterizer(w, 6)
    assert c.world is w and c.t_max == 6 and c.n_laser_colours == 2
    assert c == characterization.WorldCharacterizer(w, 6) and hash(c) == hash(characterization.WorldCharacterizer(w, 6))
    assert c != characterization.WorldCharacterizer(w, 7) and c != characterization.WorldCharacterizer(World("S0 X"), 6) and c != 6
    for call, mode in ((c.is_asymmetric, "no-asymmetric"), (c.is_fully_coupled, "no-fully-coupled"), (c.is_sequential, "no-sequence-2"),
                       (lambda: c.is_sequential(3), "no-sequence-3"), (c.is_convergent, "no-convergence-2"), (lambda: c.is_divergent(4), "no-divergence-4"),
                       (c.is_interdependent, "no-interdependence-2"), (c.is_mutual, "no-mutual")):
        with pytest.raises(NotImplementedError, match=mode):
            call()
    for call in (lambda: c.is_sequential(1), lambda: c.is_convergent(1), lambda: c.is_divergent(0), lambda: c.is_interdependent(1)):
        with pytest.raises(ValueError):
            call()


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_table_code_under_sanitizers(tmp_path):
    """tests/hostsim/search_table.cpp: its own main over search_logic.hpp, built with g++ -fsanitize=address,undefined and run as a child
    process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "search_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "search_table.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["inserts"]) > 50000 and int(out["duplicates"]) > 10000 and int(out["full"]) >= 160


def test_record_io_under_sanitizers(tmp_path):
    """tests/hostsim/record_io.cpp: its own main over the record I/O of search_logic.hpp -- the code that search.hip, forest.hip and
    policy.hip run between a batch, a pool and a table slot -- on fake batches in exactly sized vectors, built with
    g++ -fsanitize=address,undefined and run as a child process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "record_io")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "record_io.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        # 6 agent counts x 4 beam-word counts x 2 agent pitches x 2 key widths; all 5 + 25 + 125 codes below four agents, 203 above
        assert res.stdout.startswith("OK ") and int(out["cases"]) == 96 and int(out["codes"]) == 16 * (5 + 25 + 125 + 3 * 203)
        assert int(out["valid"]) > 500 and int(out["compared"]) > 2000
