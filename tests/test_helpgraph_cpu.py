"""The help-graph solver without a GPU: header / exports / binding of liblle_helpgraph.so, every refusal of its ABI, the solve modes
it serves, the restatement (tests/helpgraph_ref.py) against the reference's stated values (tests/golden/kat_helpgraph.json) and the
recorded searches, and lle_amd/helpgraph/helpgraph_logic.hpp under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/hostsim/helpgraph_logic.cpp).  The search itself runs on the MI355X (tests/test_gpu_helpgraph.py)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, characterization, generator, helpgraph, solver
from tests import helpgraph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = helpgraph_ref.load_cases()
MAPS = dict({c["name"]: c["map"] for c in CASES["catalogue"]}, **CASES["maps"])
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
KERNELS = ["hg_commit", "hg_expand", "hg_insert<false>", "hg_insert<true>"]
LAYOUTS = ["single-laser-asymmetric", "double-disjoint-asymmetric", "convergent-2-tight", "divergent-2-tight", "divergent-2-with-detour",
           "paper-convergent-2", "paper-fully-coupled", "paper-fully-coupled-legacy", "fully-coupled-4agents", "two-agent-mutual-compact",
           "two-agent-mutual-with-detours"]


def search_id(s):
    return f"{s['map']}-t{s['t_max']}-{s['mode']}-{s['param']}" + ("-gems" if s["collect_gems"] else "")


def test_kat_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location("make_kat_helpgraph", os.path.join(ROOT, "tests", "golden", "make_kat_helpgraph.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CATALOGUE == CASES["catalogue"] and mod.MAPS == CASES["maps"] and mod.SEARCHES == CASES["searches"]
    assert [c["name"] for c in CASES["catalogue"]] == LAYOUTS
    fields = {"asymmetric", "fully_coupled", "convergent", "divergent", "interdependent"}
    for c in CASES["catalogue"]:
        assert c["ref"].startswith("python/tests/world_layouts.py:") and c["expect"]
        for e in c["expect"].values():
            assert e and set(e) <= fields and set(e.get("interdependent", {"2": 0})) == {"2"}
    horizons = {c["name"]: sorted(int(t) for t in c["expect"]) for c in CASES["catalogue"]}
    assert horizons["divergent-2-tight"] == [2, 8] and horizons["divergent-2-with-detour"] == [2, 5, 6, 8]
    assert horizons["two-agent-mutual-with-detours"] == list(range(5, 15))
    assert not {s["map"] for s in CASES["searches"]} & set(BEYOND_THE_RESTATEMENT)
    for s in CASES["searches"]:
        assert s["map"] in MAPS and s["mode"] in helpgraph_ref.MODES and sum(s["frontier"]) == s["states"] <= 7599
        assert len(s["expanded"]) == len(s["frontier"]) - 1 and (s["length"] is None or s["length"] == len(s["expanded"]))


def test_library_exports():
    """liblle_helpgraph.so exports every function include/lle_helpgraph.h declares, and the binding knows exactly those; the header is
    plain C and the one the library is compiled against; struct sizes and constants of the binding are the header's."""
    L = helpgraph.lib()
    header = open(os.path.join(ROOT, "include", "lle_helpgraph.h")).read()
    declared = set(re.findall(r"\b(lle_helpgraph_[a-z_0-9]+)\s*\(", header))
    assert declared == set(helpgraph.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "helpgraph", "helpgraph.hip")).read()
    assert '#include "../../include/lle_helpgraph.h"' in source and '#include "helpgraph_logic.hpp"' in source
    assert '#include "../search/search_logic.hpp"' in source and '#include "../search/search_device.hpp"' in source
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    names = ["LLE_HELPGRAPH_CAPACITY", "LLE_HELPGRAPH_STANDARD", "LLE_HELPGRAPH_NO_ASYMMETRIC", "LLE_HELPGRAPH_NO_MUTUAL", "LLE_HELPGRAPH_NO_FULLY_COUPLED",
             "LLE_HELPGRAPH_NO_CONVERGENCE", "LLE_HELPGRAPH_NO_DIVERGENCE", "LLE_HELPGRAPH_MAX_AGENTS", "LLE_HELPGRAPH_MAX_SOURCES"]
    prog = ('#include <stdio.h>\n#include "lle_helpgraph.h"\nint main(void) { printf("%zu %zu %zu' + " %d" * len(names) + '", sizeof(lle_helpgraph_options), '
            'sizeof(lle_helpgraph_args), sizeof(lle_helpgraph_result), ' + ", ".join(names) + '); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(helpgraph.HelpGraphOptions), C.sizeof(helpgraph.HelpGraphArgs), C.sizeof(helpgraph.HelpGraphResult)] + [getattr(helpgraph, n) for n in names]
    assert helpgraph.LLE_HELPGRAPH_CAPACITY == solver.LLE_SEARCH_CAPACITY
    assert sorted(helpgraph.compiled_kernels()) == KERNELS


def test_lazy_names():
    assert lle_amd.HelpGraphSolver is helpgraph.HelpGraphSolver and lle_amd.HelpGraphCharacterizer is helpgraph.HelpGraphCharacterizer
    assert issubclass(helpgraph.HelpGraphSolver, solver.Solver) and issubclass(helpgraph.HelpGraphCharacterizer, characterization.WorldCharacterizer)
    assert {"HelpGraphSolver", "HelpGraphCharacterizer"} <= set(lle_amd.__all__)


def test_host_side_refusals():
    """NULL and bad-argument refusals of every ABI call that can be made without a device."""
    L, line, seven = helpgraph.lib(), Map(LINE), Map(SEVEN)
    assert L.lle_helpgraph_create(None, None) is None and b"NULL" in L.lle_helpgraph_last_error()
    bad = helpgraph.HelpGraphOptions(4, -1, 0, 0, None)
    assert L.lle_helpgraph_create(line.h, C.byref(bad)) is None and b"struct_bytes" in L.lle_helpgraph_last_error()
    for chunk, max_states, word in ((-1, 0, b"chunk"), ((1 << 30) + 1, 0, b"chunk"), (0, -1, b"max_states"), (0, 1 << 31, b"max_states"), (0, (1 << 30) + 1, b"max_states")):
        opt = helpgraph.HelpGraphOptions(C.sizeof(helpgraph.HelpGraphOptions), -1, chunk, max_states, None)
        assert L.lle_helpgraph_create(line.h, C.byref(opt)) is None and word in L.lle_helpgraph_last_error()
    assert L.lle_helpgraph_create(seven.h, None) is None and b"more than 6 agents" in L.lle_helpgraph_last_error()
    args, res = helpgraph.HelpGraphArgs(C.sizeof(helpgraph.HelpGraphArgs), 0, 2, 0, 5), helpgraph.HelpGraphResult(C.sizeof(helpgraph.HelpGraphResult))
    assert L.lle_helpgraph_run(None, None, None) == -1 and L.lle_helpgraph_run(None, C.byref(args), C.byref(res)) == -1
    assert L.lle_helpgraph_plan(None, None, 0) == -1
    assert L.lle_helpgraph_stats(None, None, None, 0) == -1
    L.lle_helpgraph_free(None)


def test_help_edges():
    assert helpgraph.help_edges(0, 0) == set()
    assert helpgraph.help_edges(1 << 1 | 1 << 8 | 1 << (8 * 3 + 5), 1 << (8 * 5 + 4 - 32)) == {(0, 1), (1, 0), (3, 5), (5, 4)}


# ------------------------------------------------------------------------------------------------ the mode table
REFERENCE_MODES = ["standard", "no-cooperation", "no-asymmetric", "no-mutual", "no-fully-coupled", "no-sequence", "no-sequence-2", "no-sequence-3",
                   "no-interdependence", "no-interdependence-2", "no-interdependence-3", "no-interdependence-4", "no-convergence", "no-convergence-2",
                   "no-convergence-3", "no-divergence", "no-divergence-2", "no-divergence-3"]
UNBUILT = {"no-sequence", "no-sequence-2", "no-sequence-3", "no-interdependence-3", "no-interdependence-4"}


@pytest.mark.parametrize("text", REFERENCE_MODES)
def test_every_mode_of_the_reference_is_served_or_named(text):
    s = helpgraph.HelpGraphSolver(LINE, 1)  # (the lower bound, 3, exceeds t_max: a served mode answers None without a search, without a device)
    mode = solver.SolveMode.from_str(text)
    assert helpgraph.serves(text) == helpgraph.serves(mode) == (text not in UNBUILT)
    if text in UNBUILT:
        for call, name in ((lambda: s.find_shortest(text), text), (lambda: s.find_shortest(mode), str(mode)), (lambda: s.solve(mode=text), text)):
            with pytest.raises(NotImplementedError, match=re.escape(f"'{name}'")) as err:  # the mode as the caller wrote it
                call()
            assert "'no-mutual'" in str(err.value) and "'no-convergence[-k]'" in str(err.value)  # the message lists what is served
    else:
        assert s.find_shortest(text) is None and s.find_shortest(mode) is None and s.solve(0, mode=text) is None
    assert s.h is None


def test_mutual_is_interdependence_2():
    M = solver.SolveMode
    assert M.from_str("no-mutual") == M.from_str("no-interdependence") == M.from_str("no-interdependence-2") == M.no_mutual()
    assert helpgraph._served_mode("no-mutual").kind == "no-interdependence" and helpgraph._NATIVE["no-interdependence"] == helpgraph.LLE_HELPGRAPH_NO_MUTUAL
    with pytest.raises(ValueError):
        helpgraph.HelpGraphSolver(LINE, 5).find_shortest("nonsense")
    with pytest.raises(ValueError):
        helpgraph.HelpGraphSolver(LINE, 5).find_shortest("no-convergence-1")


def test_the_solver_interface_without_a_search():
    w = World(LINE)
    s = helpgraph.HelpGraphSolver(w, 7, chunk=3, max_states=5)
    assert s.world is w and s.t_max == 7 and (s.chunk, s.max_states) == (3, 5) and s.last_stats is None and s.solution_lower_bound == 3
    assert helpgraph.HelpGraphSolver(LINE).t_max == 2
    with pytest.raises(ValueError, match="exceeds this solver's t_max"):
        s.find_shortest("no-mutual", t_min=8)
    with pytest.raises(ValueError, match="exceeds this solver's t_max=7"):
        s.solve(8, mode="no-asymmetric")
    with pytest.raises(ValueError, match="non-negative"):
        s.solve(-1, mode="no-asymmetric")
    assert s.solve(2, mode="no-divergence-3") is None  # below the lower bound: no search, no device
    for bad in (dict(t_max=-1), dict(chunk=0), dict(max_states=0)):
        with pytest.raises(ValueError):
            helpgraph.HelpGraphSolver(LINE, **dict(dict(t_max=5), **bad))
    with pytest.raises(ValueError, match="at most 6 agents"):
        helpgraph.HelpGraphSolver(SEVEN, 4)
    w2 = World("S0 . X X")  # frozen at construction, like Solver
    s2 = helpgraph.HelpGraphSolver(w2, 5)
    w2.exit_pos = [(0, 3)]
    assert s2.solution_lower_bound == 2 and helpgraph.HelpGraphSolver(w2, 5).solution_lower_bound == 3


def test_the_characterizer_without_a_search():
    w = World("S0 L1S X\n. . .\n. . X\nS1 . L0N")
    c = helpgraph.HelpGraphCharacterizer(w, 6)
    assert c.world is w and c.t_max == 6 and c.n_laser_colours == 2
    assert c == helpgraph.HelpGraphCharacterizer(w, 6) and hash(c) == hash(helpgraph.HelpGraphCharacterizer(w, 6)) and c != helpgraph.HelpGraphCharacterizer(w, 7)
    for call, mode in ((c.is_sequential, "no-sequence-2"), (lambda: c.is_sequential(3), "no-sequence-3"), (lambda: c.is_interdependent(3), "no-interdependence-3")):
        with pytest.raises(NotImplementedError, match=mode):
            call()
    for call in (lambda: c.is_sequential(1), lambda: c.is_convergent(1), lambda: c.is_divergent(0), lambda: c.is_interdependent(1),
                 lambda: c.compute_shortest_path_without_convergence(1), lambda: c.compute_shortest_path_without_divergence(1),
                 lambda: c.compute_shortest_non_interdependent_path(1)):
        with pytest.raises(ValueError):
            call()
    assert c.is_divergent(2) is False and c.is_divergent(5) is False  # k >= n_agents: no search
    assert "characterizer" in generator.Constraint.is_satisfied_by.__kwdefaults__
    assert generator.Constraint.is_satisfied_by.__kwdefaults__["characterizer"] is characterization.WorldCharacterizer


# ------------------------------------------------------------------------------------------------ the restatement
# fully-coupled-4agents stores 84 128 records within its t_max of 8 (625 joint actions each): hours of replay for the restatement, and
# more than the 7 599 records every listed search stays within.  It has no search in the golden file and no test here or on the GPU
# compares it with the restatement (tests/golden/make_kat_helpgraph.py says what the searches through World.step find on it).
BEYOND_THE_RESTATEMENT = ("fully-coupled-4agents",)


def _stated():
    for c in CASES["catalogue"]:
        if c["name"] in BEYOND_THE_RESTATEMENT:
            continue
        for t, e in c["expect"].items():
            for key, want in e.items():
                for k, v in (want.items() if isinstance(want, dict) else [(None, want)]):
                    yield pytest.param(c["map"], int(t), key, k, v, id=f"{c['name']}-t{t}-{key}" + (f"-{k}" if k else ""))


@pytest.mark.parametrize("text,t_max,key,k,want", list(_stated()))
def test_the_restatement_reproduces_the_reference(text, t_max, key, k, want):
    """Every stated value of the golden file, through the reference's predicate definitions over tests/helpgraph_ref.py: the link between
    the reference and what the GPU tests compare the library with."""
    answers = helpgraph_ref.characterize(text, t_max)
    assert (answers[key]() if k is None else answers[key](int(k))) is want


@pytest.mark.parametrize("s", CASES["searches"], ids=[search_id(s) for s in CASES["searches"]])
def test_the_restatement_reproduces_the_recorded_searches(s):
    res = helpgraph_ref.search(MAPS[s["map"]], s["t_max"], s["mode"], s["param"], s["collect_gems"])
    assert (res.length, res.n_states, res.frontier, res.expanded) == (s["length"], s["states"], s["frontier"], s["expanded"])
    if res.plan is not None:
        edges = helpgraph_ref.check_plan(MAPS[s["map"]], res.plan, s["mode"], s["param"], s["collect_gems"], length=s["length"])
        assert edges == res.edges


def test_check_plan_refuses_what_a_mode_rejects():
    text = MAPS["two-agent-mutual-compact"]
    plan = helpgraph_ref.search(text, 6).plan
    assert helpgraph_ref.check_plan(text, plan, "no-asymmetric") == {(0, 1), (1, 0)}
    with pytest.raises(AssertionError):
        helpgraph_ref.check_plan(text, plan, "no-mutual")
    with pytest.raises(AssertionError):
        helpgraph_ref.check_plan(text, plan[:-1])
    single = MAPS["single-laser-asymmetric"]
    with pytest.raises(AssertionError):
        helpgraph_ref.check_plan(single, helpgraph_ref.search(single, 6).plan, "no-asymmetric")


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_logic_under_sanitizers(tmp_path):
    """tests/hostsim/helpgraph_logic.cpp: its own main over helpgraph_logic.hpp, built with g++ -fsanitize=address,undefined and run as a
    child process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "helpgraph_logic")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "helpgraph_logic.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        # every matrix of 2, 3 and 4 agents, 10 000 each of 5 and 6; 6 modes x the parameters 2 .. A + 1
        assert res.stdout.startswith("OK ") and int(out["matrices"]) == 4 + 64 + 4096 + 20000
        assert int(out["mode_checks"]) == 6 * (4 * 2 + 64 * 3 + 4096 * 4 + 10000 * 5 + 10000 * 6)
        assert int(out["states"]) == 4000 and int(out["with_edges"]) > 1000 and int(out["stored"]) > 100 and int(out["duplicates"]) > 1000
