"""The closed-trail cooperation tracker without a GPU: the restatement (tests/coopcycles_ref.py) against the host graph class
(lle_amd.characterization) on the reference's graphs (tests/golden/kat_coop.json) and on random layered ones; cl::layer_update as the
kernel calls it, under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program (tests/hostsim/coopcycles_values.cpp)
against the restatement's encoder, bit for bit; header / exports / binding, build list and entry check; the refusals of
cooperation="closed-trails"; the scripted plans of the GPU rollouts replayed on the oracle with the coverage the GPU tests assert.
The kernel itself is compared on the MI355X (tests/test_gpu_coopcycles.py, tests/test_gpu_coopcycles_states.py)."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lle_amd
from lle_amd import coopcycles, cycles
from lle_amd.characterization import DependencyEdge, TemporalCooperationGraph
from tests import coopcycles_play, coopcycles_ref, cycles_ref, source_text
from tests.coopcycles_ref import CLEAR, FINISH, MARK_POS, MARK_STARTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
GRAPHS = [g for g in json.load(open(os.path.join(ROOT, "tests", "golden", "kat_coop.json")))["graphs"] if "interdependent" in g["expect"]]
KERNELS = ["coopcycles_kernel<3>", "coopcycles_kernel<21>"]


def _graph(edges):
    return TemporalCooperationGraph([DependencyEdge(h, b, t) for h, b, t in edges])


def random_layers(rng, n_agents):
    """1 to 6 states of 0 to 5 arcs each."""
    layers = []
    for _ in range(int(rng.integers(1, 7))):
        arcs = set()
        for _ in range(int(rng.integers(0, 6))):
            h, b = rng.choice(n_agents, 2, replace=False)
            arcs.add((int(h), int(b)))
        layers.append(frozenset(arcs))
    return layers


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", GRAPHS, ids=[c["name"] for c in GRAPHS])
def test_restatement_on_the_reference_graphs(case):
    """The closed orders of the triples against the graph class and against what the golden file states."""
    edges = [tuple(e) for e in case["edges"]]
    graph = _graph(edges)
    n_agents = 1 + max([max(h, b) for h, b, _t in edges], default=0)
    orders = coopcycles_ref.closed_orders(coopcycles_ref.graph_triples(edges))
    for k in range(2, n_agents + 2):
        assert (k in orders) == graph.has_closed_trail_of_order(k) == graph.profile().is_interdependent(k), (k, orders)
    for k, want in case["expect"]["interdependent"].items():
        assert (int(k) in orders) == want, (k, orders)


def test_restatement_on_random_layered_graphs():
    rng = np.random.default_rng(23)
    seen = set()
    for _ in range(300):
        A = int(rng.integers(2, 7))
        layers = random_layers(rng, A)
        edges = [(h, b, t) for t, arcs in enumerate(layers) for h, b in arcs]
        graph = _graph(edges)
        R = coopcycles_ref.graph_triples(edges)
        orders = coopcycles_ref.closed_orders(R)
        for k in range(2, 7):
            assert (k in orders) == graph.has_closed_trail_of_order(k), (k, orders, edges)
        assert cycles.triples(coopcycles_ref.encode(R, A), A) == set(R)  # the encoder against the package's decode
        if A <= 4:
            assert cycles.triples(coopcycles_ref.encode(R, A, words=21), 6) == set(R)
        seen |= set(orders)
    assert seen == {2, 3, 4, 5, 6} or seen >= {2, 3, 4}, seen


def test_encoder_places_the_fields_of_the_header_comment():
    """cycles_logic.hpp, THE BITS: closed field a at bit a * 2^(AC - 1), open field (a, c) at AC * 2^(AC - 1) + ... ; bit p = the
    support with a one inserted at min(a, c) and then at max(a, c)."""
    assert coopcycles_ref.encode({(0, 0, frozenset({0, 1}))}, 4) == [1 << 1, 0, 0]              # closed 0: mask 0b11 without bit 0 = 1
    assert coopcycles_ref.encode({(3, 3, frozenset({0, 1, 2, 3}))}, 4) == [1 << 31, 0, 0]        # closed 3 at bit 24, p = 7
    assert coopcycles_ref.encode({(0, 1, frozenset({0, 1}))}, 4) == [0, 1, 0]                    # the first open field, p = 0
    assert coopcycles_ref.encode({(3, 2, frozenset({0, 1, 2, 3}))}, 4) == [0, 0, 1 << 15]        # the last open field (index 11), p = 3
    assert coopcycles_ref.encode({(5, 5, frozenset({5}))}, 6)[5] == 1 and coopcycles_ref.encode({(5, 4, frozenset(range(6)))}, 6)[20] == 1 << 31
    assert coopcycles_ref.words_of(4) == 3 and coopcycles_ref.words_of(5) == 21 and coopcycles.words_of(4) == 3 and coopcycles.words_of(5) == 21
    assert coopcycles_ref.as_int32(0x80000000) == -(1 << 31) and coopcycles_ref.orders_byte({(1, 1, frozenset({0, 1, 2}))}) == 8


def test_env_ref_operations():
    r = coopcycles_ref.EnvRef(3)
    r.update(0)
    assert r.arrays() == ([0] * 3, [0] * 3, [0] * 4, [0] * 4) and not r.touched
    r.update(MARK_POS, {(0, 1)})
    r.update(MARK_POS, set())
    r.update(MARK_POS, {(1, 2)})
    assert r.R == {(0, 1, frozenset({0, 1})), (1, 2, frozenset({1, 2})), (0, 2, frozenset({0, 1, 2}))} and r.arrays()[2] == [0, 2, 0, 1]
    r.update(MARK_POS, {(2, 0)}, refused=True)  # a refused step made no state
    assert r.orders() == [] and r.arrays()[2] == [0, 2, 0, 1]
    r.update(MARK_POS, {(2, 0)})
    assert r.orders() == [3] and r.arrays()[2] == [8, 3, 0, 1] and r.flat == {(0, 1), (1, 2), (2, 0)}
    r.update(MARK_POS, {(1, 2), (2, 0)}, start_edges={(0, 1)}, was_reset=True)  # the start layer and the step layer chain
    assert r.orders() == [3] and r.orders(last=True) == [3] and r.finished and r.layers == 2 and r.arrays()[2:] == ([8, 2, 0, 1], [8, 3, 0, 1])
    r.update(MARK_POS, {(1, 0)}, start_edges={(0, 1)}, was_reset=True, refused=True)
    assert r.R == {(0, 1, frozenset({0, 1}))} and r.arrays()[2:] == ([0, 1, 0, 1], [8, 2, 0, 1])
    r.update(FINISH | CLEAR)
    assert r.arrays() == ([0] * 3, [0, 1, 0], [0, 0, 0, 1], [0, 1, 0, 1])
    r.update(MARK_STARTS | MARK_POS, {(1, 0)}, start_edges={(0, 1)})  # inside one call: starts first
    assert r.orders() == [2]


# ---------------------------------------------------------------------------------------------- the walk as the kernel calls it, sanitized
def test_values_under_sanitizers(tmp_path):
    """tests/hostsim/coopcycles_values.cpp: its own main over cycles_logic.hpp, built with g++ -fsanitize=address,undefined and run as
    a child process; nothing sanitized is loaded into this interpreter.  The cases -- the arc word and the expected words after every
    layer -- go to it as a text file written from the restatement and its encoder."""
    exe, cases = str(tmp_path / "coopcycles_values"), str(tmp_path / "cases.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "coopcycles_values.cpp"), "-o", exe] + SAN, check=True)
    rng = np.random.default_rng(29)
    named = [(3, [{(0, 1), (1, 2), (2, 0)}]), (3, [{(0, 1)}, {(1, 2)}, {(2, 0)}]), (3, [{(2, 0)}, {(1, 2)}, {(0, 1)}]),
             (4, [{(0, 1), (1, 0)}, {(1, 2), (2, 1)}, {(1, 0)}]), (6, [{(a, (a + 1) % 6) for a in range(6)}]), (5, [set(), {(4, 0)}, set()])]
    layered = named + [(A, random_layers(rng, A)) for A in [int(rng.integers(2, 7)) for _ in range(300)]]
    n_small = n_large = n_layers = 0
    with open(cases, "w") as f:
        for A, layers in layered:
            for W in ([3, 21] if A <= 4 else [21]):
                R, parts = frozenset(), []
                for arcs in layers:
                    R = cycles_ref.layer_update(R, arcs)
                    parts.append(format(sum(1 << (8 * h + b) for h, b in arcs), "x") + " " + " ".join(format(w, "x") for w in coopcycles_ref.encode(R, A, words=W)))
                f.write(f"{W} {A} {len(layers)} " + " ".join(parts) + "\n")
                n_small, n_large, n_layers = n_small + (W == 3), n_large + (W == 21), n_layers + len(layers)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    out = dict(kv.split("=") for kv in res.stdout.split()[1:])
    assert res.stdout.startswith("OK ") and int(out["small"]) == n_small and int(out["large"]) == n_large and int(out["layers"]) == n_layers
    assert n_small >= 100 and n_large >= 300 and int(out["last_word"]) >= 20 and int(out["closed"]) >= 100 and int(out["dense"]) == 3
    assert 1 <= int(out["max_spent"]) <= 64  # states of at most 5 arcs stay far inside the budget of 4 096


def test_source_is_plain_code_over_the_public_abi():
    hip = os.path.join("lle_amd", "coopcycles", "coopcycles.hip")
    source = source_text.text_of(hip)  # the .hip and the headers of lle_amd/ it includes
    assert {os.path.basename(p) for p in source_text.files_of(hip)} == {"coopcycles.hip", "cycles_logic.hpp", "helpgraph_logic.hpp", "search_logic.hpp",
                                                                        "tracker_core.hpp", "episode_ops.hpp", "abi_host.hpp"}
    assert not re.search(r"\b(__)?asm(__)?\b", source)  # plain C++ only
    assert '#include "../cycles/cycles_logic.hpp"' in source and "cl::layer_update<W>" in source and "cl::Order{A, ~0ull, 0ull}" in source
    assert "getenv" not in source and "hipMalloc" not in source_text.update_path_of(hip, "int lle_coopcycles_update(")
    # over the public ABI only: the batch through lle_batch_get_buffer, the coop handle through its buffer and start edges
    used = set(re.findall(r"\b(lle_(?:batch|coop|map|cooptrails|cycles)_[a-z_0-9]+)\s*\(", source))
    assert used == {"lle_batch_get_buffer", "lle_batch_n_envs", "lle_batch_n_maps", "lle_coop_buffer", "lle_coop_start_edges", "lle_coop_last_error"}


# ---------------------------------------------------------------------------------------------- header, exports, binding, build
def test_library_exports():
    """liblle_coopcycles.so exports every function include/lle_coopcycles.h declares, and the binding knows exactly those; the header
    is plain C and the one the library is compiled against; struct size and enum values of the binding are the header's."""
    L = coopcycles.lib()
    header = open(os.path.join(ROOT, "include", "lle_coopcycles.h")).read()
    declared = set(re.findall(r"\b(lle_coopcycles_[a-z_0-9]+)\s*\(", header))
    assert declared == set(coopcycles.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = source_text.text_of(os.path.join("lle_amd", "coopcycles", "coopcycles.hip"))
    assert '#include "../../include/lle_coopcycles.h"' in source
    names = ["LLE_COOPCYCLES_FINISH", "LLE_COOPCYCLES_CLEAR", "LLE_COOPCYCLES_MARK_STARTS", "LLE_COOPCYCLES_MARK_POS", "LLE_COOPCYCLES_HONOUR_AUTO_RESET",
             "LLE_COOPCYCLES_SKIP_REFUSED", "LLE_COOPCYCLES_EPISODE_CLOSED", "LLE_COOPCYCLES_LAST_CLOSED", "LLE_COOPCYCLES_EPISODE_CPROFILE",
             "LLE_COOPCYCLES_LAST_CPROFILE", "LLE_COOPCYCLES_BUF_COUNT", "LLE_COOPCYCLES_MAX_AGENTS", "LLE_COOPCYCLES_SMALL_WORDS", "LLE_COOPCYCLES_LARGE_WORDS",
             "LLE_COOPCYCLES_WALK_BUDGET", "LLE_COOP_FINISH", "LLE_COOP_CLEAR", "LLE_COOP_MARK_STARTS", "LLE_COOP_MARK_POS", "LLE_COOP_HONOUR_AUTO_RESET"]
    prog = ('#include <stdio.h>\n#include "lle_coopcycles.h"\nint main(void) { printf("%zu' + " %d" * len(names) + '", sizeof(lle_coopcycles_update_args), '
            + ", ".join(names) + "); return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    cc = coopcycles
    assert got == [C.sizeof(cc.UpdateArgs), cc.LLE_COOPCYCLES_FINISH, cc.LLE_COOPCYCLES_CLEAR, cc.LLE_COOPCYCLES_MARK_STARTS, cc.LLE_COOPCYCLES_MARK_POS,
                   cc.LLE_COOPCYCLES_HONOUR_AUTO_RESET, cc.LLE_COOPCYCLES_SKIP_REFUSED, cc.LLE_COOPCYCLES_EPISODE_CLOSED, cc.LLE_COOPCYCLES_LAST_CLOSED,
                   cc.LLE_COOPCYCLES_EPISODE_CPROFILE, cc.LLE_COOPCYCLES_LAST_CPROFILE, 4, cc.LLE_COOPCYCLES_MAX_AGENTS, cc.LLE_COOPCYCLES_SMALL_WORDS,
                   cc.LLE_COOPCYCLES_LARGE_WORDS, cc.LLE_COOPCYCLES_WALK_BUDGET,
                   cc.LLE_COOPCYCLES_FINISH, cc.LLE_COOPCYCLES_CLEAR, cc.LLE_COOPCYCLES_MARK_STARTS, cc.LLE_COOPCYCLES_MARK_POS, cc.LLE_COOPCYCLES_HONOUR_AUTO_RESET]
    assert [FINISH, CLEAR, MARK_STARTS, MARK_POS] == got[1:5] and coopcycles_ref.MAX_AGENTS == cc.LLE_COOPCYCLES_MAX_AGENTS
    assert C.sizeof(cc.UpdateArgs) == C.sizeof(lle_amd.cooperation.UpdateArgs) == C.sizeof(lle_amd.cooptrails.UpdateArgs)
    logic = open(os.path.join(ROOT, "lle_amd", "cycles", "cycles_logic.hpp")).read()
    assert "WALK_BUDGET = 4096" in logic and "SMALL_AGENTS = 4, SMALL_WORDS = 3, LARGE_WORDS = 21" in logic
    assert coopcycles.compiled_kernels() == KERNELS
    assert coopcycles.launched_kernels() == []


def test_build_list_and_entry_check_name_the_library():
    build = open(os.path.join(ROOT, "lle_amd", "build.py")).read()
    assert '("coopcycles", "liblle_coopcycles.so")' in build
    at = build.index('("coopcycles", "liblle_coopcycles.so")')
    assert build.index('("coop", "liblle_coop.so")') < build.index('("cooptrails", "liblle_cooptrails.so")') < at  # it links against liblle_coop.so
    assert build.index('("cycles", "liblle_cycles.so")') < at
    pairs = re.findall(r'\("([a-z]+)", "(liblle_[a-z]+\.so)"\)', build)
    assert len(pairs) == 14 and pairs[0] == ("csrc", "liblle_hip.so") and pairs[-1] == ("coopcycles", "liblle_coopcycles.so")
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "coopcycles.EXPORTS" in entry and "liblle_coopcycles.so does not export" in entry
    makefile = open(os.path.join(ROOT, "lle_amd", "coopcycles", "Makefile")).read()
    assert "-llle_coop -llle_hip" in makefile and "ARCH ?= gfx950" in makefile and "../cycles/cycles_logic.hpp" in makefile
    needed = subprocess.run(["readelf", "-d", coopcycles.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "liblle_coop.so" in needed and "liblle_hip.so" in needed and "$ORIGIN" in needed
    assert "liblle_cycles.so" not in needed and "liblle_cooptrails.so" not in needed  # the logic header only, and the coop handle only


def test_lazy_name_and_arguments():
    assert lle_amd.ClosedTrailCooperationTracker is coopcycles.ClosedTrailCooperationTracker and "ClosedTrailCooperationTracker" in lle_amd.__all__
    assert issubclass(coopcycles.ClosedTrailCooperationTracker, lle_amd.TemporalCooperationTracker)
    with pytest.raises(NotImplementedError):  # the trails tracker keeps refusing
        object.__new__(lle_amd.TemporalCooperationTracker).is_interdependent(3)
    for bad in ("flattened", "closed", "closed_trails", "Temporal"):
        with pytest.raises(ValueError, match="\"temporal\" or \"closed-trails\""):
            lle_amd.BatchedLLE.__init__(object.__new__(lle_amd.BatchedLLE), "S0 X", 1, cooperation=bad, device="cpu")
    seven = "L0E " + " ".join(f"S{a}" for a in range(7)) + " @\n" + " ".join(["X"] * 7) + " . ."
    for maps in (seven, [seven, seven], lle_amd.Map(seven)):
        with pytest.raises(ValueError, match="at most 6 agents, this one has 7"):
            lle_amd.BatchedLLE.__init__(object.__new__(lle_amd.BatchedLLE), maps, 2, cooperation="closed-trails", device="cpu")
    with pytest.raises(ValueError, match="at most 6 agents"):
        coopcycles.ClosedTrailCooperationTracker(type("W", (), {"map": lle_amd.Map(seven)})())


def test_host_side_refusals():
    L = coopcycles.lib()
    assert L.lle_coopcycles_update(None, None, None) == -1 and b"NULL" in L.lle_coopcycles_last_error()
    assert L.lle_coopcycles_update_map(None, 0, None) == -1
    assert L.lle_coopcycles_buffer(None, 0) is None
    assert L.lle_coopcycles_create(None, None, None) is None  # (no device here, or NULL handles there: refused either way)
    assert L.lle_coopcycles_last_error() != b""
    L.lle_coopcycles_free(None)


# ---------------------------------------------------------------------------------------------- the plans and the coverage of the GPU rollouts
@pytest.mark.parametrize("text", list(coopcycles_play.PLANNED), ids=["paper3", "paper3-open", "cycle3", "four"])
def test_plans_close_a_trail_over_all_agents(text):
    """The shortest plan of each scripted map, asserted by cycles_ref.check_plan through the host graph class: it closes exactly the
    orders coopcycles_play.PLANNED names; replayed layer by layer through EnvRef, the top order appears at the plan's last steps only."""
    plan = coopcycles_play.plan_of(text)
    _t_max, orders = coopcycles_play.PLANNED[text]
    R, edges, _world = cycles_ref.replay_triples(text, plan)
    n_agents = len(plan[0])
    assert coopcycles_ref.closed_orders(R) == orders and orders[-1] == n_agents
    ref = coopcycles_ref.EnvRef(n_agents)
    ref.update(CLEAR)
    for t in range(len(plan) + 1):
        ref.update(MARK_POS, {(h, b) for h, b, tt in edges if tt == t})
    assert ref.R == R and ref.orders() == orders and cycles.triples(coopcycles_ref.encode(R, n_agents), n_agents) == set(R)


@pytest.mark.parametrize("name", sorted(coopcycles_play.ROLLOUTS))
def test_rollout_coverage_on_the_oracle(oracle_mod, name):
    """play(gpu=False) with the very arguments of the GPU tests gives the counts those tests assert as their minimum."""
    kwargs, counts = coopcycles_play.ROLLOUTS[name]
    assert coopcycles_play.play(oracle_mod, gpu=False, **kwargs) == counts
    must = {"paths": ("finished_top", "running_top", "refused_scripted"), "resets_auto": ("finished_top", "running_top", "order2_only", "refused_scripted"),
            "resets_mask": ("finished_top", "running_top", "order2_only", "refused_scripted"), "resets_none": ("running_top", "order2_only", "refused_scripted"),
            "four": ("finished_top", "running_top", "order2_only", "refused_scripted"), "two_maps": ("finished_top",), "set_state": ("finished_top",),
            "chain": ("chained",)}[name]
    assert all(counts[k] >= 10 for k in must), counts
