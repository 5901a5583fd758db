"""The temporal cooperation tracker without a GPU: lle_amd/cooptrails/cooptrails_logic.hpp under AddressSanitizer +
UndefinedBehaviorSanitizer in a stand-alone program (tests/hostsim/cooptrails_logic.cpp), the restatement (tests/cooptrails_ref.py)
against the host graph class (lle_amd.characterization) on the reference's graphs (tests/golden/kat_coop.json) and on random ones, header
/ exports / binding, build list and entry check.  The kernel itself is compared on the MI355X (tests/test_gpu_cooptrails.py,
tests/test_gpu_cooptrails_states.py)."""
import ctypes as C
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lle_amd
from lle_amd import cooptrails
from lle_amd.characterization import DependencyEdge, TemporalCooperationGraph
from tests import cooptrails_ref, source_text
from tests.cooptrails_ref import CLEAR, FINISH, MARK_POS, MARK_STARTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
GRAPHS = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_coop.json")))["graphs"]
KERNELS = [f"cooptrails_kernel<{g}>" for g in (1, 2, 4, 8, 16)]


def _graph(edges):
    return TemporalCooperationGraph([DependencyEdge(h, b, t) for h, b, t in edges])


# ---------------------------------------------------------------------------------------------- the logic header, sanitized
def test_logic_header_under_sanitizers(tmp_path):
    """tests/hostsim/cooptrails_logic.cpp: its own main over cooptrails_logic.hpp, built with g++ -fsanitize=address,undefined and run as a
    child process; nothing sanitized is loaded into this interpreter.  The longest_trail cases of tests/golden/kat_coop.json go to it as
    a text file."""
    exe, kat = str(tmp_path / "cooptrails_logic"), str(tmp_path / "longest_trail.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "cooptrails_logic.cpp"), "-o", exe] + SAN, check=True)
    graphs = [g for g in GRAPHS if "longest_trail" in g["expect"]]
    fits = [g for g in graphs if all(0 <= h < 16 and 0 <= b < 16 and t >= 0 for h, b, t in g["edges"])]
    assert len(fits) >= 15 and {"trail_decreasing_times", "trail_may_not_revisit_same_edge", "trail_same_time"} <= {g["name"] for g in fits}
    with open(kat, "w") as f:
        for g in fits:
            f.write(" ".join(str(v) for v in [g["expect"]["longest_trail"], len(g["edges"])] + [x for e in g["edges"] for x in e]) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed), kat], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["graphs"]) == 8000 and int(out["kat"]) == len(fits)
        assert int(out["agent15"]) >= 20 and int(out["top_bits"]) >= 20 and int(out["beyond"]) >= 20 and int(out["same_as_narrow"]) >= 500


def test_logic_header_is_plain_code():
    logic = open(os.path.join(ROOT, "lle_amd", "cooptrails", "cooptrails_logic.hpp")).read()
    hip = os.path.join("lle_amd", "cooptrails", "cooptrails.hip")
    source = source_text.text_of(hip)  # the .hip and the headers of lle_amd/ it includes, the logic header among them
    assert {os.path.basename(p) for p in source_text.files_of(hip)} == {"cooptrails.hip", "cooptrails_logic.hpp", "tracker_core.hpp", "episode_ops.hpp", "abi_host.hpp"}
    assert not re.search(r"\b(__)?asm(__)?\b", source)  # plain C++ only
    assert "[" not in re.sub(r"//.*", "", logic), "no array in the logic header: nothing is indexed at run time"
    assert "WALK_BUDGET = 4096" in logic and "getenv" not in source
    assert "hipMalloc" not in source_text.update_path_of(hip, "int lle_cooptrails_update(")  # no allocation on the update path
    # over the public ABI only: the batch through lle_batch_get_buffer, the coop handle through its buffer and start edges
    used = set(re.findall(r"\b(lle_(?:batch|coop|map)_[a-z_0-9]+)\s*\(", source))
    assert used == {"lle_batch_get_buffer", "lle_batch_n_envs", "lle_batch_n_maps", "lle_coop_buffer", "lle_coop_start_edges", "lle_coop_last_error"}


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", GRAPHS, ids=[c["name"] for c in GRAPHS])
def test_restatement_on_the_reference_graphs(case):
    """The backward search of cooptrails_ref against the graph class: the longest trail, is_sequential for every length, and the mutual
    claim (a pair with both directions <=> a closed trail of exactly two agents)."""
    edges = [tuple(e) for e in case["edges"]]
    graph = _graph(edges)
    n_agents = 1 + max([max(h, b) for h, b, _t in edges], default=0)
    lengths = cooptrails_ref.trail_lengths(edges, n_agents, cap=len(edges) + 1)
    assert max(lengths, default=0) == graph.longest_trail_length()
    if "longest_trail" in case["expect"]:
        assert max(lengths, default=0) == case["expect"]["longest_trail"]
    capped = cooptrails_ref.trail_lengths(edges, n_agents)
    assert capped == [min(v, 15) for v in lengths]
    for length in range(2, 8):
        assert (max(capped, default=0) >= length) == graph.profile().is_sequential(length)
    assert cooptrails_ref.is_mutual((h, b) for h, b, _t in edges) == graph.has_closed_trail_of_order(2) == graph.profile().is_mutual
    if "is_mutual" in case["expect"]:
        assert cooptrails_ref.is_mutual((h, b) for h, b, _t in edges) == case["expect"]["is_mutual"]


def test_restatement_on_random_graphs():
    rng = np.random.default_rng(17)
    seen = set()
    for _ in range(300):
        A, T = int(rng.integers(2, 6)), int(rng.integers(1, 5))
        edges = {(int(rng.integers(A)), int(rng.integers(A)), int(rng.integers(T))) for _ in range(int(rng.integers(1, 9)))}
        edges = sorted(e for e in edges if e[0] != e[1])
        graph = _graph(edges)
        lengths = cooptrails_ref.trail_lengths(edges, A, cap=20)
        assert max(lengths, default=0) == graph.longest_trail_length()
        # per agent, through the graph class: a chain of K new agents behind agent a, K longer than any trail -- the longest trail of
        # that graph is the longest one that ends at a, then the chain
        K = len(edges) + 1
        for a in range(A):
            chain = [(a, A, T + 1)] + [(A + k, A + k + 1, T + 2 + k) for k in range(K - 1)]
            assert _graph(edges + chain).longest_trail_length() == lengths[a] + K
        mutual = cooptrails_ref.is_mutual((h, b) for h, b, _t in edges)
        assert mutual == graph.has_closed_trail_of_order(2)
        seen.add((mutual, max(lengths, default=0) >= 3))
    assert len(seen) == 4


def test_restatement_cap_is_the_suffix_argument():
    """A mutual pair held for ten states: 20 edges; capped at 15 the answer is min(true, 15) in both fields."""
    edges = [(0, 1, t) for t in range(10)] + [(1, 0, t) for t in range(10)]
    assert cooptrails_ref.trail_lengths(edges, 2, cap=100) == [20, 20] and cooptrails_ref.trail_lengths(edges, 2) == [15, 15]
    assert cooptrails_ref.pack([15] * 16) == -1 and cooptrails_ref.pack([1, 2, 3]) == 0x321


def test_env_ref_operations():
    r = cooptrails_ref.EnvRef(3)
    r.update(0)
    assert r.arrays() == (0, 0, [0] * 4, [0] * 4) and not r.touched
    r.update(MARK_POS, {(0, 1)})
    r.update(MARK_POS, set())
    r.update(MARK_POS, {(1, 2)})
    assert r.arrays() == (0x210, 0, [2, 2, 0, 1], [0] * 4)
    r.update(MARK_POS, {(2, 0)}, refused=True)  # a refused step made no state
    assert r.arrays() == (0x210, 0, [2, 2, 0, 1], [0] * 4)
    r.update(MARK_POS, {(0, 1)}, start_edges={(2, 0)}, was_reset=True)  # the start layer and the step layer chain
    assert r.arrays() == (0x021, 0x210, [2, 2, 0, 1], [2, 2, 0, 1]) and r.finished
    r.update(MARK_POS, {(0, 1)}, start_edges={(2, 0)}, was_reset=True, refused=True)
    assert r.arrays() == (0x001, 0x021, [1, 1, 0, 1], [2, 2, 0, 1])
    r.update(FINISH | CLEAR)
    assert r.arrays() == (0, 0x001, [0, 0, 0, 1], [1, 1, 0, 1])
    r.update(MARK_STARTS | MARK_POS, {(0, 2), (2, 0)}, start_edges={(2, 0)})  # decreasing order inside one call: starts first
    assert r.arrays()[0] == 0x203 and r.arrays()[2] == [3, 2, 0, 1]


# ---------------------------------------------------------------------------------------------- header, exports, binding, build
def test_library_exports():
    """liblle_cooptrails.so exports every function include/lle_cooptrails.h declares, and the binding knows exactly those; the header is
    plain C and the one the library is compiled against; struct size and enum values of the binding are the header's and lle_coop.h's."""
    L = cooptrails.lib()
    header = open(os.path.join(ROOT, "include", "lle_cooptrails.h")).read()
    declared = set(re.findall(r"\b(lle_cooptrails_[a-z_0-9]+)\s*\(", header))
    assert declared == set(cooptrails.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = source_text.text_of(os.path.join("lle_amd", "cooptrails", "cooptrails.hip"))
    assert '#include "../../include/lle_cooptrails.h"' in source and '#include "cooptrails_logic.hpp"' in source
    names = ["LLE_COOPTRAILS_FINISH", "LLE_COOPTRAILS_CLEAR", "LLE_COOPTRAILS_MARK_STARTS", "LLE_COOPTRAILS_MARK_POS", "LLE_COOPTRAILS_HONOUR_AUTO_RESET",
             "LLE_COOPTRAILS_SKIP_REFUSED", "LLE_COOPTRAILS_EPISODE_TRAILS", "LLE_COOPTRAILS_LAST_TRAILS", "LLE_COOPTRAILS_EPISODE_TPROFILE",
             "LLE_COOPTRAILS_LAST_TPROFILE", "LLE_COOPTRAILS_BUF_COUNT", "LLE_COOPTRAILS_SATURATED", "LLE_COOPTRAILS_WALK_BUDGET",
             "LLE_COOP_FINISH", "LLE_COOP_CLEAR", "LLE_COOP_MARK_STARTS", "LLE_COOP_MARK_POS", "LLE_COOP_HONOUR_AUTO_RESET"]
    prog = ('#include <stdio.h>\n#include "lle_cooptrails.h"\nint main(void) { printf("%zu' + " %d" * len(names) + '", sizeof(lle_cooptrails_update_args), '
            + ", ".join(names) + "); return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    ct = cooptrails
    assert got == [C.sizeof(ct.UpdateArgs), ct.LLE_COOPTRAILS_FINISH, ct.LLE_COOPTRAILS_CLEAR, ct.LLE_COOPTRAILS_MARK_STARTS, ct.LLE_COOPTRAILS_MARK_POS,
                   ct.LLE_COOPTRAILS_HONOUR_AUTO_RESET, ct.LLE_COOPTRAILS_SKIP_REFUSED, ct.LLE_COOPTRAILS_EPISODE_TRAILS, ct.LLE_COOPTRAILS_LAST_TRAILS,
                   ct.LLE_COOPTRAILS_EPISODE_TPROFILE, ct.LLE_COOPTRAILS_LAST_TPROFILE, 4, ct.LLE_COOPTRAILS_SATURATED, ct.LLE_COOPTRAILS_WALK_BUDGET,
                   ct.LLE_COOPTRAILS_FINISH, ct.LLE_COOPTRAILS_CLEAR, ct.LLE_COOPTRAILS_MARK_STARTS, ct.LLE_COOPTRAILS_MARK_POS, ct.LLE_COOPTRAILS_HONOUR_AUTO_RESET]
    assert [FINISH, CLEAR, MARK_STARTS, MARK_POS] == got[1:5] and cooptrails_ref.SATURATED == ct.LLE_COOPTRAILS_SATURATED
    assert C.sizeof(ct.UpdateArgs) == C.sizeof(lle_amd.cooperation.UpdateArgs)
    assert cooptrails.compiled_kernels() == KERNELS
    assert cooptrails.launched_kernels() == []


def test_build_list_and_entry_check_name_the_library():
    build = open(os.path.join(ROOT, "lle_amd", "build.py")).read()
    assert '("cooptrails", "liblle_cooptrails.so")' in build
    assert build.index('("coop", "liblle_coop.so")') < build.index('("cooptrails", "liblle_cooptrails.so")')  # it links against liblle_coop.so
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "cooptrails.EXPORTS" in entry and "liblle_cooptrails.so does not export" in entry
    makefile = open(os.path.join(ROOT, "lle_amd", "cooptrails", "Makefile")).read()
    assert "-llle_coop -llle_hip" in makefile and "ARCH ?= gfx950" in makefile
    needed = subprocess.run(["readelf", "-d", cooptrails.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "liblle_coop.so" in needed and "liblle_hip.so" in needed and "$ORIGIN" in needed


def test_lazy_name_and_arguments():
    assert lle_amd.TemporalCooperationTracker is cooptrails.TemporalCooperationTracker and "TemporalCooperationTracker" in lle_amd.__all__
    assert issubclass(cooptrails.TemporalCooperationTracker, lle_amd.CooperationTracker)
    tracker = object.__new__(cooptrails.TemporalCooperationTracker)  # (the queries refuse their arguments before they touch the device)
    for length in (-1, 0, 1):
        with pytest.raises(ValueError, match="at least 2"):
            tracker.is_sequential(length)
    with pytest.raises(ValueError, match="saturate"):
        tracker.is_sequential(16)
    with pytest.raises(NotImplementedError):
        tracker.is_interdependent(3)
    tracker.th = tracker.h = None
    with pytest.raises(ValueError, match="temporal"):
        lle_amd.BatchedLLE.__init__(object.__new__(lle_amd.BatchedLLE), "S0 X", 1, cooperation="flattened", device="cpu")


def test_host_side_refusals():
    L = cooptrails.lib()
    assert L.lle_cooptrails_update(None, None, None) == -1 and b"NULL" in L.lle_cooptrails_last_error()
    assert L.lle_cooptrails_update_map(None, 0, None) == -1
    assert L.lle_cooptrails_buffer(None, 0) is None
    assert L.lle_cooptrails_create(None, None, None) is None  # (no device here, or NULL handles there: refused either way)
    assert L.lle_cooptrails_last_error() != b""
    L.lle_cooptrails_free(None)
