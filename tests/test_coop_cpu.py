"""The cooperation tracker without a GPU: the reference's own tests (tests/golden/kat_coop.json) on the host graph class
(lle_amd.characterization) and on the restatement of the rule over oracle worlds (tests/coop_ref.py), the cell table of liblle_coop.so
against the laser listings, header / exports / binding.  The kernel itself is compared on the MI355X (tests/test_gpu_coop.py,
tests/test_gpu_coop_states.py)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

from lle_amd import Map, cooperation
from lle_amd.characterization import DependencyEdge, PlanProfile, TemporalCooperationGraph
from oracle.levels import LEVELS
from tests import coop_ref, coopcycles_ref, cooptrails_ref, source_text
from tests.oracle_shaping import SHAPING_MAPS
from tests.parity_util import EXTRA_MAPS, LONG_MAPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = coop_ref.load_cases()


def test_kat_file_is_what_the_maker_writes():
    spec = importlib.util.spec_from_file_location("make_kat_coop", os.path.join(ROOT, "tests", "golden", "make_kat_coop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.GRAPHS == CASES["graphs"] and mod.WORLDS == CASES["worlds"]
    assert all(c["ref"].startswith("python/tests/") for c in CASES["graphs"] + CASES["worlds"])


@pytest.mark.parametrize("case", CASES["graphs"], ids=[c["name"] for c in CASES["graphs"]])
def test_graph_kat_on_the_host_class(case):
    graph = TemporalCooperationGraph([DependencyEdge(h, b, t) for h, b, t in case["edges"]])
    coop_ref.check_graph(graph, case["expect"])
    assert isinstance(graph.profile(), PlanProfile)


@pytest.mark.parametrize("case", CASES["worlds"], ids=[c["name"] for c in CASES["worlds"]])
def test_world_kat_on_the_restatement(oracle_mod, case):
    """coop_ref.detect replayed on the oracle reproduces the edges and properties the reference asserts for the world."""
    world = oracle_mod.OracleWorld(case["map"])
    edges = coop_ref.replay(world, case["plan"])
    if "edges_t0" in case["expect"]:
        assert {(h, b) for h, b, t in edges if t == 0} == {tuple(e) for e in case["expect"]["edges_t0"]}
    coop_ref.check_graph(TemporalCooperationGraph([DependencyEdge(*e) for e in edges]), case["expect"])
    assert all(world.arrived()) or not case["plan"], "a hand-written plan must solve its world"


def test_flattened_profile_of_the_restatement():
    ring = {(h, (h + 1) % 8) for h in range(8)}
    assert coop_ref.profile(ring, 1) == [8, 8, 1, 1, 0, 1, 0, 1]
    assert coop_ref.profile({(0, 1), (0, 2), (3, 2)}, 300) == [3, 4, 2, 2, 3, 255, 0, 1]
    assert coop_ref.profile({(0, 1), (1, 0), (1, 2)}) == [3, 3, 1, 2, 0, 0, 0, 1]
    assert coop_ref.profile(set(), 0, valid=False) == [0] * 8
    assert coop_ref.edges_of(coop_ref.rows(ring, 8)) == ring
    # the profile's degree bytes are the graph class's queries on the same edges
    for edges in (ring, {(0, 1), (0, 2), (3, 2)}, {(0, 1), (1, 0), (1, 2)}, set()):
        g = TemporalCooperationGraph([DependencyEdge(h, b, 0) for h, b in edges])
        p = coop_ref.profile(edges)
        assert p[:5] == [len(g.flattened_edges()), g.n_vertices, g.max_distinct_helpers(), g.max_distinct_beneficiaries(), len(g.asymmetric_edges())]


def test_env_ref_operations():
    r = coop_ref.EnvRef(3)
    r.update(0)
    assert r.arrays() == ([0, 0, 0], [0, 0, 0], [0, 0, 0], [0] * 8, [0] * 8)
    r.update(coop_ref.MARK_POS, {(0, 1)})
    r.update(coop_ref.MARK_POS, {(1, 2)})
    assert r.arrays() == ([0, 4, 0], [2, 4, 0], [0, 0, 0], [2, 3, 1, 1, 1, 2, 0, 1], [0] * 8)
    r.update(coop_ref.MARK_POS, set(), start_edges={(2, 0)}, was_reset=True)
    assert r.arrays() == ([0, 0, 0], [0, 0, 1], [2, 4, 0], [1, 2, 1, 1, 1, 1, 0, 1], [2, 3, 1, 1, 1, 2, 0, 1])
    r.update(coop_ref.FINISH | coop_ref.CLEAR)
    assert r.arrays()[1:] == ([0, 0, 0], [0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1], [1, 2, 1, 1, 1, 1, 0, 1])


def _all_maps():
    maps = {f"level{k}": LEVELS[k] for k in range(1, 7)}
    maps.update(EXTRA_MAPS)
    maps.update(LONG_MAPS)
    maps.update(SHAPING_MAPS)
    maps.update({c["name"]: c["map"] for c in CASES["worlds"]})
    return maps


@pytest.mark.parametrize("name", sorted(_all_maps()))
def test_cell_masks_equal_the_laser_listings(oracle_mod, name):
    """lle_coop_cell_masks == {cell: sources that own a tile there} from lle_map_laser_tiles and from the oracle's World.lasers."""
    text = _all_maps()[name]
    m = Map(text)
    got = cooperation.cell_masks(m)
    assert len(got) == m.height * m.width
    want = [0] * (m.height * m.width)
    for t in m.laser_tiles():
        want[t.i * m.width + t.j] |= 1 << t.laser_id
    assert got == want
    listing = [0] * (m.height * m.width)
    for (i, j, laser_id, _agent, _on, _enabled) in oracle_mod.OracleWorld(text).lasers():
        listing[i * m.width + j] |= 1 << laser_id
    assert got == listing


def test_three_beam_cell_drops_the_third_source():
    """World.lasers lists the outer laser layer of a cell and the one directly below it: the third source owns no tile on the cell."""
    m = Map(SHAPING_MAPS["three_beam_cell"])
    at = sorted((c.depth, c.laser_id) for c in m.cell_layers() if (c.i, c.j) == (2, 2))
    assert [d for d, _ in at] == [0, 1, 2] and len({l for _, l in at}) == 3
    masks = cooperation.cell_masks(m)
    assert masks[2 * m.width + 2] == (1 << at[0][1]) | (1 << at[1][1])
    assert any((v >> at[2][1]) & 1 for v in masks), "the third source owns its other tiles"


def test_library_exports():
    """liblle_coop.so exports every function include/lle_coop.h declares, and the binding knows exactly those; the header is plain C
    and the one the library is compiled against; struct size and enum values of the binding are the header's."""
    L = cooperation.lib()
    header = open(os.path.join(ROOT, "include", "lle_coop.h")).read()
    declared = set(re.findall(r"\b(lle_coop_[a-z_0-9]+)\s*\(", header))
    assert declared == set(cooperation.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    assert '#include "../../include/lle_coop.h"' in source_text.text_of(os.path.join("lle_amd", "coop", "coop.hip"))
    prog = ('#include <stdio.h>\n#include "lle_coop.h"\nint main(void) { printf("%zu %d %d %d %d %d %d %d %d %d", sizeof(lle_coop_update_args), '
            'LLE_COOP_FINISH, LLE_COOP_CLEAR, LLE_COOP_MARK_STARTS, LLE_COOP_MARK_POS, LLE_COOP_HONOUR_AUTO_RESET, LLE_COOP_ENV_SOURCES, '
            'LLE_COOP_EPISODE_EDGES, LLE_COOP_LAST_PROFILE, LLE_COOP_BUF_COUNT); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(cooperation.UpdateArgs), cooperation.LLE_COOP_FINISH, cooperation.LLE_COOP_CLEAR, cooperation.LLE_COOP_MARK_STARTS,
                   cooperation.LLE_COOP_MARK_POS, cooperation.LLE_COOP_HONOUR_AUTO_RESET, cooperation.LLE_COOP_ENV_SOURCES,
                   cooperation.LLE_COOP_EPISODE_EDGES, cooperation.LLE_COOP_LAST_PROFILE, 5]
    assert sorted(cooperation.compiled_kernels()) == sorted(f"coop_kernel<{g},{t}>" for g in (1, 2, 4, 8, 16) for t in ("false", "true"))
    assert cooperation.launched_kernels() == []


def test_episode_ops_under_sanitizers(tmp_path):
    """tests/hostsim/episode_ops.cpp: its own main over lle_amd/coop/episode_ops.hpp, built with g++ -fsanitize=address,undefined and
    run as a child process; nothing sanitized is loaded into this interpreter.  Every decode case goes to it as text: 16 operation
    words x HONOUR_AUTO_RESET x SKIP_REFUSED x bit 7 of the event count x the error byte, 256 in all, with the operations of stages
    0, 1 and 2 by the order EnvRef.update of tests/cooptrails_ref.py and tests/coopcycles_ref.py implements: the auto-reset's phase,
    then the caller's, MARK_POS last inside a phase.  The layout function is judged on what the program prints: the properties
    include/lle_coop.h promises for a handle's arrays."""
    FINISH, CLEAR, MARK_STARTS, MARK_POS = cooptrails_ref.FINISH, cooptrails_ref.CLEAR, cooptrails_ref.MARK_STARTS, cooptrails_ref.MARK_POS
    assert (FINISH, CLEAR, MARK_STARTS, MARK_POS) == (coopcycles_ref.FINISH, coopcycles_ref.CLEAR, coopcycles_ref.MARK_STARTS, coopcycles_ref.MARK_POS)
    exe, cases = str(tmp_path / "episode_ops"), str(tmp_path / "cases.txt")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "episode_ops.cpp"), "-o", exe,
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"], check=True)
    layouts = [[1], [255], [256], [257], [1, 255, 256, 257], [4096 * 8, 4096 * 8, 4096 * 4, 4096 * 4], [7 * 4 * 21, 7 * 4 * 21, 28, 28]]
    n_cases = unread = 0
    with open(cases, "w") as f:
        for ops in range(16):
            for honour in (0, 1):
                for skip in (0, 2):
                    for evcount in (0x7F, 0x85):
                        for err in (0, 3):
                            was_reset, refused = bool(honour and evcount & 0x80), bool(skip and err)
                            phases = ([FINISH | CLEAR | MARK_STARTS] if was_reset else []) + [ops & ~MARK_POS if refused else ops]  # EnvRef.update
                            stages = [phases[0] if was_reset else 0, phases[-1] & ~MARK_POS, phases[-1] & MARK_POS]
                            for ref in (cooptrails_ref.EnvRef(2), coopcycles_ref.EnvRef(2)):  # what the restatements make of the same call
                                ref.update(ops, was_reset=was_reset, refused=refused)
                                assert ref.touched == bool(ops or was_reset) and (not ref.touched or ref.finished == any(s & FINISH for s in stages))
                            f.write("ops " + " ".join(format(v, "x") for v in [ops, honour | skip, evcount, err] + stages) + "\n")
                            n_cases, unread = n_cases + 1, unread + (not honour) + (not skip)
        for sizes in layouts:
            f.write(f"layout {len(sizes)} " + " ".join(str(s) for s in sizes) + "\n")
    assert n_cases == 256
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    res = subprocess.run([exe, cases], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
    assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
    lines = res.stdout.splitlines()
    assert lines[-1] == f"OK decoded=256 layouts={len(layouts)} unread={unread}" and len(lines) == len(layouts) + 1
    guard = 256  # LLE_COOP_GUARD_BYTES
    for sizes, line in zip(layouts, lines):
        got = [int(v) for v in line.split()[1:]]
        k, offsets, total = got[0], got[1:-1], got[-1]
        assert k == len(sizes) == len(offsets)
        assert all(o % guard == 0 for o in offsets) and offsets[0] >= guard                     # every array on a 256-byte boundary, a guard in front
        assert all(offsets[i + 1] - (offsets[i] + sizes[i]) >= guard for i in range(k - 1))    # a guard between an array's end and the next one's start
        assert total - (offsets[-1] + sizes[-1]) >= guard and total % guard == 0                # a guard behind the last
        assert total <= sum(sizes) + (2 * k + 1) * guard                                        # and no more than rounding plus the guards


def test_host_side_refusals():
    L = cooperation.lib()
    assert L.lle_coop_cell_masks(None, None, 0) == -1 and b"NULL" in L.lle_coop_last_error()
    assert L.lle_coop_update(None, None, None) == -1
    assert L.lle_coop_update_map(None, 0, None, None) == -1
    assert L.lle_coop_buffer(None, 0) is None
    assert L.lle_coop_start_edges(None, 0, None, 0) == -1
    L.lle_coop_free(None)
