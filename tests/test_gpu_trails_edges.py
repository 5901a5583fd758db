"""The trail search on the MI355X where tests/test_gpu_trails.py does not reach: trail fields above 7, the boundary between N = 15 and
N = 16, a frontier that runs empty because every trajectory reaches N, pools that fit exactly and a handle that goes on after a refusal,
cells behind the first 256 of the cell table, and worlds changed before the solver is constructed.

Every comparison is exact and is `assert_recorded` of tests/test_gpu_trails.py: length, per-depth frontier and expanded counters and
stored records against tests/golden/kat_trails.json, which tests/test_trails_cpu.py holds the restatement (tests/trails_ref.py) to; every
plan replayed on the oracle under its N and the entry's `changes`; the goal's trail word equal to the replay's L.  No test here walks a
search in Python.

The smallest shapes at which these can go wrong:
  long-trails (4 x 6, 2 agents, t_max 24)
        two-agent-mutual-compact without reachable exits.  The agents hold the mutual pair over STAYs until some trail has N edges: for
        every N in 2 .. 16 no plan, 100 + 76 (N - 2) records (1088 at N = 15, 1164 at N = 16), a greatest stored field of N - 1 and an
        empty frontier at depth N + 5.  Every N has counters of its own, so a field clipped at 7 or 8, a stack of the walk shifted wrongly
        or an N compared off by one gives the counters of another N, or of none.  The largest level has 76 records, 1 900 work items:
        30 pieces of 64.
  max_states = 1164 | 1163 on it
        the pool that fits N = 16 exactly and the one that is a record short; the refused handle answers N = 15 and N = 2.
  20 x 20, 64 x 64, 65 x 66, 6 x 255, 255 x 6 around long-trails and chain-in-one-state
        400 cells: a second, partial pass of the staging loop of stride 256; 4 096 cells: the largest table that goes to LDS; 4 290:
        global memory; 255: coordinate bytes of 253 and 254.  The layout lies in the bottom-right corner: every laser tile behind cell 256.
  two-agent-mutual-compact with source 1 disabled, source 0 disabled, source 1 recoloured, both disabled
        one layout, five worlds, five answers: the rule the solver froze at its construction decides.

NOT here: LLE_TRAILS_DENSE on the device.  No state was found, with six agents or fewer, whose walk exceeds the budget of 4 096
extensions: an agent can only help from the end of a beam segment and a cell has two layers of beams, so a state has at most about
14 arcs (a 2 x 3 block; 976 extensions if every layer counted), and the oracle keeps far fewer (7 arcs, 11 extensions on that block).
That is reasoning and two probes on the CPU, not a proof; the budget path stays covered by the stand-alone host program
(tests/hostsim/trails_logic.cpp under sanitizers), and no entry point for made-up states was added for it."""
import ctypes as C
import os
import re

import pytest

from tests import helpgraph_ref, trails_ref
from tests.test_gpu_trails import MAPS, SEARCHES, assert_recorded, recorded, run, search_id, tr, values  # noqa: F401  (tr: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG, COMPACT, T_LONG = "long-trails", "two-agent-mutual-compact", 24
CHUNK64 = dict(chunk=64, max_states=16384)
COUNTERS = ("length", "frontier", "expanded", "n_states")
OFF0 = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}]}
OFF1 = {"sources": [{"laser_id": 1, "enabled": False, "colour": None}]}
RECOLOUR1 = {"sources": [{"laser_id": 1, "enabled": None, "colour": 0}]}
ALL_OFF = {"sources": [{"laser_id": 0, "enabled": False, "colour": None}, {"laser_id": 1, "enabled": False, "colour": None}]}
CHANGED = [s for s in SEARCHES if "changes" in s]


def counters(stats):
    return {k: stats[k] for k in COUNTERS}


def want(s):
    return dict(length=s["length"], frontier=s["frontier"], expanded=s["expanded"], n_states=s["states"])


# ---------------------------------------------------------------------------------------------------------------- trail fields above 7
def test_the_recorded_searches_are_the_ones_this_file_needs():
    long_ = [s for s in SEARCHES if s["map"] == LONG and "changes" not in s]
    assert [(s["n"], s["t_max"], s["length"], s["states"], len(s["expanded"]), s["frontier"][-1]) for s in long_] == \
        [(n, T_LONG, None, 100 + 76 * (n - 2), n + 5, 0) for n in range(2, 17)]
    assert (recorded(LONG, 15)["states"], recorded(LONG, 16)["states"]) == (1088, 1164)
    assert max(recorded(LONG, 16)["frontier"]) * 25 == 1900 > 64 * 29, "the largest level: 30 pieces of 64 work items"
    assert [(s["map"], helpgraph_ref.changes_label(s["changes"]), s["n"]) for s in CHANGED] == \
        [(COMPACT, "-source1-off", 2), (COMPACT, "-source1-off", 3), (COMPACT, "-source0-off", 2), (COMPACT, "-source0-off", 3), (COMPACT, "-source1-colour0", 2),
         (COMPACT, "-source1-colour0", 3), (LONG, "-source1-off", 16), (COMPACT, "-source0-off-source1-off", 2), (COMPACT, "-source0-off-source1-off", 16)]
    four = [recorded(COMPACT, 2)] + [recorded(COMPACT, 2, changes=c) for c in (OFF1, OFF0, RECOLOUR1)]
    assert [(s["length"], s["states"]) for s in four] == [(None, 100), (5, 164), (5, 130), (None, 107)]


LONG_RUNS = [(n, "defaults") for n in range(2, 17)] + [(n, "chunk64") for n in (2, 8, 15, 16)]


@pytest.mark.parametrize("n, config", LONG_RUNS, ids=[f"n{n}-{c}" for n, c in LONG_RUNS])
def test_long_trails_for_every_n(tr, n, config):
    """No plan for any N; N + 5 levels, the last of which stores nothing; the counters of this N and of no other."""
    s = recorded(LONG, n)
    plan, stats = assert_recorded(tr, s, **({} if config == "defaults" else CHUNK64))
    assert plan is None and stats["length"] is None and stats["trail_lengths"] is None and stats["longest_trail"] is None
    assert len(stats["expanded"]) == n + 5, "depth_reached"
    assert len(stats["frontier"]) == n + 6 and stats["frontier"][-1] == 0, "what lle_trails_stats returns: the last level is empty"
    assert stats["n_states"] == 100 + 76 * (n - 2)


def test_the_result_struct_on_long_trails(tr):
    """One handle through the C ABI, N = 16, 15, 2 and 16 again: depth_reached = N + 5 < t_max, no trail word without a plan,
    lle_trails_stats returns N + 6 frontier entries, the last of them 0, and lle_trails_plan refuses."""
    from lle_amd import Map
    L = tr.lib()
    map_ = Map(MAPS[LONG])
    h = L.lle_trails_create(map_.h, C.byref(tr.TrailOptions(C.sizeof(tr.TrailOptions), -1, 64, 2048, None)))
    assert h, L.lle_trails_last_error()
    try:
        for n in (16, 15, 2, 16):
            s = recorded(LONG, n)
            res = tr.TrailResult(C.sizeof(tr.TrailResult))
            assert L.lle_trails_run(h, C.byref(tr.TrailArgs(C.sizeof(tr.TrailArgs), n, 0, T_LONG)), C.byref(res)) == 0, L.lle_trails_last_error()
            assert (res.length, res.n_states, res.depth_reached, res.trail, res.step_errors) == (-1, s["states"], n + 5, 0, 0)
            frontier, expanded = (C.c_int64 * 32)(), (C.c_int64 * 32)()
            assert L.lle_trails_stats(h, frontier, expanded, 32) == n + 6 and L.lle_trails_stats(h, None, None, 0) == n + 6
            assert list(frontier[:n + 6]) == s["frontier"] and frontier[n + 5] == 0 and list(expanded[:n + 5]) == s["expanded"]
            assert L.lle_trails_plan(h, (C.c_uint8 * 64)(), 64) == -2 and b"no plan" in L.lle_trails_last_error()
    finally:
        L.lle_trails_free(h)


# ---------------------------------------------------------------------------------------------------------------- exact fit
@pytest.mark.parametrize("chunk", [64, None], ids=["chunk64", "defaults"])
def test_a_pool_that_fits_exactly_and_one_that_is_a_record_short(tr, chunk):
    """max_states = 1164 = the records N = 16 stores: answered, with the recorded counters.  max_states = 1163: SolverCapacityError,
    nothing cached -- and the same handle then answers N = 15 (1088 records) and N = 2 with the recorded counters, and refuses N = 16
    again."""
    from lle_amd import SolverCapacityError
    options = {} if chunk is None else dict(chunk=chunk)
    assert recorded(LONG, 16)["states"] == 1164
    assert_recorded(tr, recorded(LONG, 16), max_states=1164, **options)
    s = tr.TrailSolver(MAPS[LONG], T_LONG, max_states=1163, **options)
    try:
        with pytest.raises(SolverCapacityError, match=r"max_states = 1163\b"):
            s.find_shortest("no-sequence-16")
        assert s._cache == {}
        for n in (15, 2):
            assert s.find_shortest(f"no-sequence-{n}") is None
            print(n, s.last_stats)
            assert counters(s.last_stats) == want(recorded(LONG, n)) and s.last_stats["trail_lengths"] is None
        assert len(s._cache) == 2
        with pytest.raises(SolverCapacityError, match=r"max_states = 1163\b"):
            s.find_shortest("no-sequence-16")
        assert len(s._cache) == 2
    finally:
        s.free()
    # the same on the other side of N = 15: 1088 fits it, 1087 does not
    assert_recorded(tr, recorded(LONG, 15), max_states=1088, **options)
    with pytest.raises(SolverCapacityError, match=r"max_states = 1087\b"):
        run(tr, MAPS[LONG], T_LONG, 15, max_states=1087, **options)


# ---------------------------------------------------------------------------------------------------------------- far corner
SIZES = [(20, 20), (64, 64), (65, 66), (6, 255), (255, 6)]
LDS_THREADS = 256  # TR_THREADS: cells staged per pass of the loop in tr_insert<true>
FAR = [(LONG, 16), (LONG, 3), ("chain-in-one-state", 2), ("chain-in-one-state", 3)]


def test_the_sizes_are_the_ones_the_table_turns_at():
    source = open(os.path.join(ROOT, "lle_amd", "trails", "trails.hip")).read()
    lds_max = int(re.search(r"LDS_TABLE_MAX_BYTES = (\d+);", source).group(1))
    assert int(re.search(r"TR_THREADS = (\d+);", source).group(1)) == LDS_THREADS and "table_bytes <= lle::LDS_TABLE_MAX_BYTES" in source
    assert "c < HW; c += TR_THREADS" in source, "the staging loop"
    assert 20 * 20 == LDS_THREADS + 144, "two passes of the staging loop, the second partial"
    assert 64 * 64 * 4 == lds_max == 16384, "the largest table that goes to LDS"
    assert 65 * 66 * 4 > lds_max and 65 * 66 - 1 == 4289, "global memory"
    assert 6 * 255 * 4 <= lds_max and max(max(s) for s in SIZES) == 255 and "#define LLE_MAX_DIM 255" in open(os.path.join(ROOT, "include", "lle_hip.h")).read()


@pytest.mark.parametrize("size", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("name", [LONG, "chain-in-one-state"])
def test_a_layout_in_the_far_corner(tr, name, size):
    """The layout in the bottom-right corner of a map of walls: every cell the search reads lies behind the first 256 of the table (at
    6 x 255 and 255 x 6 the coordinate bytes of agents on beams reach 253 and 254); counters are the small layout's, with a pool of one
    record more than the search stores."""
    from lle_amd import Map
    height, width = size
    big = helpgraph_ref.embed(MAPS[name], height, width)
    tiles = Map(big).laser_tiles()
    assert tiles and min(t.i * width + t.j for t in tiles) >= LDS_THREADS and max(t.i for t in tiles) >= height - 2
    assert max(t.j for t in tiles) >= width - (3 if name == LONG else 2)  # (long-trails keeps two columns of walls and exits to the right of its beams)
    for layout, n in FAR:
        if layout == name:
            s = recorded(name, n)
            assert_recorded(tr, s, text=big, chunk=256, max_states=s["states"] + 1)
    assert ("tr_insert<true>" if height * width * 4 <= 16384 else "tr_insert<false>") in tr.launched_kernels()


# ---------------------------------------------------------------------------------------------------------------- changed worlds
@pytest.mark.parametrize("config", ["defaults", "chunk64"])
@pytest.mark.parametrize("s", CHANGED, ids=[search_id(s) for s in CHANGED])
def test_changed_worlds(tr, s, config):
    """TrailSolver(apply_changes(World(text), changes), t_max): the recorded counters of the CHANGED world, the plan replayed on the
    oracle under the same changes."""
    _plan, stats = assert_recorded(tr, s, **({} if config == "defaults" else CHUNK64))
    if s["changes"] == ALL_OFF:
        assert stats["trail_lengths"] == [0, 0]


def test_the_sources_are_frozen_at_construction(tr):
    """A source disabled on the World after TrailSolver(world, t) was constructed does not reach that solver (its handle is made by the
    first search, later still); a solver constructed afterwards answers for the changed world."""
    from lle_amd import World
    before, after = recorded(COMPACT, 2), recorded(COMPACT, 2, changes=OFF1)
    assert (before["t_max"], before["length"], before["states"], after["length"], after["states"]) == (6, None, 100, 5, 164) and after["length"] <= 6
    world = World(MAPS[COMPACT])
    first = tr.TrailSolver(world, 6)
    trails_ref.apply_changes(world, OFF1)
    second = tr.TrailSolver(world, 6)
    try:
        assert first.find_shortest("no-sequence-2") is None and counters(first.last_stats) == want(before)
        plan = values(second.find_shortest("no-sequence-2"))
        assert counters(second.last_stats) == want(after)
        assert tuple(second.last_stats["trail_lengths"]) == trails_ref.check_plan(MAPS[COMPACT], plan, 2, length=5, changes=OFF1)
    finally:
        first.free()
        second.free()


def test_with_every_source_disabled_every_n_is_the_plain_search(tr):
    """two-agent-mutual-compact with both sources disabled: nobody can help anybody, so no-sequence-2 and no-sequence-16 store what
    Solver.find_shortest() stores on the same changed world -- which is what the restatement recorded."""
    from lle_amd import Solver, World
    text = MAPS[COMPACT]
    plain = Solver(trails_ref.apply_changes(World(text), ALL_OFF), 8)
    try:
        assert len(plain.find_shortest()) == 5
        stored = counters(plain.last_stats)
    finally:
        plain.free()
    for n in (2, 16):
        s = recorded(COMPACT, n, changes=ALL_OFF)
        assert stored == want(s) and s["states"] == 151
        plan, stats = run(tr, text, 8, n, changes=ALL_OFF)
        print(n, stats)
        assert counters(stats) == stored and stats["trail_lengths"] == [0, 0] and stats["longest_trail"] == 0
        assert trails_ref.check_plan(text, plan, n, length=5, changes=ALL_OFF) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- characterizer
def test_characterizer_on_an_unsolvable_and_on_a_changed_world(tr):
    """long-trails has no plan at all, so nothing about it is sequential; two-agent-mutual-compact is sequential(2) as its text gives
    it and is not once source 1 is disabled."""
    from lle_amd import World
    c = tr.TrailCharacterizer(World(MAPS[LONG]), T_LONG)
    try:
        assert c.is_solvable() is False and c.is_sequential(2) is False and c.is_sequential(16) is False
        assert c.compute_shortest_path_without_sequence(16) is None and counters(c._solver.last_stats) == want(recorded(LONG, 16))
    finally:
        c._solver.free()
    unchanged, changed = tr.TrailCharacterizer(World(MAPS[COMPACT]), 8), tr.TrailCharacterizer(trails_ref.apply_changes(World(MAPS[COMPACT]), OFF1), 8)
    try:
        assert unchanged.is_solvable() and unchanged.is_sequential(2) is True
        assert changed.is_solvable() and changed.is_sequential(2) is False
        plan = values(changed.compute_shortest_path_without_sequence(2))
        assert counters(changed._solver.last_stats) == want(recorded(COMPACT, 2, changes=OFF1))
        assert max(trails_ref.check_plan(MAPS[COMPACT], plan, 2, length=5, changes=OFF1)) < 2
    finally:
        unchanged._solver.free()
        changed._solver.free()


def test_every_kernel_was_launched(tr):
    """At the end of this file: the far-corner sizes have gone through both insert kernels."""
    assert sorted(tr.launched_kernels()) == sorted(tr.compiled_kernels()) == ["tr_commit", "tr_expand", "tr_insert<false>", "tr_insert<true>"]
