"""Reward shaping and laser-subgoal extras without a GPU: the reference's own tests (tests/golden/kat_shaping.json) on the numpy
restatement (tests/oracle_shaping.py), header / exports / binding of liblle_shaping.so, the cell table against the laser listings,
the descriptors' validation, the Builder's refusals, the refusal without a device and the ISA tripwire on the shaping kernel's
translation unit.  The kernel itself is compared on the MI355X (tests/test_gpu_shaping.py)."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import lle_amd
from lle_amd import (BatchedLLE, LaserSubgoal, Map, MultiGenerator, MultiObjective, NoExtras, PotentialShapedLLE, SingleObjective, shaping)
from oracle.levels import LEVELS
from tests import oracle_shaping
from tests.parity_util import EXTRA_MAPS, LONG_MAPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = oracle_shaping.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_shaping_kat_on_restatement(oracle_mod, case):
    oracle_shaping.run_case(lambda c: oracle_shaping.OracleAdapter(c, oracle_mod), case)


def test_kat_file_is_what_the_maker_writes(tmp_path):
    spec = importlib.util.spec_from_file_location("make_kat_shaping", os.path.join(ROOT, "tests", "golden", "make_kat_shaping.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.CASES == CASES and all(c["ref"].startswith("python/tests/") for c in CASES)


def test_library_exports():
    """liblle_shaping.so exports every function include/lle_shaping.h declares, and the binding knows exactly those; the header is
    plain C and is the one the library is compiled against; the struct layouts of the binding are the header's."""
    L = shaping.lib()
    header = open(os.path.join(ROOT, "include", "lle_shaping.h")).read()
    declared = set(re.findall(r"\b(lle_shaping_[a-z_0-9]+)\s*\(", header))
    assert declared == set(shaping.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    res = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I" + os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "include", "lle_shaping.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert '#include "../../include/lle_shaping.h"' in open(os.path.join(ROOT, "lle_amd", "shaping", "shaping.hip")).read()
    import ctypes as C
    prog = ('#include <stdio.h>\n#include "lle_shaping.h"\nint main(void) { printf("%zu %zu %d %d %d %d %d %d", sizeof(lle_shaping_config), '
            'sizeof(lle_shaping_update_args), LLE_SHAPING_CLEAR, LLE_SHAPING_MARK_STARTS, LLE_SHAPING_MARK_POS, LLE_SHAPING_HONOUR_AUTO_RESET, '
            'LLE_SHAPING_MAX_COLS, LLE_SHAPING_MAX_REPEATS); return 0; }\n')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(shaping.ShapingConfig), C.sizeof(shaping.UpdateArgs), shaping.LLE_SHAPING_CLEAR, shaping.LLE_SHAPING_MARK_STARTS,
                   shaping.LLE_SHAPING_MARK_POS, shaping.LLE_SHAPING_HONOUR_AUTO_RESET, shaping.LLE_SHAPING_MAX_COLS, shaping.LLE_SHAPING_MAX_REPEATS]
    assert sorted(shaping.compiled_kernels()) == sorted(f"shaping_kernel<{g},{t}>" for g in (1, 2, 4, 8, 16) for t in ("false", "true"))


def _all_maps():
    maps = {f"level{k}": LEVELS[k] for k in range(1, 7)}
    maps.update(EXTRA_MAPS)
    maps.update(LONG_MAPS)
    maps.update(oracle_shaping.SHAPING_MAPS)
    return maps


@pytest.mark.parametrize("name", sorted(_all_maps()))
def test_cell_masks_equal_the_laser_listings(oracle_mod, name):
    """lle_shaping_cell_masks == {cell: sources that own a tile there} derived from Map.laser_tiles(), from the first two depths of
    Map.cell_layers(), and from the oracle's own World.lasers listing."""
    text = _all_maps()[name]
    m = Map(text)
    got = shaping.cell_masks(m)
    assert len(got) == m.height * m.width
    want = [0] * (m.height * m.width)
    for t in m.laser_tiles():
        want[t.i * m.width + t.j] |= 1 << t.laser_id
    assert got == want
    layers = [0] * (m.height * m.width)
    for c in m.cell_layers():
        if c.depth < 2:
            layers[c.i * m.width + c.j] |= 1 << c.laser_id
    assert got == layers
    listing = [0] * (m.height * m.width)
    for (i, j, laser_id, _agent, _on, _enabled) in oracle_mod.OracleWorld(text).lasers():
        listing[i * m.width + j] |= 1 << laser_id
    assert got == listing
    assert any(got) == (m.n_laser_tiles > 0), name


def test_three_beam_cell_drops_the_third_source():
    """World.lasers (src/core/world.rs:159-172) lists the outer laser layer of a cell and the one directly below it: on a cell under
    three beams the deepest source owns no tile, in the reference's extras and potential as here."""
    m = Map(oracle_shaping.SHAPING_MAPS["three_beam_cell"])
    at = sorted((c.depth, c.laser_id) for c in m.cell_layers() if (c.i, c.j) == (2, 2))
    assert [d for d, _ in at] == [0, 1, 2] and len({l for _, l in at}) == 3
    mask = shaping.cell_masks(m)[2 * m.width + 2]
    assert mask == (1 << at[0][1]) | (1 << at[1][1])
    assert not (mask >> at[2][1]) & 1, "the third source must be missing from the cell"
    # ... while the same source owns its other tiles
    assert any((v >> at[2][1]) & 1 for v in shaping.cell_masks(m))
    four = Map(EXTRA_MAPS["four_layers"])
    assert bin(shaping.cell_masks(four)[2 * four.width + 2]).count("1") == 2


def test_cell_masks_ignore_colours_and_exits():
    m = Map(LEVELS[6])
    before = shaping.cell_masks(m)
    for s in m.sources():
        m.set_source(s.laser_id, enabled=0, agent_id=(s.agent_id + 1) % m.n_agents if m.colour_allowed(s.laser_id, (s.agent_id + 1) % m.n_agents) else None)
    assert shaping.cell_masks(m) == before


def test_descriptors():
    m = Map("S0 . .\n. . L0W\n. . L0W\nX . .")
    assert PotentialShapedLLE(SingleObjective()).objectives == ("reward",)
    assert PotentialShapedLLE(MultiObjective()).objectives == ("gem", "exit", "death", "done", "PBRS")
    p = PotentialShapedLLE(SingleObjective(), m, 0.9, 0.3, [(1, 2)])
    assert (p.gamma, p.reward_value, p.laser_ids(None)) == (0.9, 0.3, [0])
    assert PotentialShapedLLE(SingleObjective(), m).laser_ids(None) == [0, 1]
    assert PotentialShapedLLE(SingleObjective(), None, lasers_to_reward=[(2, 2), (1, 2), (2, 2)]).laser_ids(m) == [1, 0, 1]
    d = PotentialShapedLLE(SingleObjective())
    assert (d.gamma, d.reward_value, d.world, d.lasers_to_reward) == (0.99, 0.5, None, None)  # the reference's defaults (builder.py:78-84)
    src = m.sources()[1]
    assert LaserSubgoal(m, [src]).columns(None) == [(1, "Source 1 at (2, 2)")]
    assert LaserSubgoal().columns(m) == [(0, "Source 0 at (1, 2)"), (1, "Source 1 at (2, 2)")]
    assert LaserSubgoal(world="S0 L0E . X").columns(None) == [(0, "Source 0 at (0, 1)")]
    assert MultiGenerator(LaserSubgoal(m, [(2, 2)]), NoExtras(), "laser_subgoal").columns(m) == [
        (1, "Source 1 at (2, 2)"), (0, "Source 0 at (1, 2)"), (1, "Source 1 at (2, 2)")]
    assert NoExtras().columns(m) == []
    with pytest.raises(ValueError, match=r"Tile at position \(0, 1\) is not a laser source"):
        PotentialShapedLLE(SingleObjective(), m, lasers_to_reward=[(0, 1)])
    with pytest.raises(IndexError, match="Position out of bounds"):
        LaserSubgoal(m, [(9, 0)])
    with pytest.raises(ValueError, match="Invalid laser source"):
        LaserSubgoal(m, ["north"])
    with pytest.raises(ValueError, match="Invalid extra type: 3"):
        MultiGenerator(LaserSubgoal(), 3)
    with pytest.raises(ValueError, match="Invalid extra type: subgoals"):
        MultiGenerator("subgoals")
    with pytest.raises(ValueError):
        PotentialShapedLLE(PotentialShapedLLE(SingleObjective()))
    with pytest.raises(ValueError):
        PotentialShapedLLE("single")


def test_builder_still_refuses_and_points_at_the_way_in():
    with pytest.raises(NotImplementedError, match="reward_strategy=PotentialShapedLLE"):
        lle_amd.level(1).pbrs()
    with pytest.raises(NotImplementedError, match="extras_generator="):
        lle_amd.level(1).add_extras("laser_subgoal")
    assert isinstance(lle_amd.level(1).add_extras(), lle_amd.Builder)
    import inspect
    params = inspect.signature(lle_amd.Builder.build).parameters
    assert "reward_strategy" in params and "extras_generator" in params
    params = inspect.signature(BatchedLLE.__init__).parameters
    assert params["reward_strategy"].default is None and params["extras_generator"].default is None


def test_create_without_a_device_is_refused_with_a_message():
    import torch
    L = shaping.lib()
    assert L.lle_shaping_create(None, None, 0, None, None) is None
    msg = L.lle_shaping_last_error().decode()
    assert msg
    if not torch.cuda.is_available():
        assert "no HIP device" in msg
        with pytest.raises(RuntimeError, match="no HIP device"):
            BatchedLLE(LEVELS[1], 4, reward_strategy=PotentialShapedLLE(SingleObjective()), extras_generator="laser_subgoal")
    assert L.lle_shaping_update(None, None, None) != 0 and L.lle_shaping_cell_masks(None, None, 0) < 0
    assert L.lle_shaping_reached(None, 0) is None


def test_shaping_translation_unit_isa_scan():
    spec = importlib.util.spec_from_file_location("isa_exec_copy_scan", os.path.join(ROOT, "tools", "isa_exec_copy_scan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text = mod.asm_of(os.path.join(ROOT, "lle_amd", "shaping", "shaping.hip"))
    assert "shaping_kernel" in text
    assert mod.scan(text) == []
    # the count is summed with cross-lane reads inside the wavefront: no atomics, and LDS traffic only for the cell table
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic", text) and not re.search(r"\bds_(add|sub|inc)", text)
