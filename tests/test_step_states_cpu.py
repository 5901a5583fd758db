"""Steps from set states over every joint action (tests/step_states.py) on the host builds of the device state machines.

The protocol of tests/test_gpu_step_states.py -- set_state, the explicit step, two sampled steps, one with auto-reset -- on tests/hostsim
with all three engines (step_logic.hpp; step_lanes.hpp with and without its no-op-pass shortcut) against the oracle, every env
compared after every step.  The coverage assertions live here: a generator that lost a class fails on the CPU, before a GPU is
booked.  Every class is decided from the oracle's events and dumps."""
import functools

import numpy as np
import pytest

from tests import step_states as ss
from tests.parity_util import assert_set_state_events, assert_state_equal, assert_step_equal, legal_colours, unpack_engine

ENGINES = ["env", "lanes", "lanes_no_shortcut"]
PER_ENV_MAPS = ["q1", "nested", "four_layers", "long_crossing", "im_7_7x", "many_agents"]


@functools.lru_cache(maxsize=None)
def _reference(name):
    from oracle import oracle
    oracle.build()
    return ss.reference_run(oracle, ss.build_case(name))


def _bufs(sb):
    return {k: sb.buf(k) for k in ("pos", "bits", "gems", "beams", "avail", "actions", "err", "evcount", "events", "obs")}


def _load_requests(sb, case):
    from lle_amd import _decode
    sb.buf("req_pos")[:] = case.pos
    sb.buf("req_gems")[:] = [_decode.pack_bits(g) for g in case.gems]
    sb.buf("req_alive")[:] = [_decode.pack_bits(a) for a in case.alive]


def _run_protocol(sb, ref, tag, env_offset=ss.ENV_OFFSET):
    """The engine's side of the protocol against a Reference: every env, every field, after every step."""
    from lle_amd import _capi
    ob, case = ref.ob, ref.case
    _load_requests(sb, case)
    sb.set_state()
    assert not sb.buf("err").any(), f"{tag}: set_state refused envs {np.nonzero(sb.buf('err'))[0][:8].tolist()} the oracle accepts"
    eng = unpack_engine(_bufs(sb), *ob.dims)
    assert_state_equal(eng, ref.after_set_state["dump"], f"{tag} after set_state")
    assert_set_state_events(eng, ref.after_set_state, f"{tag} after set_state")
    assert np.array_equal(sb.buf("done"), ref.after_set_state["done"]), f"{tag}: done after set_state"
    assert np.array_equal(eng["obs"], ref.after_set_state["obs"]), f"{tag}: observation after set_state"
    stats0 = sb.buf("stats").copy()
    for rec in ref.steps:
        where = f"{tag} t={rec['t']}"
        if rec["actions"] is not None:
            sb.step(rec["actions"])
        else:
            flags = _capi.LLE_STEP_SAMPLE_ACTIONS | (_capi.LLE_STEP_AUTO_RESET if rec["auto_reset"] else 0)
            sb.step(None, flags=flags, seed=ss.SEED, t=rec["t"], env_offset=env_offset)
        eng = unpack_engine(_bufs(sb), *ob.dims)
        assert_step_equal(eng, rec["ostep"], where)
        assert_state_equal(eng, rec["dump"], where)
        assert np.array_equal(sb.buf("done"), rec["done"]), f"{where}: done"
        stats = sb.buf("stats").copy()
        want = rec["reward"].sum(0)
        got = stats[2:5] - stats0[2:5]
        assert np.array_equal(got, want[:3]), f"{where}: gem / exit / death counters {got.tolist()} != {want[:3].tolist()}"
        assert stats[7] - stats0[7] == want[0] + want[1] - want[2] + want[3], f"{where}: reward sum"
        assert stats[5] - stats0[5] == int((rec["ostep"]["err"] != 0).sum()) and stats[6] - stats0[6] == int((rec["ostep"]["ev_count"] >> 7).sum()), where
        stats0 = stats


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", ss.MAP_NAMES)
def test_steps_from_set_states(name, engine):
    from tests import hostsim

    ref = _reference(name)
    sb = hostsim.SimBatch(ref.case.text, ref.case.n)
    sb.set_engine(engine)
    _run_protocol(sb, ref, f"{name} {engine}")
    assert ref.ob.world(0).panics()[0] == 0


@pytest.mark.parametrize("name", PER_ENV_MAPS)
def test_steps_from_set_states_with_per_env_sources(oracle_mod, name):
    """Per-environment colours and enabled flags first (lle_batch_set_sources): a state is then accepted or refused by the env's OWN
    world, and a refused one is replaced for that env."""
    from tests import hostsim
    from tests.test_gpu_env_sources import Mirror

    case = ss.build_case(name)
    sb = hostsim.SimBatch(case.text, case.n)
    sb.set_engine("lanes")
    L = sb.map.n_sources
    rng = np.random.default_rng(len(name))
    colours = legal_colours(sb.map, rng.integers(0, case.A, size=(case.n, L), dtype=np.uint8))
    enabled = rng.integers(0, 1 << L, size=case.n, dtype=np.int64)
    sb.set_sources(colours, enabled.astype(np.uint32))
    ref = ss.reference_run(oracle_mod, case, sources=lambda ob: Mirror(ob, case.n, L).apply(colours, enabled, None), rng=rng)
    _run_protocol(sb, ref, f"{name} per-env sources")
    assert (ref.steps[0]["ostep"]["err"] == 0).mean() >= 0.5


@functools.lru_cache(maxsize=None)
def _coverage(name):
    ref = _reference(name)
    rec = ref.steps[0]
    flags = ss.classify(ref.case, ss.Geometry(ref.ob.world0), ref.after_set_state["dump"], rec["ostep"], rec["dump"])
    return {k: int(v.sum()) for k, v in flags.items()}


@pytest.mark.parametrize("name", ss.MAP_NAMES)
def test_coverage_of_every_map(name):
    """Per map: the batch is ragged and below 8 192 envs, at least half of its envs step, every agent is the lowest offender of a
    refusal somewhere, and the classes only this map can show are there -- after truncation."""
    case, cov = _reference(name).case, _coverage(name)
    assert case.n % 16 == 5 and case.n < ss.MAX_ENVS
    assert 2 * cov["stepped"] >= case.n, (name, cov["stepped"], case.n)
    for cls in ss.structural_classes(name, case.A):
        assert cov[cls] > 0, f"{name}: no env of class '{cls}'"
    refused = _reference(name).steps[0]
    untouched = refused["ostep"]["err"] != 0
    for key in ("pos", "alive", "arrived", "occupant", "gems", "beams", "avail"):  # (a refusal leaves the oracle's env as set_state left it)
        assert np.array_equal(refused["dump"][key][untouched], _reference(name).after_set_state["dump"][key][untouched]), key


@pytest.mark.parametrize("group", sorted(ss.GROUPS))
def test_coverage_of_every_lane_group(group):
    """Per lanes-per-environment class of step_kernel: between them the maps of the group show every class of step."""
    names = ss.GROUPS[group]
    total = {}
    for name in names:
        for k, v in _coverage(name).items():
            total[k] = total.get(k, 0) + v
    a_max = max(_reference(name).case.A for name in names)
    assert ss.group_size(a_max) == group
    missing = [cls for cls in ss.required_classes(a_max) if total.get(cls, 0) == 0]
    assert not missing, f"G = {group}: no env of {missing} on {names}"


def test_layouts_of_the_maps():
    """Between them the maps hold beams in registers with single layers, crossings up to four layers, more than 8 sources (the beams
    in the LDS record) and chained beam words; which of them can take the kernels with row heads is what the GPU suite lists."""
    from lle_amd import _capi
    from tests.test_gpu_step_states import HEAD_MAPS, PES_HEAD_MAPS

    maps = {name: _capi.Map(ss.text_of(name), row_align=128) for name in ss.MAP_NAMES}
    assert any(m.max_cell_layers == 1 and m.n_beam_words <= 8 for m in maps.values())
    assert maps["four_layers"].max_cell_layers == 4
    assert sum(m.n_sources > 8 for m in maps.values()) >= 3
    assert all(maps[name].n_beam_words > maps[name].n_sources for name in ss.CHAINED)
    assert {ss.group_size(m.n_agents) for m in maps.values()} == {1, 2, 4, 8, 16}
    for name, m in maps.items():
        assert ss.group_size(m.n_agents) == ss.GROUP_OF[name], name
    assert sorted(HEAD_MAPS) == sorted(name for name, m in maps.items() if m.n_beam_words <= 8 and m.row_head[1] != 0)
    assert sorted(PES_HEAD_MAPS) == sorted(name for name, m in maps.items() if m.n_sources and m.n_beam_words <= 8 and m.row_head_env_sources[1] != 0)
    assert maps["gems32"].n_gems == 32


def test_passes_on_the_planted_cascades():
    """move_agents passes, visible only on the host build (SimBatch.lane_passes on one-env batches), over the planted Q1 / cascade
    states: one, two and three passes occur with the shortcut; it is taken in some steps (the build without it runs one pass more:
    the no-op pass) and not in others (same count: the last pass ended the loop by itself)."""
    from lle_amd import _decode
    from tests import hostsim

    counts = {}
    for name in ss.MAP_NAMES:
        text = ss.text_of(name)
        for k, (pos, gems, alive, acts) in enumerate(ss.cascade_states(name)):
            got = []
            for engine in ("lanes", "lanes_no_shortcut"):
                sb = hostsim.SimBatch(text, 1)
                sb.set_engine(engine)
                sb.buf("req_pos")[0] = pos
                sb.buf("req_gems")[0] = _decode.pack_bits(gems)
                sb.buf("req_alive")[0] = _decode.pack_bits(alive)
                sb.set_state()
                assert int(sb.buf("err")[0]) == 0
                p0 = sb.lane_passes()
                sb.step(np.asarray(acts, np.uint8).reshape(1, -1))
                assert int(sb.buf("err")[0]) == 0
                got.append(sb.lane_passes() - p0)
            assert got[1] in (got[0], got[0] + 1), (name, k, got)
            counts[(name, k)] = tuple(got)
    with_shortcut = {c[0] for c in counts.values()}
    assert {1, 2, 3} <= with_shortcut, sorted(with_shortcut)
    assert any(c[1] == c[0] + 1 for c in counts.values()) and any(c[1] == c[0] and c[0] >= 1 for c in counts.values())
    assert counts[("q1", 0)] == (2, 3)  # the reference's Q1 script: tests/test_hostsim_lanes.py


def stale_reference(oracle_mod, n):
    """The oracle's side of the stale-availability scenario (tests/step_states.py STALE_MAP) for n identical envs: the refused request,
    then the step; asserts that the scenario is what it is meant to be."""
    ob = oracle_mod.OracleBatch(ss.STALE_MAP, n)
    pos, gems, alive = ss.STALE_REQUEST
    for e in range(n):
        with pytest.raises(oracle_mod.OracleError, match="InvalidWorldState"):
            ob.world(e).set_state(pos, gems, alive)
    d0 = ob.dump()
    assert d0["pos"][0].tolist() == [list(p) for p in pos] and d0["alive"][0].tolist() == [1, 1, 1, 0] and (d0["avail"][0, :3] == 31).all()
    ostep = ob.step(np.tile(np.array(ss.STALE_ACTIONS, np.uint8), (n, 1)))
    d1 = ob.dump()
    assert not ostep["err"].any() and np.array_equal(d1["pos"], d0["pos"]), "agents 0 and 1 share a target, agent 2 wants the cell agent 0 returns to"
    assert ob.world(0).panics()[0] == 0
    return ob, d0, ostep, d1


@pytest.mark.parametrize("engine", ENGINES)
def test_a_second_round_of_vertex_conflicts_through_stale_availability(oracle_mod, engine):
    """solve_vertex_conflicts (world.rs:365-378) repeats until no two agents share a target.  From a state the reference accepts one
    round always settles it (a cell an agent can be sent back to is occupied, so no move onto it is available); after a REFUSED set_state
    the lists are stale and a third agent may walk onto the cell the first one is sent back to."""
    from lle_amd import _decode
    from tests import hostsim

    n = 5
    ob, d0, ostep, d1 = stale_reference(oracle_mod, n)
    sb = hostsim.SimBatch(ss.STALE_MAP, n)
    sb.set_engine(engine)
    pos, gems, alive = ss.STALE_REQUEST
    sb.buf("req_pos")[:] = _decode.pack_positions(pos)
    sb.buf("req_gems")[:] = 0
    sb.buf("req_alive")[:] = _decode.pack_bits(alive)
    sb.set_state()
    assert (sb.buf("err") == 0x40).all()
    assert_state_equal(unpack_engine(_bufs(sb), *ob.dims), d0, f"{engine} after the refused set_state")
    sb.step(np.tile(np.array(ss.STALE_ACTIONS, np.uint8), (n, 1)))
    eng = unpack_engine(_bufs(sb), *ob.dims)
    assert_step_equal(eng, ostep, engine)
    assert_state_equal(eng, d1, engine)
