"""tests/observers_ref.StateWorld, the plain-data stand-in that lets oracle/observers.py run on synthetic states, pinned WITHOUT a GPU
(Map is a host object): the static parts of render_ref.Scene.of(Map(text)) against the OracleWorld of the same text, and along a seeded
oracle rollout every builder on the stand-in -- built from the oracle's own positions / gems / alive flags and the on-flags of
lasers(), mapped to beam words through Scene.stacks -- against the builder on the oracle world itself.  Independent of the kernels."""
import random

import numpy as np
import pytest

from lle_amd._capi import Map
from oracle import observers as oo
from tests import observers_ref, render_ref

MAPS = observers_ref.state_maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_scene_is_the_oracles_static_world(oracle_mod, name):
    m = Map(MAPS[name])
    scene = render_ref.Scene.of(m)
    ow = oracle_mod.OracleWorld(MAPS[name])
    sw = observers_ref.StateWorld(scene, render_ref.State(ow.start_pos, 0, [0] * m.n_beam_words, None), 0xFFFF, [31] * ow.n_agents)
    assert (sw.n_agents, sw.height, sw.width, sw.n_gems, sw.n_sources) == (ow.n_agents, ow.height, ow.width, ow.n_gems, ow.n_sources)
    assert len(sw.wall_pos) == len(set(sw.wall_pos)) and set(sw.wall_pos) == set(ow.wall_pos)   # (sources included)
    assert {(s[0], s[1]) for s in ow.sources()} <= set(sw.wall_pos)
    assert sorted(sw.exit_pos) == sorted(ow.exit_pos) and sorted(sw.void_pos) == sorted(ow.void_pos)
    assert sw.gem_pos == ow.gem_pos                                                              # (in index order)
    assert [s[:4] for s in sw.sources()] == [s[:4] for s in ow.sources()]
    assert len(sw.lasers()) == len(ow.lasers()) and {l[:4] for l in sw.lasers()} == {l[:4] for l in ow.lasers()}
    words = observers_ref.source_words(m)
    assert len(words) == ow.n_sources and all(lo < hi for lo, hi in words) and (not words or words[-1][1] == m.n_beam_words)
    for stack in scene.stacks.values():   # a layer's word is one of its source's
        assert all(words[l][0] <= word < words[l][1] and 0 <= bit < 32 for l, _d, word, bit in stack)


def _stand_in(scene, m, ow, explicit_colours):
    """The StateWorld of an oracle world's current state."""
    pos, gems, alive = ow.get_state()
    beams = [0] * m.n_beam_words
    for i, j, laser_id, _colour, is_on, _en in ow.lasers():
        entry = [e for e in scene.stacks[(i, j)][:2] if e[0] == laser_id]
        assert len(entry) == 1, "World.lasers() lists a layer that is none of the two outer ones of the stack"
        if is_on:
            beams[entry[0][2]] |= 1 << entry[0][3]
    colours = None
    if explicit_colours:
        colours = [0] * m.n_beam_words
        for (lo, hi), src in zip(observers_ref.source_words(m), ow.sources()):
            colours[lo:hi] = [src[3]] * (hi - lo)
    state = render_ref.State(pos, sum(1 << g for g, c in enumerate(gems) if c), beams, colours)
    avail = [sum(1 << k for k in acts) for acts in ow.available_actions()]
    return observers_ref.StateWorld(scene, state, sum(1 << a for a, v in enumerate(alive) if v), avail)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_builders_on_the_stand_in_equal_those_on_the_oracle_world(oracle_mod, name):
    """30 seeded steps (a reset after a death or when everybody has arrived): all of observer_checks.KINDS, windows 9 to 15 added, both
    availability modes; the colours from the map in even steps, spelled out per beam word in odd ones."""
    m = Map(MAPS[name])
    scene = render_ref.Scene.of(m)
    ow = oracle_mod.OracleWorld(MAPS[name])
    ow.reset()
    rng = random.Random(len(name))
    for t in range(31):
        sw = _stand_in(scene, m, ow, explicit_colours=t % 2 == 1)
        for kname, kind, param in observers_ref.kinds():
            want, got = observers_ref.observe(ow, kind, param), observers_ref.observe(sw, kind, param)
            assert (want is None) == (got is None), (name, t, kname)
            if want is not None:
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, t, kname)
        for walkable in (True, False):
            assert np.array_equal(oo.available_actions(sw, walkable), oo.available_actions(ow, walkable)), (name, t, walkable)
        if not all(ow.alive()) or all(ow.arrived()):
            ow.reset()
        else:
            ow.step([rng.choice(acts) for acts in ow.available_actions()])


def test_observer_states_keep_the_render_generator_and_the_domain():
    """observer_states: pos / gems / beams are render_ref.random_states' own arrays for the same seed; the colours are one per source,
    below n_agents; the planted corners and the all-on-one-cell env are there; assert_domain refuses what the kernels cannot take."""
    m = Map(MAPS["long_crossing"])
    scene = render_ref.Scene.of(m)
    plants, corners = observers_ref.corner_plants(scene, m.n_agents, 40)
    scenes, arrays = observers_ref.observer_states([m], 133, 5, plants)
    plain = render_ref.random_states([scene], 133, m.n_agents, m.n_beam_words, 5, plants)
    assert all(np.array_equal(arrays[k], plain[k]) for k in ("pos", "gems", "beams"))
    observers_ref.assert_domain([m], arrays)
    assert len(corners) == 4 and {a for _e, a, _c in plants[:4]} >= {0, m.n_agents - 1}
    for e, a, c in plants:
        assert tuple(arrays["pos"][e, a]) == c
    assert len({tuple(p) for p in arrays["pos"][3]}) == 1
    assert len(set(arrays["colours"].reshape(-1).tolist())) == m.n_agents and len(set(arrays["alive"].tolist())) > 4
    for key, e, value in (("pos", (7, 0), (m.height, 0)), ("pos", (7, 1), (0, m.width)), ("pos", (9, 2), (int(m.sources()[0].i), int(m.sources()[0].j))),
                          ("colours", (11, 0), m.n_agents)):
        bad = {k: v.copy() for k, v in arrays.items()}
        bad[key][e] = value
        with pytest.raises(AssertionError):
            observers_ref.assert_domain([m], bad)
    words = observers_ref.source_words(m)
    long = [w for w in words if w[1] - w[0] > 1]
    assert long, "long_crossing has beams of several words"
    bad = {k: v.copy() for k, v in arrays.items()}
    bad["colours"][:, long[0][0]] = (bad["colours"][:, long[0][0]] + 1) % m.n_agents
    with pytest.raises(AssertionError):
        observers_ref.assert_domain([m], bad)
