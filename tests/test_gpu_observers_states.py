"""The observation builders of lle_amd/csrc/observers.hip over the parts of their domain that rollouts do not reach, against
oracle/observers.py run on plain-data worlds (tests/observers_ref.StateWorld), byte for byte, on EVERY environment of a batch.

What lle_batch_observe_as / lle_batch_available_actions give depends only on `pos`, `gems`, `beams`, `bits` (the alive mask), `avail`,
`src_colour` and the map tables, and BatchedWorld exposes those device buffers as torch views: the tests write SYNTHETIC states into
them (observers_ref.write_observer_states; no step follows, so the engine's invariants do not matter), read them back and compare.
The domain of such states -- positions inside the grid, none on a laser source, colours below n_agents -- is the module docstring of
tests/observers_ref.py; it is asserted before every write and no test leaves it.

Coverage is asserted on the arrays that are written (test_gpu_render_states.assert_coverage: the classes of cells that hold an agent,
every bit of every beam word on alone / on / off, every gem index both ways), and in addition an agent stands on every corner cell
that is no source -- another agent per corner, agents 0 and A - 1 among them -- and all agents stand on one cell in one env.  Batches
are ragged, 16 m + 5 environments: the last wavefront, the last batch of E rows and a batch with fewer rows than E are all there.

The partial k x k observation is compared under every launch variant (VARIANTS): the window-sets and the bitmap form of the lane
kernel with 1, 2 and 4 environments per batch, several batches per wavefront, plain stores, and the window and projection kernels.
A variant the launcher cannot honour for a map (an E above the largest its lanes can cover) falls back by the launcher's own rule; the
bytes must be the reference's all the same.  `-s` prints which window sizes obs_desc reports per map and which variants fall back."""
import numpy as np
import pytest
import torch

from lle_amd import _capi, mapgen
from lle_amd._capi import Map
from oracle.levels import LEVELS
from tests import observers_ref, render_ref
from tests.test_gpu_render_states import assert_coverage, make_batch

pytestmark = pytest.mark.gpu

MAPS = observers_ref.state_maps()
N = 133                      # 16 * 8 + 5
WINDOWS = (3, 5, 7, 9, 11, 13, 15)
VARIANTS = {
    "rule": {},
    "sets": {"LLE_PARTIAL_SETS": "1"},
    "sets-E1": {"LLE_PARTIAL_SETS": "1", "LLE_PARTIAL_E": "1"},
    "sets-E2": {"LLE_PARTIAL_SETS": "1", "LLE_PARTIAL_E": "2"},
    "sets-E4": {"LLE_PARTIAL_SETS": "1", "LLE_PARTIAL_E": "4"},
    "bitmap-E1": {"LLE_PARTIAL_NO_SETS": "1", "LLE_PARTIAL_E": "1"},
    "bitmap-E2": {"LLE_PARTIAL_NO_SETS": "1", "LLE_PARTIAL_E": "2"},
    "batches4": {"LLE_PARTIAL_BATCHES": "4"},
    "plain-stores": {"LLE_PARTIAL_WT": "0"},
    "window": {"LLE_PARTIAL_KERNEL": "window"},
    "project": {"LLE_PARTIAL_KERNEL": "project"},
}
PARTIAL_KERNELS = ("partial_lanes_kernel", "partial_observe_kernel", "partial_project_kernel")


class variant:
    """The LLE_PARTIAL_* overrides of one launch variant, set for a `with` block and taken back behind it (the library reads most of them
    once: _capi.refresh_tuning)."""

    def __init__(self, monkeypatch, name):
        self.mp, self.env = monkeypatch, VARIANTS[name]

    def __enter__(self):
        for k, v in self.env.items():
            self.mp.setenv(k, v)
        _capi.refresh_tuning()

    def __exit__(self, *exc):
        try:
            for k in self.env:
                self.mp.delenv(k)
        finally:
            _capi.refresh_tuning()


def e_max(n_agents, k):
    """The largest E the lane kernel's launcher takes for a window size (observers.hip launch_partial_observe): only to REPORT which variants fall back."""
    a_pad = 1 << max(0, (n_agents - 1).bit_length())
    s_min = 1 if k <= 8 else (k + 3) // 4
    e = 64 // a_pad
    while e > 1 and 64 // (e * a_pad) < s_min:
        e >>= 1
    return e


class Rig:
    """A BatchedWorld of `texts` (map m owns block m) holding seeded synthetic states, and the reference of every env.
    env_sources: one set_sources of the maps' own colours goes first, so that the batch keeps per-environment sources; the states then carry
    a colour per source and env.  The states are written once and never changed; the references are computed once per observation."""

    def __init__(self, texts, n, seed, env_sources, plant=True, cover=True):
        self.maps = [Map(t) for t in texts]
        self.n, self.env_sources = n, env_sources
        scene0 = render_ref.Scene.of(self.maps[0])
        plants, self.corners = observers_ref.corner_plants(scene0, self.maps[0].n_agents, 40) if plant else ([], [])
        self.scenes, self.arrays = observers_ref.observer_states(self.maps, n, seed, plants)
        A = self.maps[0].n_agents
        if cover:
            assert_coverage(self.maps, self.arrays)
        if plant:
            pos = self.arrays["pos"]
            assert all(tuple(pos[e, a]) == c for e, a, c in plants) and {c for _e, _a, c in plants} == set(self.corners) and self.corners
            firsts = [a for _e, a, _c in plants[:len(self.corners)]]
            assert len(set(firsts)) == min(A, len(self.corners)) and (A == 1 or len(self.corners) < 2 or {0, A - 1} <= set(firsts))
            assert len({tuple(p) for p in pos[3]}) == 1, "all agents on one cell"
        self.bw = make_batch(self.maps if len(self.maps) > 1 else self.maps[0], n, env_sources)
        observers_ref.write_observer_states(self.bw, self.arrays, env_sources)
        # what the device holds is what was drawn: the references are those of the worlds read back
        self.worlds = observers_ref.read_back(self.bw, self.scenes, env_sources)
        for w, v in zip(self.worlds, observers_ref.worlds_of_arrays(self.scenes, self.arrays, env_sources)):
            assert (w.positions(), w.state.gem_bits, [int(b) for b in w.state.beam_words], w._alive, w._avail) == \
                   (v.positions(), v.state.gem_bits, [int(b) for b in v.state.beam_words], v._alive, v._avail)
            assert (w.state.colours is None) == (not env_sources) and (not env_sources or [int(c) for c in w.state.colours] == [int(c) for c in v.state.colours])
        assert int(self.bw.bits.max()) < 1 << 16
        self._refs = {}

    def want(self, kind, param):
        if (kind, param) not in self._refs:
            self._refs[kind, param] = observers_ref.reference(self.worlds, kind, param)
        return self._refs[kind, param]

    def check(self, kinds, where):
        """Every env of every kind; where the reference raises IndexError the engine must refuse (and the other way round)."""
        served = []
        for name, kind, param in kinds:
            want = self.want(kind, param)
            supported = bool(self.bw.obs_desc(kind, param).supported)
            assert supported == (want is not None), f"{where} {name}: obs_desc says supported = {supported}, the reference {'raises IndexError' if want is None else 'serves it'}"
            if want is None:
                with pytest.raises(IndexError):
                    self.bw.observe_as(kind, param)
                continue
            got = self.bw.observe_as(kind, param)
            torch.cuda.synchronize(self.bw.device)
            diff = observers_ref.first_difference(name, kind, got.cpu().numpy(), want)
            assert diff is None, f"{where} (env_sources={self.env_sources}) {diff}"
            served.append(name)
        return served

    def check_avail(self, where):
        for walkable in (True, False):
            key = ("avail", walkable)
            if key not in self._refs:
                self._refs[key] = observers_ref.reference_avail(self.worlds, walkable)
            got = self.bw.available_actions(walkable)
            torch.cuda.synchronize(self.bw.device)
            diff = observers_ref.first_difference(f"available_actions({walkable})", -1, got.cpu().numpy(), self._refs[key])
            assert diff is None, f"{where} (env_sources={self.env_sources}) {diff}"


_RIGS = {}


def rig_of(name, env_sources):
    """The rig of a map of MAPS, shared by the tests and variants that read it (nothing ever changes its states)."""
    key = (name, env_sources)
    if key not in _RIGS:
        _RIGS[key] = Rig([MAPS[name]], N, 2000 + len(name), env_sources)
    return _RIGS[key]


def source_modes(name):
    """(False, True): the map's sources, then per-environment colours -- where the map has sources and lle_batch_set_sources takes its own
    colours (colour_alias: they lie above n_agents, outside the domain of per-environment colours; level1 and corridor have no source)."""
    m = Map(MAPS[name])
    return (False, True) if m.n_sources and all(int(s.agent_id) < m.n_agents for s in m.sources()) else (False,)


# ---------------------------------------------------------------------------------------------- views, state, availability
@pytest.mark.parametrize("name", sorted(MAPS))
def test_views_on_synthetic_states(name):
    """Layered, layered-padded (p = 1 and 3), perspective, state and normalized-state (bit for bit as uint32) and both availability modes
    (from the written `avail` bytes), with the map's sources and with per-environment colours."""
    for env_sources in source_modes(name):
        rig = rig_of(name, env_sources)
        served = rig.check(observers_ref.kinds(partial_sizes=()), name)
        assert {"state", "normalized-state"} <= set(served) and (len(source_modes(name)) == 1 or len(served) == 6), served   # (colours below n_agents: all six)
        rig.check_avail(name)


# ---------------------------------------------------------------------------------------------- partial k x k
@pytest.mark.parametrize("var", list(VARIANTS))
@pytest.mark.parametrize("name", sorted(MAPS))
def test_partial_on_synthetic_states(name, var, monkeypatch):
    """Every odd window from 3 to 15 that obs_desc reports supported, under one launch variant, with the map's sources and with
    per-environment colours.  (colour_alias: its colours have no layer in this observation -- IndexError, like the reference.)"""
    rigs = [rig_of(name, env_sources) for env_sources in source_modes(name)]
    A = rigs[0].maps[0].n_agents
    with variant(monkeypatch, var):
        served = [rig.check(observers_ref.kinds(WINDOWS, views=False, states=False), f"{name} [{var}]") for rig in rigs]
    assert all(s == served[0] for s in served) and (len(rigs) == 1 or len(served[0]) == len(WINDOWS)), served   # (colours below n_agents: every window)
    forced = int(VARIANTS[var].get("LLE_PARTIAL_E", 0))
    back = [k for k in WINDOWS if forced > e_max(A, k)]
    print(f"\npartial {name} [{var}]: supported {served[0]}" + (f"; E={forced} falls back to the rule for k in {back}" if back else ""))


def test_zz_all_three_partial_kernels_ran():
    """Behind the sweep (this file's tests run in order): the lane, window and projection kernels were all launched by this process."""
    launched = set(_capi.launched_kernels())
    assert all(k in launched for k in PARTIAL_KERNELS), sorted(launched)


def test_partial_trial_picks_identical_bytes(monkeypatch):
    """4 096 + 37 environments of level 6: from 4 096 on, the first lle_batch_observe_as(LLE_OBS_PARTIAL, 3 | 5 | 7) of a batch times
    window sets against the bitmap and E against E / 2 (capi.cpp PartialChoice) and later calls launch the winner -- which code a user
    gets depends on timing.  The first call (trial and final launch) and the second (the winner) both equal the reference on EVERY
    env; a fresh batch with the same states under LLE_PARTIAL_NO_TRIAL=1 gives the same bytes."""
    n = 4096 + 37
    rig = Rig([LEVELS[6]], n, 77, False)
    kinds = observers_ref.kinds((3, 5, 7), views=False, states=False)
    first = {}
    for _name, kind, k in kinds:
        first[k] = rig.bw.observe_as(kind, k).clone()
    assert rig.check(kinds, "the trial's call") == ["partial3", "partial5", "partial7"]   # (each size's SECOND call: the winner)
    for name, kind, k in kinds:
        diff = observers_ref.first_difference(name, kind, first[k].cpu().numpy(), rig.want(kind, k))
        assert diff is None, f"first call: {diff}"
    monkeypatch.setenv("LLE_PARTIAL_NO_TRIAL", "1")
    try:
        fresh = make_batch(rig.maps[0], n, False)
        observers_ref.write_observer_states(fresh, rig.arrays, False)
        for _name, kind, k in kinds:
            assert torch.equal(fresh.observe_as(kind, k), first[k]), k
    finally:
        monkeypatch.delenv("LLE_PARTIAL_NO_TRIAL")


# ---------------------------------------------------------------------------------------------- blocks of maps
@pytest.mark.parametrize("per", [8, 24, 64])
def test_blocks_of_maps_on_synthetic_states(per, monkeypatch):
    """Four generated 9 x 11 maps of 3 agents, `per` environments each: envs_per_map is no multiple of 16 (8, 24) or is one (64), which
    shrinks the environments per wavefront, E, the wavefronts per workgroup and the batches.  Every env against the reference built from
    ITS map's scene: layered, perspective, partial 3 / 7 / 9 under the rule and with the window sets forced; availability too."""
    texts = [mapgen.generate(height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2, seed=300 + s) for s in range(4)]
    assert len(set(texts)) == 4
    kinds = [k for k in observers_ref.kinds((3, 7, 9), states=False) if not k[0].startswith("padded")]
    for env_sources in (False, True):
        rig = Rig(texts, 4 * per, 50 + per, env_sources, plant=False, cover=False)
        assert rig.bw.envs_per_map == per and len({id(w.scene) for w in rig.worlds}) == 4
        for var in ("rule", "sets"):
            with variant(monkeypatch, var):
                assert len(rig.check(kinds, f"per={per} [{var}]")) == 5
        rig.check_avail(f"per={per}")


# ---------------------------------------------------------------------------------------------- stray writes
@pytest.mark.parametrize("what", ["padded3", "perspective", "partial3", "partial15", "state", "avail"])
def test_observers_write_only_their_output(what, monkeypatch):
    """`out=` is a slice of exactly the announced size inside an allocation filled with 0x5A, 4 KiB on each side (the slice keeps the 16-byte
    alignment obs_desc asks for); n is ragged, so the last wavefront and the last block of E rows end inside the slice.  Not a guard byte
    changes, and the slice holds the reference.  The partial sizes under the lane kernel's two forms and the two older kernels."""
    guard = 4096
    for name in ("level6", "gen_5agents"):
        rig = rig_of(name, False)
        bw, A = rig.bw, rig.maps[0].n_agents
        if what == "avail":
            need = N * A * 5
        else:
            (kname, kind, param), = [k for k in observers_ref.kinds() if k[0] == what]
            need = int(bw.obs_desc(kind, param).bytes)
        for var in (("rule", "sets", "bitmap-E2", "window", "project") if what.startswith("partial") else ("rule",)):
            big = torch.full((need + 2 * guard,), 0x5A, dtype=torch.uint8, device=bw.device)
            out = big[guard:guard + need]
            assert out.data_ptr() % 16 == 0
            with variant(monkeypatch, var):
                if what == "avail":
                    got = bw.available_actions(False, out=out.view(N, A, 5))
                    want, kind = rig._refs.get(("avail", False)), -1
                    want = observers_ref.reference_avail(rig.worlds, False) if want is None else want
                else:
                    got, want = bw.observe_as(kind, param, out=out), rig.want(kind, param)
            torch.cuda.synchronize(bw.device)
            assert got.data_ptr() == big.data_ptr() + guard
            assert bool((big[:guard] == 0x5A).all()) and bool((big[guard + need:] == 0x5A).all()), f"{name} {what} [{var}]: a guard byte was written"
            diff = observers_ref.first_difference(what, kind, got.cpu().numpy(), want)
            assert diff is None, f"{name} [{var}] {diff}"


# ---------------------------------------------------------------------------------------------- one case by hand
# level 6 with ONE cell changed: a gem at (4, 1), the first tile of source 0's beam (level 6 itself has no gem under a beam)
HAND_MAP = LEVELS[6].replace("L0E . . . . . . @", "L0E G . . . . . @")


def test_dead_and_stacked_agents_by_hand(monkeypatch):
    """Agents 1 (alive) and 2 (DEAD) both on the gem cell (4, 1) under the lit first tile of source 0's beam; agent 0 in the corner
    (11, 0); agent 3 in the corner (11, 12) on a collected gem next to two exits; every other beam bit off.  The expected bytes are written
    out here -- layers: agents 0-3, WALL 4, lasers 5-8, GEM 9, EXIT 10 (observations.py:318-323) -- so this case does not depend on the
    stand-in: 3 x 3 for every observer, 15 x 15 for the observer in the corner (window cell (wi, wj) = map cell (4 + wi, wj - 7))."""
    m = Map(HAND_MAP)
    scene = render_ref.Scene.of(m)
    assert (m.n_agents, m.height, m.width) == (4, 12, 13) and (4, 1) in scene.gems and (11, 12) in scene.gems
    (lid, _d, word, bit), = scene.stacks[(4, 1)]
    src, = [l for l, s in enumerate(scene.sources) if s[:2] == (4, 0)]   # (laser ids follow the map text: L2S in row 0 comes first)
    assert lid == src and scene.sources[src][3] == 0
    n = 21
    pos = np.tile(np.array([[11, 0], [4, 1], [4, 1], [11, 12]], np.uint8), (n, 1, 1))
    beams = np.zeros((n, m.n_beam_words), np.uint32)
    beams[:, word] = 1 << bit
    arrays = dict(pos=pos, gems=np.full(n, 1 << scene.gems.index((11, 12)), np.uint32), beams=beams, colours=np.zeros((n, m.n_beam_words), np.uint8),
                  alive=np.full(n, 0b1011, np.uint16), avail=np.full((n, 4), 31, np.uint8))
    bw = make_batch(m, n, False)
    observers_ref.write_observer_states(bw, arrays, False)
    WALL, L0, GEM, EXIT = 4, 5, 9, 10
    want3 = np.zeros((4, 11, 3, 3), np.int8)
    want3[0, 0, 1, 1] = 1                                            # the corner (11, 0): itself and bare floor
    for a in (1, 2):                                                  # the window of (4, 1): rows 3-5, columns 0-2
        want3[a, 1, 1, 1] = want3[a, 2, 1, 1] = 1                      # both agents, the dead one too
        want3[a, WALL, 0, 0] = want3[a, WALL, 0, 1] = 1                # walls (3, 0), (3, 1)
        want3[a, WALL, 1, 0], want3[a, L0, 1, 0] = 1, -1               # the source (4, 0): a wall, and -1 in its colour's layer
        want3[a, L0, 1, 1] = want3[a, GEM, 1, 1] = 1                   # the lit tile over the gem that is still there
    want3[3, 3, 1, 1] = 1                                            # the corner (11, 12): the gem under it is collected
    want3[3, EXIT, 0, 0] = want3[3, EXIT, 1, 0] = 1                    # exits (10, 11), (11, 11)
    want15 = np.zeros((11, 15, 15), np.int8)
    want15[0, 7, 7] = want15[1, 0, 8] = want15[2, 0, 8] = 1           # agent 3 lies outside (column 12 -> wj 19)
    for wi, wj in ((0, 7), (0, 14), (3, 14), (4, 14)):                # source (4, 0), walls (4, 7), (7, 7), (8, 7)
        want15[WALL, wi, wj] = 1
    want15[L0, 0, 7], want15[L0, 0, 8] = -1, 1
    want15[GEM, 0, 8] = want15[GEM, 6, 11] = 1                        # gems (4, 1) and (10, 4); (7, 9) lies outside (wj 16)
    for var in ("rule", "sets", "bitmap-E1", "window", "project"):
        with variant(monkeypatch, var):
            got3 = bw.observe_as(_capi.LLE_OBS_PARTIAL, 3).cpu().numpy()
            got15 = bw.observe_as(_capi.LLE_OBS_PARTIAL, 15).cpu().numpy()
        for e in range(n):
            assert np.array_equal(got3[e], want3), (var, e, np.argwhere(got3[e] != want3)[:4].tolist())
            assert np.array_equal(got15[e, 0], want15), (var, e, np.argwhere(got15[e, 0] != want15)[:4].tolist())
    state = bw.observe_as(_capi.LLE_OBS_STATE).cpu().numpy()
    G = m.n_gems
    assert state.shape == (n, 12 + G) and (state[:, :8] == [11, 0, 4, 1, 4, 1, 11, 12]).all() and (state[:, 8 + G:] == [1, 1, 0, 1]).all()
    assert state[:, 8:8 + G].sum() == n and (state[:, 8 + scene.gems.index((11, 12))] == 1).all()
