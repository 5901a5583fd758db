"""Plain-data worlds for oracle/observers.py, and the synthetic states of the observer tests (tests/test_gpu_observers_states.py).

oracle/observers.py restates python/lle/observations.py and env.py:146-163 over the ACCESSORS of a world: n_agents / height / width,
wall_pos / void_pos / exit_pos / gem_pos, sources(), lasers(), gems_collected(), positions(), get_state(), available_actions().
`StateWorld` answers those from plain data -- a render_ref.Scene (the static map), a render_ref.State (positions, gem bits, beam words,
colour per beam word), a 16-bit alive mask and a 5-bit availability mask per agent -- so that the oracle's builders run UNCHANGED on
states no world can be stepped into.  This is no second restatement of the observation rules; tests/test_observers_ref_cpu.py pins the
stand-in and the (word, bit) addressing of the beams against OracleWorld along rollouts.

THE STATE DOMAIN OF THE OBSERVERS.  The kernels of lle_amd/csrc/observers.hip do not bounds-check what they read from the state
buffers, so a state written into them must keep three limits (`assert_domain`, asserted before every write):
  * every position lies inside the grid (a position indexes the cell tables, the window sets and the non-empty bitmap);
  * no position is the cell of a laser source (the engine never puts an agent there; the source's -1 and the agent's 1 do not commute);
  * every colour is below n_agents, and ONE colour per source, replicated over all of its beam words (LLE_BUF_SRC_COLOUR holds a byte
    per word; a colour selects a layer: the reference raises IndexError on one without a layer, a kernel would write past the
    observer's block).
Everything else is free: any subset of gems, arbitrary beam words (not only prefixes), several agents on a cell, agents on walls,
voids and exits, dead agents anywhere, any availability bits.  No step may follow a write: the engine's invariants are not kept."""
import numpy as np

from oracle import observers as oo
from tests import render_ref

_capi = None


def _c():
    global _capi
    if _capi is None:
        from lle_amd import _capi as c
        _capi = c
    return _capi


class StateWorld:
    """The accessors oracle/observers.py uses, from plain data.
      scene  render_ref.Scene        state  render_ref.State (colours None: the map's)
      alive  bit a = agent a alive    avail  byte a: bit k = Action k available to agent a"""

    def __init__(self, scene, state, alive, avail):
        self.scene, self.state = scene, state
        self.n_agents, self.height, self.width = len(state.positions), scene.height, scene.width
        self.n_gems, self.n_sources = len(scene.gems), len(scene.sources)
        source_cells = [(s[0], s[1]) for s in scene.sources]
        walls = [tuple(c) for c in scene.walls]
        self.wall_pos = walls + [c for c in source_cells if c not in set(walls)]   # wall_pos holds the sources too (parser_v1.rs:22-25)
        self.void_pos = [tuple(c) for c in scene.voids]
        self.exit_pos = [tuple(c) for c in scene.exits]
        self.gem_pos = [tuple(c) for c in scene.gems]
        self._alive, self._avail = int(alive), [int(v) for v in avail]
        assert len(self._avail) == self.n_agents
        self._lasers = None

    def _colour(self, word, laser_id):
        return self.scene.sources[laser_id][3] if self.state.colours is None else int(self.state.colours[word])

    def sources(self):
        """[(i, j, direction, agent_id, enabled, length)]: each source with the colour of its FIRST word."""
        return [(i, j, d, self._colour(first, l), 1, 0) for l, (i, j, d, _c, first) in enumerate(self.scene.sources)]

    def lasers(self):
        """[(i, j, laser_id, agent_id, is_on, is_enabled)]: the two outer layers of every stack and no more (World.lasers(),
        world.rs:159-172); is_on = bit `bit` of beam word `word`, the colour that word's."""
        if self._lasers is None:
            out = []
            for (i, j), stack in sorted(self.scene.stacks.items()):
                for laser_id, _d, word, bit in stack[:2]:
                    on = (int(self.state.beam_words[word]) >> bit) & 1
                    out.append((i, j, laser_id, self._colour(word, laser_id), on, 1))
            self._lasers = out
        return self._lasers

    def gems_collected(self):
        return [bool((self.state.gem_bits >> g) & 1) for g in range(self.n_gems)]

    def positions(self):
        return [(int(p[0]), int(p[1])) for p in self.state.positions]

    def get_state(self):
        return self.positions(), self.gems_collected(), [bool((self._alive >> a) & 1) for a in range(self.n_agents)]

    def available_actions(self):
        return [[k for k in range(oo.N_ACTIONS) if (m >> k) & 1] for m in self._avail]


# ---------------------------------------------------------------------------------------------- the builders by (name, kind, param)
def kinds(partial_sizes=(3, 5, 7, 9, 11, 13, 15), views=True, states=True):
    c = _c()
    out = []
    if views:
        out += [("layered", c.LLE_OBS_LAYERED, 0), ("padded1", c.LLE_OBS_LAYERED_PADDED, 1), ("padded3", c.LLE_OBS_LAYERED_PADDED, 3),
                ("perspective", c.LLE_OBS_PERSPECTIVE, 0)]
    out += [(f"partial{k}", c.LLE_OBS_PARTIAL, k) for k in partial_sizes]
    if states:
        out += [("state", c.LLE_OBS_STATE, 0), ("normalized-state", c.LLE_OBS_NORMALIZED_STATE, 0)]
    return out


def observe(w, kind, param):
    """The oracle's tensor for one world, reduced to what the engine materialises (tests/observer_checks.oracle_observe), or None where
    the reference raises IndexError."""
    from tests.observer_checks import oracle_observe
    return oracle_observe(w, kind, param)


# ---------------------------------------------------------------------------------------------- the maps of the state tests
def state_maps():
    """name -> map text: every map of tests/test_gpu_observers_states.py (none is a workload size).  1 / 4 / 4 agents; two layers, three
    beams, aliasing colours; 3 and 5 agents (no power of two); 16 agents; 14 beam words; rows of several bitmap words and beams of several
    words; 32 x 32 with 8 agents; 3 x 255 and 255 x 3, the limits of the position packing and of the bitmap's margin."""
    from lle_amd import mapgen
    from oracle.levels import LEVELS
    from tests.parity_util import EXTRA_MAPS, LONG_MAPS
    from tests.test_gpu_render_states import MAP16, TALL, WIDE
    maps = {"level1": LEVELS[1], "level6": LEVELS[6]}
    maps.update({k: EXTRA_MAPS[k] for k in ("corridor", "nested", "four_layers", "three_beams", "colour_alias", "many_agents", "config5_32x32")})
    maps.update({k: LONG_MAPS[k] for k in ("long_three_words", "long_crossing")})
    maps.update(gen_3agents=mapgen.generate(9, 11, 3, 4, 3, n_voids=2, seed=31), gen_5agents=mapgen.generate(9, 11, 5, 5, 4, n_voids=2, seed=32),
                map16=MAP16, wide=WIDE, tall=TALL)
    return maps


# ---------------------------------------------------------------------------------------------- synthetic states
def source_words(m):
    """[(first word, one past the last word)] of every source of a Map."""
    first = m.source_first_words()
    return list(zip(first, first[1:] + [m.n_beam_words]))


def corner_plants(scene, n_agents, env0):
    """(env, agent, cell) entries for render_ref.random_states(planted=): an agent on each of the four corner cells that is no laser
    source -- corner q in env env0 + q, each with another agent index where the map has that many, agents 0 and A - 1 first -- and then
    all of them at once in env env0 + 4."""
    H, W = scene.height, scene.width
    corners = []
    for c in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]:
        if c not in corners and c not in {(s[0], s[1]) for s in scene.sources}:
            corners.append(c)
    order = []
    for a in [0, n_agents - 1] + list(range(1, n_agents - 1)):
        if a not in order:
            order.append(a)
    plants = [(env0 + q, order[q % len(order)], c) for q, c in enumerate(corners)]
    plants += [(env0 + 4, order[q], c) for q, c in enumerate(corners) if q < len(order)]
    return plants, corners


def observer_states(maps, n_envs, seed, planted=()):
    """render_ref.random_states of the maps (unchanged: same generator, same seed, same arrays) made fit for the observers: the colours are
    drawn again, one per SOURCE in [0, n_agents), replicated over the source's words; plus `alive` u16 [n] (env 0 of a block: everybody,
    env 1: nobody) and `avail` u8 [n, A] of five random bits (env 0: all five, env 1: none)."""
    scenes = [render_ref.Scene.of(m) for m in maps]
    A, Lw = maps[0].n_agents, maps[0].n_beam_words
    arrays = render_ref.random_states(scenes, n_envs, A, Lw, seed, planted)
    rng = np.random.default_rng([seed, 0x0B5])
    per = n_envs // len(maps)
    colours = np.zeros((n_envs, Lw), np.uint8)
    for k, m in enumerate(maps):
        for lo, hi in source_words(m):
            colours[k * per:(k + 1) * per, lo:hi] = rng.integers(0, A, (per, 1), dtype=np.uint8)
    alive = rng.integers(0, 1 << A, n_envs, dtype=np.uint32).astype(np.uint16)
    avail = rng.integers(0, 32, (n_envs, A), dtype=np.uint8)
    alive[0::per], avail[0::per] = (1 << A) - 1, 31
    alive[1::per], avail[1::per] = 0, 0
    arrays.update(colours=colours, alive=alive, avail=avail)
    return scenes, arrays


def assert_domain(maps, arrays):
    """The three limits of the module docstring, on the arrays that are about to be written."""
    pos, colours = arrays["pos"], arrays.get("colours")
    n, A = pos.shape[:2]
    per = n // len(maps)
    for k, m in enumerate(maps):
        block = pos[k * per:(k + 1) * per].reshape(-1, 2).astype(np.int64)
        assert (block[:, 0] < m.height).all() and (block[:, 1] < m.width).all(), "a position outside the grid"
        flat = set((block[:, 0] * 256 + block[:, 1]).tolist())
        for s in m.sources():
            assert int(s.i) * 256 + int(s.j) not in flat, "an agent on a laser source"
        if colours is not None and colours.size:
            c = colours[k * per:(k + 1) * per]
            assert int(c.max()) < A, "a colour without an agent"
            for lo, hi in source_words(m):
                assert (c[:, lo:hi] == c[:, lo:lo + 1]).all(), "the words of one source differ in colour"
    assert arrays["alive"].dtype == np.uint16 and int(arrays["avail"].max(initial=0)) < 32


def write_observer_states(bw, arrays, env_sources):
    """Write the arrays into the device buffers the observers read (render_ref.write_states, plus LLE_BUF_BITS -- the alive mask in the low
    16 bits, every other field zero -- and LLE_BUF_AVAIL).  env_sources: the batch keeps per-environment sources (one set_sources went
    before): the colours go into LLE_BUF_SRC_COLOUR; otherwise the map's colours hold and `colours` is not written."""
    import torch
    assert_domain(bw.maps, arrays if env_sources else {k: v for k, v in arrays.items() if k != "colours"})
    render_ref.write_states(bw, pos=arrays["pos"], gems=arrays["gems"], beams=arrays["beams"], colours=arrays["colours"] if env_sources else None)
    bw.bits.copy_(torch.from_numpy(arrays["alive"].astype(np.int64)).to(bw.device))
    bw.avail.copy_(torch.from_numpy(np.ascontiguousarray(arrays["avail"])).to(bw.device))
    torch.cuda.synchronize(bw.device)


def worlds_of(scenes, states, alive, avail):
    """One StateWorld per env; scenes: one per block of envs."""
    per = len(states) // len(scenes)
    return [StateWorld(scenes[e // per], states[e], int(alive[e]), avail[e]) for e in range(len(states))]


def worlds_of_arrays(scenes, arrays, env_sources):
    """The worlds the arrays describe, without a device (what write_observer_states + read_back give on one)."""
    n = len(arrays["pos"])
    states = [render_ref.State([(int(p[0]), int(p[1])) for p in arrays["pos"][e]], int(arrays["gems"][e]), list(arrays["beams"][e]),
                               list(arrays["colours"][e]) if env_sources else None) for e in range(n)]
    return worlds_of(scenes, states, arrays["alive"], arrays["avail"])


def read_back(bw, scenes, env_sources):
    """The StateWorld of every env of a batch, from its device buffers: render_ref.states_of plus `bits` and `avail`."""
    states = render_ref.states_of(bw, env_sources)
    alive = (bw.bits.cpu().numpy().astype(np.uint64) & np.uint64(0xFFFF)).astype(np.uint16)
    avail = bw.avail.cpu().numpy()
    return worlds_of(scenes, states, alive, avail)


def reference(worlds, kind, param):
    """The reference's tensor of every env stacked, [n, ...] (float32; the layered kinds hold -1 / 0 / 1), or None where it raises
    IndexError (then for every env or for none: the colours that decide it are the map's, or all below n_agents)."""
    rows = [observe(w, kind, param) for w in worlds]
    if any(r is None for r in rows):
        assert all(r is None for r in rows)
        return None
    return np.stack(rows)


def reference_avail(worlds, walkable):
    return np.stack([oo.available_actions(w, walkable) for w in worlds])


def first_difference(name, kind, got, want):
    """None, or the first difference as text: env, kind, observer, layer, cell, got, want.  The state kinds are compared bit for bit as
    uint32 (the reference rounds a float64 quotient to float32), the others as values."""
    c = _c()
    if kind in (c.LLE_OBS_STATE, c.LLE_OBS_NORMALIZED_STATE):
        assert got.dtype == np.float32 and want.dtype == np.float32
        g, w = got.view(np.uint32), want.view(np.uint32)
    else:
        g, w = got, want.astype(got.dtype)
        assert np.array_equal(w.astype(np.float32), want)
    assert g.shape == w.shape, f"{name}: shape {g.shape} != {w.shape}"
    if np.array_equal(g, w):
        return None
    idx = tuple(int(v) for v in np.argwhere(g != w)[0])
    where = {5: "env {} observer {} layer {} cell ({}, {})", 4: "env {} observer - layer {} cell ({}, {})", 3: "env {} agent {} action {}",
             2: "env {} element {}"}[g.ndim].format(*idx)
    return f"{name}: {int((g != w).sum())} values in {len(set(np.argwhere(g != w)[:, 0].tolist()))} envs differ; first {where}: got {got[idx]}, want {want[idx]}"
