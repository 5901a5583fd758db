"""The coop kernel (liblle_coop.so, lle_amd/coop/coop.hip) over the parts of its domain that BatchedLLE rollouts do not reach, against
the plain-data restatement of the rule (tests/coop_ref.detect_state) and of the operations (tests/coop_ref.EnvRef), exactly.

lle_coop_update depends only on LLE_BUF_POS, LLE_BUF_BITS, LLE_BUF_EVCOUNT, LLE_BUF_SRC_COLOUR / _ENABLED, the handle's five arrays and
the map tables.  The tests write SYNTHETIC states into those buffers (no step follows, so the engine's invariants do not matter),
call the C ABI once and compare everything the call may write.  The handle's arrays lie between runs of guard bytes that no call
may touch; the guards and the rows of the environments that env_mask leaves out are checked after every call (`Rig.call`)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import coop_ref
from tests.coop_ref import CLEAR, FINISH, MARK_POS, MARK_STARTS
from tests.test_gpu_coop import line_map

pytestmark = pytest.mark.gpu

LLE_ERR_NULL, LLE_ERR_ARG = -1, -2
GUARD = 256  # LLE_COOP_GUARD_BYTES

TWO_SOURCES_ONE_COLOUR = "L0E . . . @\nS0 S1 S2 . .\nL0E . . . @\nX X X . ."
CROSSING = ". . L1S . .\nL0E . . . @\n. . . . .\nS0 S1 . S2 .\nX X . X ."
THREE_BEAMS = ". . L2S . .\n. . . S2 .\nL0E S0 . S1 @\n. . . . .\nX X L0N X ."
START_ON_BEAM = "L0E S0 S1 . X\n. . . . X"


def many_sources_map():
    """32 sources (LLE_MAX_SOURCES), colours cycling over 4 agents, every beam 6 cells."""
    rows = [f"L{k % 4}E . . . . . . @" for k in range(32)]
    return "\n".join(rows + ["S0 S1 S2 S3 X X X X"])


def _raw(ptr, nbytes, device):
    class _Bytes:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(_Bytes(), device=device)


class Rig:
    """A BatchedWorld of `texts` (map m owns block m), a CooperationTracker on it and one coop_ref.EnvRef per environment."""

    def __init__(self, oracle_mod, texts, n):
        from lle_amd import BatchedWorld
        from lle_amd.cooperation import CooperationTracker, lib
        self.texts = list(texts)
        self.bw = BatchedWorld(self.texts if len(self.texts) > 1 else self.texts[0], n)
        self.tr = CooperationTracker(self.bw)
        self.lib = lib()
        self.worlds = [oracle_mod.OracleWorld(t) for t in self.texts]
        w = self.worlds[0]
        self.n, self.per = int(n), int(n) // len(self.texts)
        self.A, self.L, self.H, self.W = w.n_agents, w.n_sources, w.height, w.width
        self.lasers = [[(i, j, l) for i, j, l, _c, _on, _en in w.lasers()] for w in self.worlds]
        self.colours = [[s[3] for s in w.sources()] for w in self.worlds]
        self.enabled = [[bool(s[4]) for s in w.sources()] for w in self.worlds]
        self.starts = []
        for m, w in enumerate(self.worlds):
            w.reset()
            self.starts.append(coop_ref.detect(w))
            assert set(self.tr.start_edges(m)) == self.starts[m], "the start edges of the handle are those of the freshly reset oracle world"
        self.views = [self.tr.step_edges, self.tr.episode_edges, self.tr.last_edges, self.tr.episode_profile, self.tr.last_profile]
        self.first_words = self.bw.map.source_first_words()
        self.env_colours = self.env_enabled = None
        self.pos = self.bw.pos.cpu().numpy().copy()
        self.occupant = np.ones((self.n, self.A), bool)
        self.ev = np.zeros(self.n, np.uint8)
        # every array between two runs of guard bytes (include/lle_coop.h)
        self.guards = []
        for which, v in enumerate(self.views):
            assert v.data_ptr() == self.lib.lle_coop_buffer(self.tr.h, which) and v.is_contiguous()
            nbytes = v.numel() * v.element_size()
            self.guards.append((_raw(v.data_ptr() - GUARD, GUARD, self.bw.device), _raw(v.data_ptr() + nbytes, GUARD - nbytes % GUARD if nbytes % GUARD else GUARD, self.bw.device)))

    # ---- synthetic state
    def write(self, pos=None, occupant=None, evcount=None, colours=None, enabled=None):
        dev = self.bw.device
        if pos is not None:
            self.pos = np.ascontiguousarray(pos, np.uint8).reshape(self.n, self.A, 2)
            self.bw.pos.copy_(torch.from_numpy(self.pos).to(dev))
        if occupant is not None:
            self.occupant = np.asarray(occupant, bool).reshape(self.n, self.A)
            bits = np.full(self.n, (1 << self.A) - 1, np.int64)  # everybody alive; the kernel must read the occupant bits only
            for a in range(self.A):
                bits |= self.occupant[:, a].astype(np.int64) << (32 + a)
            self.bw.bits.copy_(torch.from_numpy(bits).to(dev))
        if evcount is not None:
            self.ev = np.ascontiguousarray(evcount, np.uint8).reshape(self.n)
            self.bw.evcount.copy_(torch.from_numpy(self.ev).to(dev))
        if colours is not None:  # per-environment sources, written straight into LLE_BUF_SRC_COLOUR / LLE_BUF_SRC_ENABLED
            self.env_colours = np.ascontiguousarray(colours, np.uint8).reshape(self.n, self.L)
            self.env_enabled = np.ascontiguousarray(enabled, np.int64).reshape(self.n)
            rec = torch.zeros_like(self.bw.src_colour)
            rec[:, self.first_words] = torch.from_numpy(self.env_colours).to(dev)
            self.bw.src_colour.copy_(rec)
            self.bw.src_enabled.copy_(torch.from_numpy(self.env_enabled.astype(np.uint32).view(np.int32)).to(dev))
        torch.cuda.synchronize(dev)

    def preset(self, rng):
        """Random valid contents for the five arrays (rows without self-loops, bits below A); returns the EnvRefs that stand for them."""
        refs = []
        host = [np.zeros((self.n, self.A), np.int32) for _ in range(3)] + [np.zeros((self.n, 8), np.uint8) for _ in range(2)]
        for e in range(self.n):
            r = coop_ref.EnvRef(self.A)
            sets = []
            for _ in range(3):
                density = rng.choice([0.0, 0.15, 0.6])
                sets.append({(h, b) for h in range(self.A) for b in range(self.A) if h != b and rng.random() < density})
            r.step, r.episode, r.last = sets
            r.n_states, r.last_states = int(rng.choice([0, 1, 7, 254, 255])), int(rng.integers(0, 256))
            r.episode_valid, r.last_valid = bool(rng.integers(2)), bool(rng.integers(2))
            for k, arr in enumerate(r.arrays()[:3]):
                host[k][e] = arr
            # (the counter and the degree bytes are there whatever the valid byte says: an update reads the counter)
            host[3][e] = coop_ref.profile(r.episode, r.n_states, r.episode_valid)
            host[4][e] = coop_ref.profile(r.last, r.last_states, r.last_valid)
            refs.append(r)
        for v, h in zip(self.views, host):
            v.copy_(torch.from_numpy(h).to(v.device))
        torch.cuda.synchronize(self.bw.device)
        return refs, host

    def state_edges(self, e, env_sources):
        m = e // self.per
        colours = self.env_colours[e] if env_sources else self.colours[m]
        enabled = [(int(self.env_enabled[e]) >> l) & 1 for l in range(self.L)] if env_sources else self.enabled[m]
        return coop_ref.detect_state(self.lasers[m], self.pos[e], self.occupant[e], [int(c) for c in colours], enabled)

    def call(self, where, ops, honour=False, mask=None, env_sources=False, rng=None):
        """One lle_coop_update over random presets; every array compared, the unselected rows and the guards untouched."""
        rng = rng or np.random.default_rng(0)
        refs, before = self.preset(rng)
        self.tr.update(ops, honour_auto_reset=honour, env_mask=None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)), env_sources=env_sources)
        torch.cuda.synchronize(self.bw.device)
        got = [v.cpu().numpy() for v in self.views]
        want = [b.copy() for b in before]
        n_edges = 0
        for e, r in enumerate(refs):
            if mask is not None and not mask[e]:
                continue
            edges = self.state_edges(e, env_sources) if ops & MARK_POS else set()
            n_edges += len(edges)
            r.update(ops, edges, self.starts[e // self.per], was_reset=honour and bool(self.ev[e] & 0x80))
            if not r.touched:
                continue
            new = r.arrays()
            if ops & MARK_POS:
                want[0][e] = new[0]
            want[1][e], want[3][e] = new[1], new[3]
            if r.finished:
                want[2][e], want[4][e] = new[2], new[4]
        names = ("step_edges", "episode_edges", "last_edges", "episode_profile", "last_profile")
        for name, g, w in zip(names, got, want):
            if not np.array_equal(g, w):
                bad = int(np.nonzero((g != w).reshape(self.n, -1).any(axis=1))[0][0])
                raise AssertionError(f"{where}: {name} differs in env {bad}: {g[bad].tolist()} != {w[bad].tolist()} (before {before[names.index(name)][bad].tolist()})")
        for lo, hi in self.guards:
            assert int(lo.max()) == 0 and int(hi.max()) == 0, f"{where}: a guard byte was written"
        return n_edges


def beam_cells(rig, m=0):
    return sorted({(i, j) for i, j, _l in rig.lasers[m]})


# ---------------------------------------------------------------------------------------------- one beam
def test_one_blocker_with_1_to_15_beneficiaries(oracle_mod):
    """line_map(16): the beam covers (0, 1) .. (0, 16).  Environment e puts k = e % 15 + 1 other agents on it, the rest on the row
    below; in the second half of the batch the blocker stands at the FAR end, every beneficiary upstream of it: the beam's on / off
    bits play no part, only who occupies a tile."""
    n = 128
    rig = Rig(oracle_mod, [line_map(16)], n)
    pos = np.zeros((n, 16, 2), np.uint8)
    want = []
    for e in range(n):
        k = e % 15 + 1
        upstream = e >= n // 2
        for a in range(16):
            on = a <= k
            col = (16 - a) if upstream else (1 + a)
            pos[e, a] = (0, col) if on else (1, a)
        want.append({(0, b) for b in range(1, k + 1)})
    rig.write(pos=pos, occupant=np.ones((n, 16), bool))
    assert [rig.state_edges(e, False) for e in range(n)] == want
    rig.call("1-15 beneficiaries", CLEAR | MARK_POS)
    assert rig.tr.step_edges.cpu()[:, 0].tolist() == [(1 << (e % 15 + 2)) - 2 for e in range(n)]
    assert rig.tr.episode_profile.cpu()[14].tolist() == [15, 16, 1, 15, 15, 1, 0, 1]
    assert bool(rig.tr.is_divergent(15)[14]) and not bool(rig.tr.is_divergent(15)[13]) and bool(rig.tr.is_asymmetric().all())


def test_dead_agent_on_a_beam_gives_no_edge(oracle_mod):
    """An agent that died entering a beam is not the tile's occupant (laser.rs:184-197): no edge to it, and none from it."""
    n = 64
    rig = Rig(oracle_mod, [line_map(3)], n)
    pos = np.tile(np.array([[0, 1], [0, 2], [0, 3]], np.uint8), (n, 1, 1))
    occ = np.ones((n, 3), bool)
    occ[1::4, 1] = False   # a beneficiary that is no occupant
    occ[2::4, 0] = False   # the blocker itself is no occupant: nobody is helped
    occ[3::4, :] = False
    rig.write(pos=pos, occupant=occ)
    rig.call("dead agents", CLEAR | MARK_POS)
    got = [coop_ref.edges_of(r) for r in rig.tr.step_edges.cpu().tolist()]
    assert got == [{(0, 1), (0, 2)}, {(0, 2)}, set(), set()] * (n // 4)


def test_positions_outside_the_grid_are_on_no_tile(oracle_mod):
    n = 64
    rig = Rig(oracle_mod, [line_map(3)], n)
    pos = np.tile(np.array([[0, 1], [0, 2], [0, 3]], np.uint8), (n, 1, 1))
    pos[::2, 1] = (255, 255)
    pos[1::2, 2] = (0, 200)
    rig.write(pos=pos, occupant=np.ones((n, 3), bool))
    rig.call("outside", CLEAR | MARK_POS)
    assert [coop_ref.edges_of(r) for r in rig.tr.step_edges.cpu().tolist()] == [{(0, 2)}, {(0, 1)}] * (n // 2)


# ---------------------------------------------------------------------------------------------- several beams
def random_positions(rig, rng, on_beam=0.7):
    """Distinct cells per environment, mostly laser cells."""
    cells = [beam_cells(rig, m) for m in range(len(rig.texts))]
    free = [[(i, j) for i in range(rig.H) for j in range(rig.W) if (i, j) not in set(c)] for c in cells]
    pos = np.zeros((rig.n, rig.A, 2), np.uint8)
    for e in range(rig.n):
        m = e // rig.per
        taken = set()
        for a in range(rig.A):
            pool = cells[m] if rng.random() < on_beam else free[m]
            pool = [c for c in pool if c not in taken] or [c for c in free[m] if c not in taken]
            c = pool[int(rng.integers(len(pool)))]
            taken.add(c)
            pos[e, a] = c
    return pos


def one_row_positions(rig, rng):
    """Most agents of an environment on ONE beam row of many_sources_map, drawn per environment (distinct cells)."""
    pos = np.zeros((rig.n, rig.A, 2), np.uint8)
    for e in range(rig.n):
        row = int(rng.integers(32))
        cols = rng.permutation(6) + 1
        for a in range(rig.A):
            pos[e, a] = (row, cols[a]) if rng.random() < 0.8 else (32, a)
    return pos


@pytest.mark.parametrize("name,text", [("two_sources_of_one_colour", TWO_SOURCES_ONE_COLOUR), ("crossing", CROSSING), ("three_beam_cell", THREE_BEAMS)])
def test_random_states_on_small_maps(oracle_mod, name, text):
    """Two sources of one colour (an agent on one of its beams helps nobody on the other), an agent on the crossing of two beams of
    which it blocks one, the cell under three beams whose deepest source owns no tile."""
    rng = np.random.default_rng(7)
    rig = Rig(oracle_mod, [text], 256)
    rig.write(pos=random_positions(rig, rng), occupant=rng.random((256, rig.A)) < 0.9)
    assert rig.call(name, CLEAR | MARK_POS, rng=rng) >= 20
    assert rig.call(name + " masked", MARK_POS, mask=rng.integers(0, 2, 256), rng=rng) >= 10


def test_crossing_blocks_one_of_two_beams(oracle_mod):
    """Agent 1 on the crossing (1, 2) of its own vertical beam and agent 0's horizontal one: it helps whoever stands further down its
    own beam and is helped by agent 0 -- not the other way round."""
    rig = Rig(oracle_mod, [CROSSING], 64)
    pos = np.tile(np.array([[1, 1], [1, 2], [2, 2]], np.uint8), (64, 1, 1))
    rig.write(pos=pos, occupant=np.ones((64, 3), bool))
    rig.call("crossing", CLEAR | MARK_POS)
    assert rig.tr.edges(5, "step") == [(0, 1), (1, 2)]


def test_three_beam_cell_by_hand(oracle_mod):
    """Whatever source is deepest at (2, 2) owns no tile there: the kernel's table and the oracle's listing agree on which."""
    rig = Rig(oracle_mod, [THREE_BEAMS], 64)
    layers = [l for i, j, l in rig.lasers[0] if (i, j) == (2, 2)]
    assert len(layers) == 2 and rig.L == 3
    pos = np.tile(np.array([[2, 1], [2, 2], [3, 2]], np.uint8), (64, 1, 1))
    pos[1::2] = np.array([[3, 2], [2, 3], [2, 2]], np.uint8)
    rig.write(pos=pos, occupant=np.ones((64, 3), bool))
    rig.call("three beams", CLEAR | MARK_POS)


def test_32_sources_and_per_environment_sources(oracle_mod):
    """Bit 31 of every word in use; then colours and flags per environment, written straight into LLE_BUF_SRC_COLOUR / _ENABLED
    (colours >= n_agents included: they never block)."""
    rng = np.random.default_rng(8)
    n = 128
    rig = Rig(oracle_mod, [many_sources_map()], n)
    assert rig.L == 32 and any(l == 31 for _i, _j, l in rig.lasers[0])
    rig.write(pos=one_row_positions(rig, rng), occupant=np.ones((n, 4), bool))
    assert rig.call("32 sources", CLEAR | MARK_POS, rng=rng) >= 20
    # everybody on the last beam: source 31
    pos = np.tile(np.array([[31, 1], [31, 2], [31, 3], [31, 4]], np.uint8), (n, 1, 1))
    rig.write(pos=pos)
    rig.call("source 31", CLEAR | MARK_POS)
    assert rig.tr.edges(0, "step") == [(3, 0), (3, 1), (3, 2)]
    colours = rng.integers(0, 6, (n, 32))
    enabled = rng.integers(0, 1 << 32, n, dtype=np.int64)
    rig.write(pos=one_row_positions(rig, rng), colours=colours, enabled=enabled)
    assert rig.call("per-environment sources", CLEAR | MARK_POS, env_sources=True, rng=rng) >= 20
    rig.write(pos=pos)
    rig.call("per-environment source 31", MARK_POS, env_sources=True, mask=rng.integers(0, 2, n), rng=rng)


# ---------------------------------------------------------------------------------------------- operations
@pytest.mark.parametrize("n_agents", [1, 2, 3, 5, 8, 9, 16])
def test_every_operation_combination(oracle_mod, n_agents):
    """All 16 combinations of FINISH / CLEAR / MARK_STARTS / MARK_POS, with and without LLE_COOP_HONOUR_AUTO_RESET (bit 7 of the
    event count set in a random half), with and without env_mask, over random presets of all five arrays.  line_map: every agent
    starts on the beam, so the start edges are not empty."""
    rng = np.random.default_rng(100 + n_agents)
    n = 96
    rig = Rig(oracle_mod, [line_map(n_agents)], n)
    assert bool(rig.starts[0]) == (n_agents > 1)
    rig.write(pos=random_positions(rig, rng), occupant=rng.random((n, n_agents)) < 0.9, evcount=rng.integers(0, 4, n) | (rng.integers(0, 2, n) << 7))
    for ops in range(16):
        for honour in (False, True):
            for mask in (None, rng.integers(0, 2, n)):
                rig.call(f"ops={ops} honour={honour} mask={mask is not None}", ops, honour=honour, mask=mask, rng=rng)


def test_several_maps_in_global_memory_and_in_lds(oracle_mod):
    rng = np.random.default_rng(9)
    for per in (3, 64):
        rig = Rig(oracle_mod, [line_map(5, v) for v in (0, 1, 1, 0)], 4 * per)
        rig.write(pos=random_positions(rig, rng), occupant=np.ones((4 * per, 5), bool), evcount=rng.integers(0, 2, 4 * per) << 7)
        for ops in (MARK_POS, FINISH | CLEAR | MARK_STARTS | MARK_POS):
            rig.call(f"per={per} ops={ops}", ops, honour=True, mask=rng.integers(0, 2, 4 * per), rng=rng)


def test_state_counter_saturates(oracle_mod):
    rig = Rig(oracle_mod, [line_map(2)], 64)
    for _ in range(3):
        rig.tr.update(MARK_POS)
    assert rig.tr.episode_profile.cpu()[:, 5].tolist() == [3] * 64
    prof = rig.tr.episode_profile
    prof[:, 5] = 254
    rig.tr.update(MARK_POS)
    rig.tr.update(MARK_POS)
    assert rig.tr.episode_profile.cpu()[0].tolist() == [1, 2, 1, 1, 1, 255, 0, 1]


def test_one_update_in_a_captured_graph(oracle_mod):
    """lle_coop_update allocates nothing and never synchronises: one update captured into a graph, replayed over two states."""
    rng = np.random.default_rng(11)
    n = 96
    rig = Rig(oracle_mod, [line_map(5)], n)
    dev = rig.bw.device
    args = rig.tr.make_args(CLEAR | MARK_POS)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):   # warm-up on the side stream: the kernel's code object is loaded outside the capture
        rig.tr.launch(args)
    side.synchronize()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rig.tr.launch(args)   # (the current stream is the capturing one)
    for k in range(2):
        rig.write(pos=random_positions(rig, rng), occupant=rng.random((n, 5)) < 0.9)
        graph.replay()
        torch.cuda.synchronize(dev)
        want = [coop_ref.rows(rig.state_edges(e, False), 5) for e in range(n)]
        assert rig.tr.step_edges.cpu().tolist() == want and rig.tr.episode_edges.cpu().tolist() == want, f"replay {k}"
        assert any(any(r) for r in want)


# ---------------------------------------------------------------------------------------------- ABI refusals
def test_refusals(oracle_mod):
    from lle_amd import Map
    from lle_amd.cooperation import UpdateArgs
    rig = Rig(oracle_mod, [line_map(3)], 64)
    L, h, st = rig.lib, rig.tr.h, rig.bw._stream()
    before = [v.cpu().clone() for v in rig.views]

    def refused(rc, text):
        assert rc in (LLE_ERR_NULL, LLE_ERR_ARG) and text in L.lle_coop_last_error().decode(), (rc, L.lle_coop_last_error())
    ok = UpdateArgs(C.sizeof(UpdateArgs), MARK_POS, 0, 0, None)
    refused(L.lle_coop_update(h, None, st), "NULL")
    refused(L.lle_coop_update(None, C.byref(ok), st), "NULL")
    refused(L.lle_coop_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs) - 8, MARK_POS, 0, 0, None)), st), "struct_bytes")
    refused(L.lle_coop_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs), 16, 0, 0, None)), st), "unknown operation or flag")
    refused(L.lle_coop_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs), MARK_POS, 4, 0, None)), st), "unknown operation or flag")
    # (the Map objects must outlive the calls: `Map(...).h` alone would free the map before the library reads it)
    swapped, wider, moved_beam = Map("L0E S0 S2 S1 @\nX X X . ."), Map(line_map(4)), Map(". S0 S1 S2 @\nL0E X X X .")
    for other in (swapped, wider, moved_beam):  # the starts moved, another shape, the beam moved
        refused(L.lle_coop_update_map(h, 0, other.h, st), "not a recompilation")
    refused(L.lle_coop_update_map(h, 1, rig.bw.map.h, st), "map_index")
    refused(L.lle_coop_update_map(h, 0, None, st), "NULL")
    assert L.lle_coop_buffer(h, 5) is None and L.lle_coop_buffer(h, -1) is None
    handles = (C.c_void_p * 2)(rig.bw.map.h, rig.bw.map.h)
    assert L.lle_coop_create(rig.bw.h, handles, 2, st) is None and "n_maps" in L.lle_coop_last_error().decode()
    assert L.lle_coop_create(None, handles, 1, st) is None and L.lle_coop_create(rig.bw.h, None, 1, st) is None
    torch.cuda.synchronize(rig.bw.device)
    for v, b in zip(rig.views, before):
        assert torch.equal(v.cpu(), b), "a refused call wrote"
    assert L.lle_coop_update_map(h, 0, rig.bw.map.h, st) == 0  # the same map is a recompilation of itself


def test_start_on_beam_with_per_environment_sources(oracle_mod):
    """The start edges of a map with a start cell on a laser cell depend on the colours: with per-environment sources
    LLE_COOP_MARK_STARTS and LLE_COOP_HONOUR_AUTO_RESET are refused, and the masked host reset followed by FINISH | CLEAR | MARK_POS
    on the reset state is exact."""
    n = 64
    rig = Rig(oracle_mod, [START_ON_BEAM], n)
    assert rig.starts[0] == {(0, 1)}
    colours = torch.zeros((n, 1), dtype=torch.uint8)
    colours[1::2] = 1   # agent 1's colour: at reset agent 0 ... stands on a foreign beam (blocked or not, it is the state the batch holds)
    with pytest.raises(RuntimeError, match="per-environment sources"):
        rig.tr.update(MARK_STARTS, env_sources=True)
    with pytest.raises(RuntimeError, match="per-environment sources"):
        rig.tr.update(MARK_POS, honour_auto_reset=True, env_sources=True)
    rig.tr.update(MARK_STARTS | MARK_POS, honour_auto_reset=True, env_sources=False)  # the map's own sources: served
    # the masked host reset: env 0, 2, ... keep colour 0, the odd ones would put agent 0's start on agent 1's beam -- refused per env
    # by lle_batch_set_sources (LLE_ENV_COLOUR_CROSSES_START), which leaves them with the map's colour
    rig.bw.set_sources(colours=colours, reset_first=True)
    rig.tr.reset()
    torch.cuda.synchronize(rig.bw.device)
    bits = rig.bw.bits.cpu().numpy()
    pos = rig.bw.pos.cpu().numpy()
    cols = rig.bw.src_colour.cpu().numpy()[:, rig.first_words]
    en = rig.bw.src_enabled.cpu().numpy()
    for e in range(n):
        occ = [(int(bits[e]) >> (32 + a)) & 1 for a in range(2)]
        want = coop_ref.detect_state(rig.lasers[0], pos[e], occ, [int(cols[e, 0])], [int(en[e]) & 1])
        assert set(rig.tr.edges(e, "step")) == want and set(rig.tr.edges(e, "episode")) == want, e
    assert rig.tr.last_profile.cpu()[:, 7].tolist() == [1] * n
