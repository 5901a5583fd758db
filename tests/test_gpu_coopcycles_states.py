"""The coopcycles kernel (liblle_coopcycles.so, lle_amd/coopcycles/coopcycles.hip) on SYNTHETIC edges, against the restatement from the
definition of a trail (tests/coopcycles_ref.py over tests/cycles_ref.layer_update), exactly.

lle_coopcycles_update depends only on LLE_COOP_STEP_EDGES, bit 7 of LLE_BUF_EVCOUNT, LLE_BUF_ERR, the handle's four arrays and the start
edges of the maps.  The tests write rows straight into the LLE_COOP_STEP_EDGES view and bytes into the batch's two buffers, launch the
coopcycles update ALONE (no coop launch rewrites the rows) and compare all four arrays with torch.equal after every call -- the rows of
the environments outside the mask included -- and the guard bytes around the arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import coopcycles_ref, cooptrails_ref
from tests.coopcycles_ref import CLEAR, FINISH, MARK_POS, MARK_STARTS
from tests.test_gpu_coop import line_map
from tests.test_gpu_coop_states import _raw

pytestmark = pytest.mark.gpu

LLE_ERR_NULL, LLE_ERR_ARG = -1, -2
GUARD = 256  # LLE_COOP_GUARD_BYTES
NAMES = ("episode_closed", "last_closed", "episode_cprofile", "last_cprofile")


def rows_of(edges, n_agents):
    out = [0] * n_agents
    for h, b in edges:
        out[h] |= 1 << b
    return out


def edges_of(rows):
    return {(h, b) for h, row in enumerate(rows) for b in range(32) if (int(row) >> b) & 1}


class Rig:
    """A BatchedWorld of line_map(A) variants (map m owns block m: every agent starts on the beam agent 0 blocks, so the start edges are
    0 -> 1 .. 0 -> A - 1), a ClosedTrailCooperationTracker on it and one coopcycles_ref.EnvRef per environment."""

    def __init__(self, n_agents, n, n_maps=1):
        from lle_amd import BatchedWorld
        from lle_amd.coopcycles import ClosedTrailCooperationTracker, lib, words_of
        texts = [line_map(n_agents, m % 2) for m in range(n_maps)]
        self.bw = BatchedWorld(texts if n_maps > 1 else texts[0], n)
        self.tr = ClosedTrailCooperationTracker(self.bw)
        self.lib = lib()
        self.n, self.A, self.W, self.dev = int(n), int(n_agents), words_of(n_agents), self.bw.device
        self.starts = {(0, b) for b in range(1, n_agents)}
        assert all(set(self.tr.start_edges(m)) == self.starts for m in range(n_maps))
        self.refs = [coopcycles_ref.EnvRef(n_agents) for _ in range(n)]
        self.views = [self.tr.episode_closed, self.tr.last_closed, self.tr.episode_cprofile, self.tr.last_cprofile]
        assert self.tr.episode_closed.shape == (self.W, n) and self.tr.n_words == self.W
        self.guards = []
        for which, v in enumerate(self.views):
            assert v.data_ptr() == self.lib.lle_coopcycles_buffer(self.tr.ch, which) and v.is_contiguous() and v.data_ptr() % 256 == 0
            nbytes = v.numel() * v.element_size()
            self.guards.append((_raw(v.data_ptr() - GUARD, GUARD, self.dev), _raw(v.data_ptr() + nbytes, GUARD - nbytes % GUARD if nbytes % GUARD else GUARD, self.dev)))
        self.ev = np.zeros(n, np.uint8)
        self.err = np.zeros(n, np.uint8)
        self.rows = np.zeros((n, n_agents), np.int32)

    def write(self, rows=None, evcount=None, err=None):
        if rows is not None:
            self.rows = np.ascontiguousarray(rows, np.int64).astype(np.uint32).view(np.int32).reshape(self.n, self.A)
            self.tr.step_edges.copy_(torch.from_numpy(self.rows).to(self.dev))
        if evcount is not None:
            self.ev = np.ascontiguousarray(evcount, np.uint8).reshape(self.n)
            self.bw.evcount.copy_(torch.from_numpy(self.ev).to(self.dev))
        if err is not None:
            self.err = np.ascontiguousarray(err, np.uint8).reshape(self.n)
            self.bw.err.copy_(torch.from_numpy(self.err).to(self.dev))
        torch.cuda.synchronize(self.dev)

    def planted(self, edges):
        """The same rows in every environment."""
        self.write(rows=np.tile(np.array(rows_of(edges, self.A), np.int64), (self.n, 1)))

    def expect(self):
        cols = list(zip(*[r.arrays() for r in self.refs]))
        return [torch.tensor(cols[0], dtype=torch.int32).t().contiguous(), torch.tensor(cols[1], dtype=torch.int32).t().contiguous(),
                torch.tensor(cols[2], dtype=torch.uint8), torch.tensor(cols[3], dtype=torch.uint8)]

    def snapshot(self):
        torch.cuda.synchronize(self.dev)
        return [v.cpu().clone() for v in self.views]

    def check_guards(self, where):
        for lo, hi in self.guards:
            assert int(lo.max()) == 0 and int(hi.max()) == 0, f"{where}: a guard byte was written"

    def check(self, where, want=None):
        torch.cuda.synchronize(self.dev)
        for name, got, exp in zip(NAMES, [v.cpu() for v in self.views], want or self.expect()):
            if not torch.equal(got, exp):
                diff = got != exp
                bad = int((diff.any(dim=0) if name.endswith("closed") else diff.any(dim=1)).nonzero()[0])
                got_b, exp_b = (got[:, bad], exp[:, bad]) if name.endswith("closed") else (got[bad], exp[bad])
                raise AssertionError(f"{where}: {name} differs in env {bad}: {got_b.tolist()} != {exp_b.tolist()} (rows {self.rows[bad].tolist()}, "
                                     f"evcount {self.ev[bad]}, err {self.err[bad]})")
        self.check_guards(where)

    def call(self, where, ops, honour=False, skip=False, mask=None, compare=True, beyond=()):
        """One lle_coopcycles_update alone; every array compared, the unselected rows and the guards untouched.  `beyond`: environments
        whose state the restatement is not asked about (it enumerates every trail and knows no budget)."""
        m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(self.dev)
        self.tr.launch_closed(self.tr.make_closed_args(ops, honour, m, skip))
        for e, r in enumerate(self.refs):
            if (mask is not None and not mask[e]) or e in beyond:
                continue
            r.update(ops, edges_of(self.rows[e].view(np.uint32)), self.starts, was_reset=honour and bool(self.ev[e] & 0x80),
                     refused=skip and bool(self.err[e]))
        if compare:
            self.check(where)

    def orders(self, last=False):
        """Per environment: the closed orders of the bit set on the device, as a sorted list."""
        return [[k for k in range(8) if (int(b) >> k) & 1] for b in self.tr.closed_orders(last).cpu().tolist()]


def random_rows(rng, n, A, stray=True):
    """At most 5 arcs per environment (such a state stays far inside the budget), most environments none; with `stray`, now and then a
    self-loop or a bit of an agent the map does not have, which the kernel drops."""
    rows = np.zeros((n, A), np.int64)
    for e in range(n):
        for _ in range(int(rng.choice([0, 0, 0, 1, 2, 3, 5]))):
            h, b = rng.choice(A, 2, replace=False)
            rows[e, h] |= 1 << int(b)
        if stray and rng.random() < 0.2:
            h = int(rng.integers(A))
            rows[e, h] |= (1 << h) | ((1 << int(rng.integers(A, 17))) & 0xFFFF)
    return rows


# ---------------------------------------------------------------------------------------------- operations, flags, masks
@pytest.mark.parametrize("n_agents,n", [(2, 257), (3, 63), (4, 65), (5, 257), (6, 63), (6, 1), (4, 1)])
def test_every_operation_combination(n_agents, n):
    """All 16 combinations of FINISH / CLEAR / MARK_STARTS / MARK_POS x HONOUR_AUTO_RESET x SKIP_REFUSED, with and without a mask with
    holes, in a seeded order on ONE trajectory per environment: the values carry over from call to call.  Both word classes, a ragged
    last workgroup, a wavefront boundary, a batch of one.  After every call is_interdependent(2) is the parent's derivation from the
    flattened edges (a pair with both directions among the arcs the episode entered)."""
    rng = np.random.default_rng(400 + 10 * n_agents + n)
    rig = Rig(n_agents, n)
    order = [(ops, honour, skip, masked) for ops in range(16) for honour in (False, True) for skip in (False, True) for masked in (False, True)]
    two_layers = closed = mutual = 0
    for k in rng.permutation(len(order)):
        ops, honour, skip, masked = order[int(k)]
        rig.write(rows=random_rows(rng, n, n_agents), evcount=rng.integers(0, 4, n) | (rng.integers(0, 2, n) << 7), err=rng.integers(0, 3, n) * rng.integers(0, 2, n))
        mask = rng.integers(0, 2, n) if masked else None
        rig.call(f"ops={ops} honour={honour} skip={skip} masked={masked}", ops, honour, skip, mask)
        two_layers += sum(r.touched and r.layers >= 2 for r in rig.refs)
        closed += sum(max(r.orders(), default=0) >= 3 for r in rig.refs)
        flat = [cooptrails_ref.is_mutual(r.flat) for r in rig.refs]
        mutual += sum(flat)
        assert rig.tr.is_interdependent(2).cpu().tolist() == [r.episode_valid and f for r, f in zip(rig.refs, flat)]
    assert bool(rig.tr.closed_exact().all()) and bool(rig.tr.closed_exact(last=True).all())
    assert mutual > 0 and (n == 1 or two_layers > 0) and (n_agents == 2 or n == 1 or closed > 0), (two_layers, closed, mutual)


def test_several_maps():
    rng = np.random.default_rng(5)
    rig = Rig(5, 4 * 7, n_maps=4)
    for k in range(12):
        rig.write(rows=random_rows(rng, rig.n, 5), evcount=rng.integers(0, 2, rig.n) << 7)
        rig.call(f"call {k}", int(rng.integers(16)) | MARK_STARTS, honour=True, mask=rng.integers(0, 2, rig.n))
    assert any(r.count >= 2 for r in rig.refs)


# ---------------------------------------------------------------------------------------------- named sequences
@pytest.mark.parametrize("n_agents", [3, 5])
def test_three_cycle_inside_one_state(n_agents):
    rig = Rig(n_agents, 65)
    rig.planted({(0, 1), (1, 2), (2, 0)})
    rig.call("cycle", CLEAR | MARK_POS)
    assert rig.orders() == [[3]] * 65 and bool(rig.tr.is_interdependent(3).all()) and not bool(rig.tr.is_interdependent(2).any())
    assert not bool(rig.tr.is_interdependent(3, last=True).any())  # no episode has finished: the row is not valid
    assert rig.tr.triples(64) == set(rig.refs[64].R) and (1, 1, frozenset({0, 1, 2})) in rig.tr.triples(0)
    assert not bool(rig.tr.is_interdependent(n_agents + 1).any()) and not bool(rig.tr.is_interdependent(7).any()) and not bool(rig.tr.is_interdependent(1).any())


@pytest.mark.parametrize("n_agents", [3, 6])
def test_three_arcs_over_three_states_in_order_and_against_time(n_agents):
    """0 -> 1, then 1 -> 2, then 2 -> 0 closes over three agents; 2 -> 0, then 1 -> 2, then 0 -> 1 are the same flattened edges and no
    trail of two: the times decrease."""
    rig = Rig(n_agents, 65)
    rig.call("clear", CLEAR)
    for k, arc in enumerate([(0, 1), (1, 2), (2, 0)]):
        rig.planted({arc})
        rig.call(f"in order {k}", MARK_POS)
        assert rig.orders() == [[3] if k == 2 else []] * 65
    rig.call("finish and clear", FINISH | CLEAR)
    assert rig.orders() == [[]] * 65 and rig.orders(last=True) == [[3]] * 65 and bool(rig.tr.is_interdependent(3, last=True).all())
    for k, arc in enumerate([(2, 0), (1, 2), (0, 1)]):
        rig.planted({arc})
        rig.call(f"against time {k}", MARK_POS)
    assert rig.orders() == [[]] * 65 and rig.tr.episode_cprofile.cpu()[0].tolist() == [0, 3, 0, 1]


def test_figure_eight_closes_over_three_agents_without_a_three_cycle():
    """a <-> b, then b <-> c, then b -> a: a -> b -> c -> b -> a closes over 3 agents though no 3-cycle exists; orders {2, 3}.  (Anchored
    at b the figure eight b -> a -> b -> c -> b is closed after the second state already; anchored at a only after the third.)"""
    rig = Rig(4, 65)
    rig.call("clear", CLEAR)
    eight = (0, 0, frozenset({0, 1, 2}))
    for k, arcs in enumerate([{(0, 1), (1, 0)}, {(1, 2), (2, 1)}, {(1, 0)}]):
        rig.planted(arcs)
        rig.call(f"state {k}", MARK_POS)
        assert rig.orders() == [[2, 3] if k >= 1 else [2]] * 65
        assert (eight in rig.tr.triples(3)) == (k == 2) and ((1, 1, frozenset({0, 1, 2})) in rig.tr.triples(64)) == (k >= 1)
    assert bool(rig.tr.is_mutual().all()) and not bool(rig.tr.is_interdependent(4).any())


def test_ring_over_six_agents():
    """One state holds a -> a + 1 for all six agents: the only closed trail is the ring, order 6; the triples of the last pair reach
    the last value word."""
    rig = Rig(6, 65)
    rig.planted({(a, (a + 1) % 6) for a in range(6)})
    rig.call("ring", CLEAR | MARK_POS)
    assert rig.orders() == [[6]] * 65 and bool(rig.tr.is_interdependent(6).all())
    assert int((rig.tr.episode_closed[20] != 0).sum()) == 65 and coopcycles_ref.encode(rig.refs[0].R, 6)[20] != 0


def test_reset_environment_chains_start_layer_and_step_layer():
    """Bit 7: FINISH | CLEAR | MARK_STARTS ahead of MARK_POS -- two layer updates in one launch; the start edge 0 -> 1, the state's
    1 -> 2 and 2 -> 0 close over three agents only where both layers were entered."""
    for n_agents in (3, 5):
        rig = Rig(n_agents, 65)
        rig.planted({(2, 0)})
        rig.call("before", CLEAR | MARK_POS)
        rig.planted({(1, 2), (2, 0)})
        rig.write(evcount=(np.arange(65) % 2 << 7) | 1)
        rig.call("reset in every other environment", MARK_POS, honour=True)
        assert rig.orders()[:2] == [[], [2, 3]] == [rig.refs[0].orders(), rig.refs[1].orders()] and rig.refs[1].layers == 2
        assert rig.tr.last_cprofile.cpu()[:2].tolist() == [[0, 0, 0, 0], [0, 1, 0, 1]]


def test_refused_environment_keeps_its_value():
    rig = Rig(3, 65)
    rig.planted({(0, 1)})
    rig.call("first", CLEAR | MARK_POS)
    before = rig.snapshot()
    rig.planted({(1, 0)})
    rig.write(err=np.arange(65) % 3 == 0)
    rig.call("refused in every third", MARK_POS, skip=True)
    now = rig.snapshot()
    assert torch.equal(now[0][:, ::3], before[0][:, ::3]) and rig.orders()[:3] == [[], [2], [2]]
    rig.call("without the flag the layer is entered", MARK_POS)
    assert rig.orders()[0] == [2]


def test_finish_copies_every_word_and_clear_empties():
    rig = Rig(6, 63)
    rig.planted({(a, (a + 1) % 6) for a in range(6)} | {(5, 4)})
    rig.call("something in most words", CLEAR | MARK_POS)
    value = rig.snapshot()[0]
    assert int((value != 0).any(dim=1).sum()) >= 18 and bool((value[20] != 0).all())
    rig.call("finish", FINISH)
    now = rig.snapshot()
    assert torch.equal(now[1], value) and torch.equal(now[0], value) and torch.equal(now[3], now[2])
    rig.call("clear", CLEAR)
    now = rig.snapshot()
    assert int(now[0].abs().max()) == 0 and torch.equal(now[1], value) and now[2].tolist() == [[0, 0, 0, 1]] * 63


# ---------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize("n_agents", [4, 5])
def test_complete_digraph_on_4_agents_is_dense(n_agents):
    """12 arcs allow far more than 4 096 extensions: the layer is dropped WHOLE -- the value equals the value before it --, the dense
    mark is set, stays through FINISH and goes with CLEAR; the environments between the dense ones are exact."""
    n = 65
    rig = Rig(n_agents, n)
    rig.planted({(0, 1), (1, 2)})
    rig.call("a value to keep", CLEAR | MARK_POS)
    before = rig.snapshot()
    full = rows_of({(h, b) for h in range(4) for b in range(4) if h != b}, n_agents)
    rows = np.tile(np.array(rows_of({(2, 0)}, n_agents), np.int64), (n, 1))
    rows[::2] = full
    rig.write(rows=rows)
    rig.call("complete digraph in every other environment", MARK_POS, compare=False, beyond=range(0, n, 2))
    now = rig.snapshot()
    assert torch.equal(now[0][:, ::2], before[0][:, ::2]), "a dropped layer changed the value"
    assert now[2][::2].tolist() == [[0, 2, 1, 1]] * (n - n // 2) and now[2][1::2].tolist() == [[1 << 3, 2, 0, 1]] * (n // 2)
    want = rig.expect()  # (of the neighbours: the restatement was not asked about the dense environments)
    assert torch.equal(now[0][:, 1::2], want[0][:, 1::2]), "a neighbour of a dense environment is not exact"
    assert rig.tr.closed_exact().cpu().tolist() == [bool(e % 2) for e in range(n)]
    rig.check_guards("dense")
    rig.write(rows=np.zeros((n, n_agents), np.int64))
    rig.call("sticky", FINISH | MARK_POS, compare=False)
    after = rig.snapshot()
    assert after[2][::2, 2].tolist() == [1] * (n - n // 2) and after[3][::2, 2].tolist() == [1] * (n - n // 2) and int(after[3][1::2, 2].max()) == 0
    assert torch.equal(after[0], now[0]) and torch.equal(after[1], now[0])
    assert not bool(rig.tr.closed_exact(last=True)[0]) and bool(rig.tr.closed_exact(last=True)[1])
    rig.call("cleared", CLEAR, compare=False)
    assert rig.snapshot()[2].tolist() == [[0, 0, 0, 1]] * n and bool(rig.tr.closed_exact().all())
    rig.check_guards("cleared")


# ---------------------------------------------------------------------------------------------- capture, refusals
def test_one_update_in_a_captured_graph():
    """lle_coopcycles_update allocates nothing and never synchronises: one update captured into a graph, replayed over two states."""
    rig = Rig(5, 96)
    args = rig.tr.make_closed_args(MARK_POS)
    side = torch.cuda.Stream(device=rig.dev)
    side.wait_stream(torch.cuda.current_stream(rig.dev))
    with torch.cuda.stream(side):   # warm-up on the side stream: the kernel's code object is loaded outside the capture
        rig.tr.launch_closed(rig.tr.make_closed_args(CLEAR))
    side.synchronize()
    torch.cuda.current_stream(rig.dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rig.tr.launch_closed(args)   # (the current stream is the capturing one)
    for edges in ({(0, 1), (1, 2)}, {(2, 3), (3, 0)}):
        rig.planted(edges)
        graph.replay()
        torch.cuda.synchronize(rig.dev)
    assert rig.orders() == [[4]] * 96 and rig.tr.episode_cprofile.cpu()[95].tolist() == [1 << 4, 2, 0, 1]


def test_refusals():
    from lle_amd import BatchedWorld, CooperationTracker
    from lle_amd.coopcycles import UpdateArgs
    rig = Rig(3, 64)
    L, h, st = rig.lib, rig.tr.ch, rig.bw._stream()
    rig.planted({(0, 1)})
    rig.call("something to lose", CLEAR | MARK_POS)
    before = rig.snapshot()

    def refused(rc, text, codes=(LLE_ERR_NULL, LLE_ERR_ARG)):
        assert rc in codes and text in L.lle_coopcycles_last_error().decode(), (rc, L.lle_coopcycles_last_error())
    ok = UpdateArgs(C.sizeof(UpdateArgs), MARK_POS, 0, 0, None)
    refused(L.lle_coopcycles_update(h, None, st), "NULL")
    refused(L.lle_coopcycles_update(None, C.byref(ok), st), "NULL")
    refused(L.lle_coopcycles_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs) - 8, MARK_POS, 0, 0, None)), st), "struct_bytes")
    refused(L.lle_coopcycles_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs), 16, 0, 0, None)), st), "unknown operation or flag")
    refused(L.lle_coopcycles_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs), MARK_POS, 4, 0, None)), st), "unknown operation or flag")
    refused(L.lle_coopcycles_update_map(h, 1, st), "map_index")
    refused(L.lle_coopcycles_update_map(h, -1, st), "map_index")
    assert L.lle_coopcycles_buffer(h, 4) is None and L.lle_coopcycles_buffer(h, -1) is None
    assert L.lle_coopcycles_create(None, rig.tr.h, st) is None and L.lle_coopcycles_create(rig.bw.h, None, st) is None
    seven = BatchedWorld(line_map(7), 8)
    coop7 = CooperationTracker(seven)
    assert L.lle_coopcycles_create(seven.h, coop7.h, seven._stream()) is None
    assert "at most 6 agents" in L.lle_coopcycles_last_error().decode()
    from lle_amd.coopcycles import ClosedTrailCooperationTracker
    with pytest.raises(ValueError, match="at most 6 agents"):
        ClosedTrailCooperationTracker(seven)
    torch.cuda.synchronize(rig.dev)
    for v, b in zip(rig.views, before):
        assert torch.equal(v.cpu(), b), "a refused call wrote"
    assert L.lle_coopcycles_update_map(h, 0, st) == 0
    rig.tr.update_map(0)  # (all three handles, through the tracker)
    rig.call("the start edges are still there", CLEAR | MARK_STARTS)
    assert rig.tr.triples(0) == {(0, 1, frozenset({0, 1})), (0, 2, frozenset({0, 2}))}
