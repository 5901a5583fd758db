"""The cooptrails kernel (liblle_cooptrails.so, lle_amd/cooptrails/cooptrails.hip) on SYNTHETIC edges, against the restatement from the
definition of a trail (tests/cooptrails_ref.py), exactly.

lle_cooptrails_update depends only on LLE_COOP_STEP_EDGES, bit 7 of LLE_BUF_EVCOUNT, LLE_BUF_ERR, the handle's four arrays and the start
edges of the maps.  The tests write rows straight into the LLE_COOP_STEP_EDGES view and bytes into the batch's two buffers, launch the
trails update ALONE (no coop launch rewrites the rows) and compare all four arrays with torch.equal after every call -- the rows of the
environments outside the mask included -- and the guard bytes around the arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cooptrails_ref
from tests.cooptrails_ref import CLEAR, FINISH, MARK_POS, MARK_STARTS
from tests.test_gpu_coop import line_map
from tests.test_gpu_coop_states import _raw

pytestmark = pytest.mark.gpu

LLE_ERR_NULL, LLE_ERR_ARG = -1, -2
GUARD = 256  # LLE_COOP_GUARD_BYTES
NAMES = ("episode_trails", "last_trails", "episode_tprofile", "last_tprofile")


def rows_of(edges, n_agents):
    out = [0] * n_agents
    for h, b in edges:
        out[h] |= 1 << b
    return out


def edges_of(rows):
    return {(h, b) for h, row in enumerate(rows) for b in range(32) if (int(row) >> b) & 1}


class Rig:
    """A BatchedWorld of line_map(A) variants (map m owns block m: every agent starts on the beam agent 0 blocks, so the start edges are
    0 -> 1 .. 0 -> A - 1), a TemporalCooperationTracker on it and one cooptrails_ref.EnvRef per environment."""

    def __init__(self, n_agents, n, n_maps=1):
        from lle_amd import BatchedWorld
        from lle_amd.cooptrails import TemporalCooperationTracker, lib
        texts = [line_map(n_agents, m % 2) for m in range(n_maps)]
        self.bw = BatchedWorld(texts if n_maps > 1 else texts[0], n)
        self.tr = TemporalCooperationTracker(self.bw)
        self.lib = lib()
        self.n, self.A, self.dev = int(n), int(n_agents), self.bw.device
        self.starts = {(0, b) for b in range(1, n_agents)}
        assert all(set(self.tr.start_edges(m)) == self.starts for m in range(n_maps))
        self.refs = [cooptrails_ref.EnvRef(n_agents) for _ in range(n)]
        self.views = [self.tr.episode_trails, self.tr.last_trails, self.tr.episode_tprofile, self.tr.last_tprofile]
        self.guards = []
        for which, v in enumerate(self.views):
            assert v.data_ptr() == self.lib.lle_cooptrails_buffer(self.tr.th, which) and v.is_contiguous() and v.data_ptr() % 256 == 0
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
        return [torch.tensor(cols[0], dtype=torch.int64), torch.tensor(cols[1], dtype=torch.int64),
                torch.tensor(cols[2], dtype=torch.uint8), torch.tensor(cols[3], dtype=torch.uint8)]

    def check(self, where, want=None):
        torch.cuda.synchronize(self.dev)
        for name, got, exp in zip(NAMES, [v.cpu() for v in self.views], want or self.expect()):
            if not torch.equal(got, exp):
                bad = int((got != exp).reshape(self.n, -1).any(dim=1).nonzero()[0])
                raise AssertionError(f"{where}: {name} differs in env {bad}: {got[bad].tolist()} != {exp[bad].tolist()} (rows {self.rows[bad].tolist()}, "
                                     f"evcount {self.ev[bad]}, err {self.err[bad]})")
        for lo, hi in self.guards:
            assert int(lo.max()) == 0 and int(hi.max()) == 0, f"{where}: a guard byte was written"

    def call(self, where, ops, honour=False, skip=False, mask=None, compare=True):
        """One lle_cooptrails_update alone; every array compared, the unselected rows and the guards untouched."""
        m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(self.dev)
        self.tr.launch_trails(self.tr.make_trails_args(ops, honour, m, skip))
        for e, r in enumerate(self.refs):
            if mask is not None and not mask[e]:
                continue
            r.update(ops, edges_of(self.rows[e].view(np.uint32)), self.starts, was_reset=honour and bool(self.ev[e] & 0x80),
                     refused=skip and bool(self.err[e]))
        if compare:
            self.check(where)


def random_rows(rng, n, A, stray=True):
    """At most 5 arcs per environment (a state of up to 6 arcs never exhausts the budget), most environments none; with `stray`, now and
    then a self-loop or a bit of an agent the map does not have, which the kernel drops."""
    rows = np.zeros((n, A), np.int64)
    if A < 2:
        return rows | (rng.integers(0, 2, (n, A)) * 0xFFFE if stray else 0)
    for e in range(n):
        for _ in range(int(rng.choice([0, 0, 0, 1, 2, 3, 5]))):
            h, b = rng.choice(A, 2, replace=False)
            rows[e, h] |= 1 << int(b)
        if stray and rng.random() < 0.2:
            h = int(rng.integers(A))
            rows[e, h] |= (1 << h) | ((1 << int(rng.integers(A, 17))) & 0xFFFF)
    return rows


# ---------------------------------------------------------------------------------------------- operations, flags, masks
@pytest.mark.parametrize("n_agents,n", [(1, 65), (2, 257), (3, 63), (4, 65), (5, 257), (8, 63), (9, 65), (16, 257)])
def test_every_operation_combination(n_agents, n):
    """All 16 combinations of FINISH / CLEAR / MARK_STARTS / MARK_POS x HONOUR_AUTO_RESET x SKIP_REFUSED, with and without a mask with
    holes, one after the other on ONE trajectory per environment: the values carry over from call to call.  Every G (idle lanes at 3, 5
    and 9 agents), a ragged last workgroup."""
    rng = np.random.default_rng(200 + n_agents)
    rig = Rig(n_agents, n)
    order = [(ops, honour, skip, masked) for ops in range(16) for honour in (False, True) for skip in (False, True) for masked in (False, True)]
    seen_two_layers = 0
    for k in rng.permutation(len(order)):
        ops, honour, skip, masked = order[int(k)]
        rig.write(rows=random_rows(rng, n, n_agents), evcount=rng.integers(0, 4, n) | (rng.integers(0, 2, n) << 7), err=rng.integers(0, 3, n) * rng.integers(0, 2, n))
        mask = rng.integers(0, 2, n) if masked else None
        rig.call(f"ops={ops} honour={honour} skip={skip} masked={masked}", ops, honour, skip, mask)
        seen_two_layers += sum(r.touched and r.count >= 2 for r in rig.refs)
    assert n_agents == 1 or (seen_two_layers > 0 and max(max(r.lengths()) for r in rig.refs) >= 2)


@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("n_agents", [3, 16])
def test_batch_sizes_over_a_long_episode(n_agents, n):
    """40 marked states without a clear: the lengths grow into the saturation in some environments, whatever the batch size."""
    rng = np.random.default_rng(300 + n)
    rig = Rig(n_agents, n)
    rig.call("clear", CLEAR)
    for t in range(40):
        rows = random_rows(rng, n, n_agents, stray=False)
        rows[0] = rows_of({(t % n_agents, (t + 1) % n_agents)}, n_agents)  # environment 0: a chain, one arc per state
        err = rng.integers(0, 2, n) * (rng.random(n) < 0.1)
        err[0] = 0  # (the chain of environment 0 loses no state)
        rig.write(rows=rows, err=err)
        rig.call(f"t={t}", MARK_POS, skip=True, mask=None if t % 3 else rng.integers(0, 2, n) | (np.arange(n) == 0), compare=t % 8 == 7)
    assert max(rig.refs[0].lengths()) == 15 and int(rig.tr.longest_trail()[0]) == 15


def test_several_maps():
    rng = np.random.default_rng(5)
    rig = Rig(5, 4 * 7, n_maps=4)
    for k in range(12):
        rig.write(rows=random_rows(rng, rig.n, 5), evcount=rng.integers(0, 2, rig.n) << 7)
        rig.call(f"call {k}", int(rng.integers(16)) | MARK_STARTS, honour=True, mask=rng.integers(0, 2, rig.n))


# ---------------------------------------------------------------------------------------------- named sequences
def test_two_arcs_of_one_state_chain():
    rig = Rig(3, 65)
    rig.planted({(0, 1), (1, 2)})
    rig.call("chain", CLEAR | MARK_POS)
    assert rig.tr.trail_lengths().cpu().tolist() == [[0, 1, 2]] * 65 and bool(rig.tr.is_sequential(2).all()) and not bool(rig.tr.is_sequential(3).any())
    assert not bool(rig.tr.is_sequential(2, last=True).any())  # no episode has finished: the row is not valid


def test_mutual_pair_in_one_state():
    rig = Rig(2, 65)
    rig.planted({(0, 1), (1, 0)})
    rig.call("pair", CLEAR | MARK_POS)
    assert rig.tr.trail_lengths().cpu().tolist() == [[2, 2]] * 65
    for state in range(2, 10):  # held: two more per state, saturating in the eighth
        rig.call(f"state {state}", MARK_POS)
        assert rig.tr.longest_trail().cpu().tolist() == [min(2 * state, 15)] * 65
    assert rig.tr.episode_tprofile.cpu()[0].tolist() == [15, 9, 0, 1] and bool(rig.tr.trails_exact().all())


def test_three_cycle_repeated_to_saturation():
    rig = Rig(3, 63)
    rig.planted({(0, 1), (1, 2), (2, 0)})
    rig.call("first", CLEAR | MARK_POS)
    for want in (6, 9, 12, 15, 15):
        rig.call(f"to {want}", MARK_POS)
        assert rig.tr.trail_lengths().cpu().tolist() == [[want] * 3] * 63
    with pytest.raises(ValueError, match="saturate"):
        rig.tr.is_sequential(16)
    assert bool(rig.tr.is_sequential(15).all())


def test_decreasing_times_longest_1():
    """b -> c, then a -> b: the flattened edges chain, the times do not."""
    rig = Rig(3, 65)
    rig.planted({(1, 2)})
    rig.call("later edge first", CLEAR | MARK_POS)
    rig.planted({(0, 1)})
    rig.call("earlier edge second", MARK_POS)
    assert rig.tr.trail_lengths().cpu().tolist() == [[0, 1, 1]] * 65 and not bool(rig.tr.is_sequential(2).any())
    rig.planted({(1, 2)})
    rig.call("again in order", MARK_POS)
    assert rig.tr.longest_trail().cpu().tolist() == [2] * 65


def test_reset_environment_chains_start_layer_and_step_layer():
    """Bit 7: FINISH | CLEAR | MARK_STARTS ahead of MARK_POS -- two layer updates in one launch; the start edge 0 -> 1 and the state's
    1 -> 2 chain.  The other environments only get the state's arc."""
    rig = Rig(3, 65)
    rig.planted({(2, 0)})
    rig.call("before", CLEAR | MARK_POS)
    rig.planted({(1, 2)})
    rig.write(evcount=(np.arange(65) % 2 << 7) | 1)
    rig.call("reset in every other environment", MARK_POS, honour=True)
    got = rig.tr.trail_lengths().cpu().tolist()
    assert got[0] == [1, 0, 1] and got[1] == [0, 1, 2]
    assert rig.tr.last_tprofile.cpu()[:2].tolist() == [[0, 0, 0, 0], [1, 1, 0, 1]]


def test_refused_environment_keeps_its_value():
    rig = Rig(3, 65)
    rig.planted({(0, 1)})
    rig.call("first", CLEAR | MARK_POS)
    rig.planted({(1, 2)})
    rig.write(err=np.arange(65) % 3 == 0, evcount=(np.arange(65) % 2 << 7))
    rig.call("refused in every third", MARK_POS, skip=True)
    assert rig.tr.longest_trail().cpu()[:3].tolist() == [1, 2, 2]
    rig.call("refused and reset", MARK_POS, honour=True, skip=True)  # env 3: refused AND reset -- the start layer alone
    got = rig.tr.trail_lengths().cpu().tolist()
    assert got[3] == [0, 1, 1] and got[1] == [0, 1, 2] and got[0] == [0, 1, 0]
    rig.call("without the flag the layer is entered", MARK_POS)
    assert rig.tr.trail_lengths().cpu()[0].tolist() == [0, 1, 2]


def test_ring_over_16_agents():
    """One state holds a -> a + 1 for all 16 agents: from every agent a trail of 15 arcs is open; bit 15 of a row, agent 15, bits
    60-63 of the value."""
    rig = Rig(16, 65)
    rig.planted({(a, (a + 1) % 16) for a in range(16)})
    rig.call("ring", CLEAR | MARK_POS)
    assert rig.tr.trail_lengths().cpu().tolist() == [[15] * 16] * 65 and int(rig.tr.episode_trails[0]) == -1
    rig.planted({(14, 15)})
    rig.call("one arc", CLEAR | MARK_POS)
    assert int(rig.tr.episode_trails[7]) == cooptrails_ref.pack([0] * 15 + [1])


def test_complete_digraph_on_4_agents_is_dense():
    """12 arcs allow far more than 4 096 extensions per starting agent: the dense mark is set, stays until CLEAR, and the fields are
    lower bounds of the exact ones (a closed trail over all 12 arcs ends at every agent)."""
    n = 65
    rig = Rig(4, n)
    full = {(h, b) for h in range(4) for b in range(4) if h != b}
    rows = np.zeros((n, 4), np.int64)
    rows[::2] = rows_of(full, 4)
    rig.write(rows=rows)
    rig.call("complete digraph", CLEAR | MARK_POS, compare=False)
    torch.cuda.synchronize(rig.dev)
    prof, lengths = rig.tr.episode_tprofile.cpu(), rig.tr.trail_lengths().cpu()
    assert prof[1::2].tolist() == [[0, 0, 0, 1]] * (n // 2) and prof[::2, 1:].tolist() == [[1, 1, 1]] * (n - n // 2)
    assert int(lengths[::2].min()) >= 4 and int(lengths[::2].max()) <= 12 and int(lengths[1::2].max()) == 0
    assert torch.equal(prof[:, 0], lengths.max(dim=1).values)
    assert rig.tr.trails_exact().cpu().tolist() == [bool(e % 2) for e in range(n)]
    before = lengths.clone()
    rig.write(rows=np.zeros((n, 4), np.int64))
    rig.call("sticky", FINISH | MARK_POS, compare=False)
    torch.cuda.synchronize(rig.dev)
    assert rig.tr.episode_tprofile.cpu()[::2, 2].tolist() == [1] * (n - n // 2) and rig.tr.last_tprofile.cpu()[::2, 2].tolist() == [1] * (n - n // 2)
    assert torch.equal(rig.tr.trail_lengths().cpu(), before) and torch.equal(rig.tr.trail_lengths(last=True).cpu(), before)
    rig.call("cleared", CLEAR, compare=False)
    torch.cuda.synchronize(rig.dev)
    assert rig.tr.episode_tprofile.cpu().tolist() == [[0, 0, 0, 1]] * n and bool(rig.tr.trails_exact().all())
    for lo, hi in rig.guards:
        assert int(lo.max()) == 0 and int(hi.max()) == 0


def test_mutual_and_interdependent_from_the_flattened_edges():
    """is_mutual / is_interdependent(2): torch over episode_edges / last_edges, against the restatement."""
    rng = np.random.default_rng(6)
    n, A = 65, 5
    rig = Rig(A, n)
    rows = random_rows(rng, n, A, stray=False)
    rows[3] = rows_of({(4, 0), (0, 4)}, A)
    rig.tr.episode_edges.copy_(torch.from_numpy(rows.astype(np.int32)).to(rig.dev))
    rig.tr.last_edges.copy_(torch.from_numpy(np.roll(rows, 1, axis=0).astype(np.int32)).to(rig.dev))
    want = [cooptrails_ref.is_mutual(edges_of(r)) for r in rows]
    assert rig.tr.is_mutual().cpu().tolist() == want and rig.tr.is_interdependent(2).cpu().tolist() == want and want[3] and not all(want)
    assert rig.tr.is_mutual(last=True).cpu().tolist() == want[-1:] + want[:-1]
    assert not bool(rig.tr.is_interdependent(1).any()) and not bool(rig.tr.is_interdependent(0).any())
    with pytest.raises(NotImplementedError):
        rig.tr.is_interdependent(3)


# ---------------------------------------------------------------------------------------------- capture, refusals
def test_one_update_in_a_captured_graph():
    """lle_cooptrails_update allocates nothing and never synchronises: one update captured into a graph, replayed over two states."""
    rig = Rig(5, 96)
    args = rig.tr.make_trails_args(MARK_POS)
    side = torch.cuda.Stream(device=rig.dev)
    side.wait_stream(torch.cuda.current_stream(rig.dev))
    with torch.cuda.stream(side):   # warm-up on the side stream: the kernel's code object is loaded outside the capture
        rig.tr.launch_trails(rig.tr.make_trails_args(CLEAR))
    side.synchronize()
    torch.cuda.current_stream(rig.dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rig.tr.launch_trails(args)   # (the current stream is the capturing one)
    for k, edges in enumerate(({(0, 1)}, {(1, 2), (2, 3)})):
        rig.planted(edges)
        graph.replay()
        torch.cuda.synchronize(rig.dev)
    assert rig.tr.trail_lengths().cpu().tolist() == [[0, 1, 2, 3, 0]] * 96


def test_refusals():
    from lle_amd.cooptrails import UpdateArgs
    rig = Rig(3, 64)
    L, h, st = rig.lib, rig.tr.th, rig.bw._stream()
    rig.planted({(0, 1)})
    rig.call("something to lose", CLEAR | MARK_POS)
    before = [v.cpu().clone() for v in rig.views]

    def refused(rc, text):
        assert rc in (LLE_ERR_NULL, LLE_ERR_ARG) and text in L.lle_cooptrails_last_error().decode(), (rc, L.lle_cooptrails_last_error())
    ok = UpdateArgs(C.sizeof(UpdateArgs), MARK_POS, 0, 0, None)
    refused(L.lle_cooptrails_update(h, None, st), "NULL")
    refused(L.lle_cooptrails_update(None, C.byref(ok), st), "NULL")
    refused(L.lle_cooptrails_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs) - 8, MARK_POS, 0, 0, None)), st), "struct_bytes")
    refused(L.lle_cooptrails_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs), 16, 0, 0, None)), st), "unknown operation or flag")
    refused(L.lle_cooptrails_update(h, C.byref(UpdateArgs(C.sizeof(UpdateArgs), MARK_POS, 4, 0, None)), st), "unknown operation or flag")
    refused(L.lle_cooptrails_update_map(h, 1, st), "map_index")
    refused(L.lle_cooptrails_update_map(h, -1, st), "map_index")
    assert L.lle_cooptrails_buffer(h, 4) is None and L.lle_cooptrails_buffer(h, -1) is None
    assert L.lle_cooptrails_create(None, rig.tr.h, st) is None and L.lle_cooptrails_create(rig.bw.h, None, st) is None
    torch.cuda.synchronize(rig.dev)
    for v, b in zip(rig.views, before):
        assert torch.equal(v.cpu(), b), "a refused call wrote"
    assert L.lle_cooptrails_update_map(h, 0, st) == 0
    rig.tr.update_map(0)  # (both handles, through the tracker)
    rig.call("the start edges are still there", CLEAR | MARK_STARTS)
    assert rig.tr.trail_lengths().cpu()[0].tolist() == [0, 1, 1]
