"""The shaping kernel (liblle_shaping.so, lle_amd/shaping/shaping.hip) over the parts of its domain that BatchedLLE rollouts do not
reach, against the array-level restatement tests/shaping_ref.py, bit for bit: reward_out, extras_out and both reached arrays are
compared with np.array_equal on their 32-bit patterns -- there is no tolerance in this file.

lle_shaping_update depends only on LLE_BUF_POS, LLE_BUF_EVCOUNT, the two reached arrays and the map tables.  BatchedWorld exposes the
first two as torch views and Shaping.reached the arrays: the tests write SYNTHETIC states into them (no step follows, so the engine's
invariants do not matter), call the C ABI once and compare everything the call may write.  Every output is a slice of a larger tensor
filled with a canary: the canary on both sides and the rows of environments that env_mask leaves out must be untouched after every
call (`Handle.call` checks it each time).  What a generator covers is asserted, not assumed."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from lle_amd import mapgen
from oracle.levels import LEVELS
from tests import instantiation_maps, shaping_ref
from tests.oracle_shaping import SHAPING_MAPS
from tests.parity_util import _grid
from tests.shaping_ref import CLEAR, HONOUR_AUTO_RESET, MARK_POS, MARK_STARTS, ShapingRef

pytestmark = pytest.mark.gpu

LLE_ERR_NULL, LLE_ERR_ARG, LLE_ERR_UNSUPPORTED = -1, -2, -4
CANARY = 0x5A5AA5A5   # (as float32: 1.5389e16, no value the kernel computes here)
PAD = 64              # canary elements on either side of an output; a multiple of 4, so that [n][4] bases stay 16-byte aligned
THREADS = 256         # SHAPING_THREADS
LDS_TABLE_MAX_BYTES = 16384
INTENDED = set()      # the kernels this file meant to reach (Handle.__init__), for the last test
AGENT_COUNTS = [1, 2, 3, 4, 5, 8, 9, 13, 16]
RAN_AGENT_COUNTS = set()

# kind 0: the bases the issue names; 1e-40 is a float32 denormal
BASES = np.array([0.0, -0.0, 1.0, -1.0, 3.0, 1e-40, 1e30, 16777216.0, np.inf, -np.inf], np.float32)


def group_of(n_agents):
    g = 1
    while g < n_agents:
        g *= 2
    return g


# ---------------------------------------------------------------------------------------------- the rig
class Batch:
    """A BatchedWorld of `texts` (map m owns block m) with host mirrors of what was last written into pos / evcount."""

    def __init__(self, oracle_mod, texts, n):
        from lle_amd import BatchedWorld
        self.texts = list(texts)
        self.bw = BatchedWorld(self.texts if len(self.texts) > 1 else self.texts[0], n)
        self.worlds = [oracle_mod.OracleWorld(t) for t in self.texts]
        w = self.worlds[0]
        self.n, self.per = int(n), int(n) // len(self.texts)
        self.A, self.L, self.H, self.W = w.n_agents, w.n_sources, w.height, w.width
        assert tuple(self.bw.pos.shape) == (self.n, self.A, 2) and self.bw.pos.dtype == torch.uint8
        assert tuple(self.bw.evcount.shape) == (self.n,) and self.bw.evcount.dtype == torch.uint8
        self.pos = self.bw.pos.cpu().numpy().copy()
        self.ev = self.bw.evcount.cpu().numpy().copy()

    def write(self, pos=None, evcount=None):
        dev = self.bw.device
        if pos is not None:
            self.pos = np.ascontiguousarray(pos, np.uint8).reshape(self.n, self.A, 2)
            self.bw.pos.copy_(torch.from_numpy(self.pos).to(dev))
        if evcount is not None:
            self.ev = np.ascontiguousarray(evcount, np.uint8).reshape(self.n)
            self.bw.evcount.copy_(torch.from_numpy(self.ev).to(dev))
        torch.cuda.synchronize(dev)


class Canaried:
    """`count` 32-bit elements between two runs of PAD canaries."""

    def __init__(self, count, dev):
        self.count = count
        self.full = torch.full((count + 2 * PAD,), CANARY, dtype=torch.int32, device=dev)
        self.out = self.full[PAD:PAD + count]
        assert self.out.data_ptr() % 16 == 0

    def host(self):
        full = self.full.cpu().numpy().view(np.uint32)
        assert (full[:PAD] == CANARY).all() and (full[PAD + self.count:] == CANARY).all(), "the call wrote outside its output"
        return full[PAD:PAD + self.count]


class Handle:
    """One lle_shaping on a Batch next to its ShapingRef."""

    def __init__(self, batch, pbrs_cols, extras_cols, gamma=0.9, reward_value=0.3):
        from lle_amd.shaping import Shaping
        self.b = batch
        self.sh = Shaping(batch.bw, pbrs_cols, extras_cols, gamma, reward_value)
        self.ref = ShapingRef(batch.worlds, batch.per, pbrs_cols, extras_cols, gamma, reward_value)
        self.views = [self.sh.reached(0), self.sh.reached(1)]
        for which, v in enumerate(self.views):
            assert v.dtype == torch.int32 and tuple(v.shape) == (batch.n, batch.A) and v.is_cuda and v.is_contiguous()
            assert v.data_ptr() == self.sh.reached_ptr(which), "Shaping.reached is a view of the handle's array, not a copy"
        self.E = len(extras_cols)
        g = group_of(batch.A)
        lds = batch.H * batch.W * 4 <= LDS_TABLE_MAX_BYTES and (len(batch.texts) == 1 or batch.per % (THREADS // g) == 0)
        self.kernel = f"shaping_kernel<{g},{'true' if lds else 'false'}>"
        INTENDED.add(self.kernel)

    def preset(self, words_s=None, words_e=None):
        for v, w in zip(self.views, (words_s, words_e)):
            if w is not None:
                w = np.ascontiguousarray(w, np.uint32).reshape(self.b.n, self.b.A)
                v.copy_(torch.from_numpy(w.view(np.int32)).to(v.device))
        torch.cuda.synchronize(self.b.bw.device)

    def read(self):
        return tuple(v.cpu().numpy().view(np.uint32).copy() for v in self.views)

    def device_args(self, s_ops, e_ops, flags, kind, mask, base, want_reward, want_extras):
        """(UpdateArgs, reward Canaried | None, extras Canaried | None, tensors to keep alive)."""
        dev, n = self.b.bw.device, self.b.n
        width_in, width_out = (1, 1) if kind == 0 else (4, 5)
        mask_t = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
        base_t = None
        if base is not None:
            base_t = torch.from_numpy(np.ascontiguousarray(base, np.float32).reshape(n, width_in).view(np.int32)).to(dev)
        reward = Canaried(n * width_out, dev) if want_reward else None
        extras = Canaried(n * self.b.A * self.E, dev) if want_extras else None
        args = self.sh.make_args(strategy_ops=s_ops, extras_ops=e_ops, flags=flags, reward_kind=kind, env_mask=mask_t, base_reward=base_t,
                                 reward_out=None if reward is None else reward.out, extras_out=None if extras is None else extras.out)
        return args, reward, extras, (mask_t, base_t)

    def expect(self, before, s_ops, e_ops, flags, kind, mask, base, want_reward):
        state = self.ref.from_words(*before)
        new, (reward, extras) = self.ref.update(state, self.b.pos, self.b.ev, s_ops, e_ops, flags, kind, mask, base if want_reward else None)
        return self.ref.to_words(new), reward, extras

    def compare(self, where, before, want, reward, extras, mask, kind):
        """The device after a call against `want` = (words, reward, extras) of the reference."""
        n, A = self.b.n, self.b.A
        want_words, want_r, want_e = want
        sel = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
        after = self.read()
        for k, name in enumerate(("strategy", "extras")):
            if not np.array_equal(after[k], want_words[k]):
                e, a = np.argwhere(after[k] != want_words[k])[0]
                raise AssertionError(f"{where}: the {name} array differs at env {e} agent {a}: {after[k][e, a]:#x} != {want_words[k][e, a]:#x} "
                                     f"(was {before[k][e, a]:#x}, pos {self.b.pos[e, a].tolist()}, evcount {self.b.ev[e]:#x}, selected {bool(sel[e])})")
        if reward is not None:
            got = reward.host().reshape(n, -1)
            want_bits = np.where(sel[:, None], want_r.view(np.uint32), np.uint32(CANARY))
            if not np.array_equal(got, want_bits):
                e = int(np.argwhere((got != want_bits).any(axis=1))[0][0])
                raise AssertionError(f"{where}: reward_out (kind {kind}) differs in env {e} (selected {bool(sel[e])}): {got[e].view(np.float32).tolist()} != "
                                     f"{want_bits[e].view(np.float32).tolist()}; counts {self.ref.last['before'][e]} -> {self.ref.last['after'][e]} of {self.ref.last['size']}")
        if extras is not None:
            got = extras.host().reshape(n, A * self.E)
            want_bits = np.where(sel[:, None], want_e.reshape(n, -1).view(np.uint32), np.uint32(CANARY))
            if not np.array_equal(got, want_bits):
                e = int(np.argwhere((got != want_bits).any(axis=1))[0][0])
                raise AssertionError(f"{where}: extras_out differs in env {e} (selected {bool(sel[e])}): {got[e].view(np.float32).tolist()} != "
                                     f"{want_bits[e].view(np.float32).tolist()}")

    def call(self, s_ops, e_ops, flags=0, kind=0, mask=None, base=None, want_reward=False, want_extras=False, where=""):
        """One lle_shaping_update on the state the device holds now, compared in full.  Returns the reference's bookkeeping."""
        before = self.read()
        args, reward, extras, keep = self.device_args(s_ops, e_ops, flags, kind, mask, base, want_reward, want_extras)
        want = self.expect(before, s_ops, e_ops, flags, kind, mask, base, want_reward)
        self.sh.update(args, self.b.bw._stream())
        torch.cuda.synchronize(self.b.bw.device)
        self.compare(f"{where} [{self.kernel} s_ops {s_ops} e_ops {e_ops} flags {flags}]", before, want, reward, extras, mask, kind)
        del keep
        return dict(self.ref.last) if want_reward else None

    def assert_launched(self):
        from lle_amd import shaping
        assert self.kernel in shaping.launched_kernels(), f"{self.kernel} was meant to run and did not"


# ---------------------------------------------------------------------------------------------- generators
def covering_positions(batch, shift, rng):
    """pos u8 [n, A, 2]: agent a of environment e < H * W stands on cell (e + shift * a) % (H * W) -- every cell of the map holds every agent
    once, walls, sources, cells under two and three beams included.  The environments from H * W on: all agents outside the grid at (255,
    255); one agent outside; just past the last row (H, 0); just past the last column (0, W); then random cells."""
    n, A, H, W = batch.n, batch.A, batch.H, batch.W
    HW = H * W
    assert n >= HW + 4
    cell = (np.arange(n)[:, None] + shift * np.arange(A)[None, :]) % HW
    cell[HW + 4:] = rng.integers(0, HW, (n - HW - 4, A))
    pos = np.stack([cell // W, cell % W], axis=2).astype(np.uint8)
    pos[HW] = 255
    pos[HW + 1, 0] = 255
    pos[HW + 2, :, 0], pos[HW + 2, :, 1] = H, 0
    pos[HW + 3, :, 0], pos[HW + 3, :, 1] = 0, W
    return pos


def assert_every_cell_holds_every_agent(batch, pos):
    for m in range(len(batch.texts)):
        block = pos[m * batch.per:(m + 1) * batch.per].astype(np.int64)
        for a in range(batch.A):
            inside = (block[:, a, 0] < batch.H) & (block[:, a, 1] < batch.W)
            seen = set((block[inside, a, 0] * batch.W + block[inside, a, 1]).tolist())
            assert seen == set(range(batch.H * batch.W)), f"map {m}, agent {a}: {batch.H * batch.W - len(seen)} cells never hold it"
    assert (pos == 255).all(axis=(1, 2)).any(), "no environment with every agent outside the grid"


def random_words(batch, rng):
    """u32 [n, A] over the sources of the map (bits from n_sources on stand for no source and are left clear); environments 0 / 1 / 2 of
    every 8: nothing, everything, the highest source alone."""
    full = (1 << batch.L) - 1
    w = (rng.integers(0, 1 << 32, (batch.n, batch.A), dtype=np.uint64) & rng.integers(0, 1 << 32, (batch.n, batch.A), dtype=np.uint64)) & full
    w[0::8] = 0
    w[1::8] = full
    if batch.L:
        w[2::8] = 1 << (batch.L - 1)
    return w.astype(np.uint32)


def random_evcount(batch, rng):
    """Random low bits, random bit 7."""
    return (rng.integers(0, 128, batch.n) | (rng.integers(0, 2, batch.n) << 7)).astype(np.uint8)


def random_base(batch, kind, rng):
    """kind 0: drawn from BASES; kind 1: arbitrary non-NaN bit patterns [n, 4]."""
    if kind == 0:
        return BASES[rng.integers(0, len(BASES), batch.n)]
    bits = rng.integers(0, 1 << 32, (batch.n, 4), dtype=np.uint64).astype(np.uint32)
    nan = ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0)
    bits[nan] &= 0xFF800000   # the infinity of the same sign
    out = bits.view(np.float32)
    assert not np.isnan(out).any()
    return out


MASK_KINDS = ("none", "random", "all-zero")


def make_mask(kind, batch, rng):
    if kind == "none":
        return None
    if kind == "all-zero":
        return np.zeros(batch.n, np.uint8)
    m = (rng.random(batch.n) < 0.5) * rng.integers(1, 256, batch.n)   # any non-zero byte selects
    return m.astype(np.uint8)


# ---------------------------------------------------------------------------------------------- every operation pair
HANDLE_KINDS = ("both", "pbrs", "extras", "neither")
OP_MAPS = {"level6": (LEVELS[6], 197), "start_on_beam": (SHAPING_MAPS["start_on_beam"], 150), "three_beam_cell": (SHAPING_MAPS["three_beam_cell"], 131)}


def op_sample(seed):
    """The full product (strategy_ops, extras_ops) x flag x mask kind x reward kind = 64 * 2 * 3 * 2 = 768 calls in a seeded order.  The four
    calls of a pair under a random mask are laid down -- every output on a handle that has the array it reads --; the others get a seeded
    handle kind and a seeded subset of the outputs the handle can give (extras_out needs extras columns)."""
    rng = np.random.default_rng(seed)
    fixed = {(0, 0): ("both", True, True), (0, 1): ("pbrs", True, False), (1, 0): ("extras", True, True), (1, 1): ("both", True, True)}
    calls = []
    for s_ops, e_ops, flags, mask, kind in itertools.product(range(8), range(8), (0, HONOUR_AUTO_RESET), MASK_KINDS, (0, 1)):
        if mask == "random":
            handle, want_reward, want_extras = fixed[(flags, kind)]
        else:
            handle = HANDLE_KINDS[int(rng.integers(0, 4))]
            want_reward, want_extras = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)) and handle in ("both", "extras")
        calls.append(dict(s_ops=s_ops, e_ops=e_ops, flags=flags, mask=mask, kind=kind, handle=handle, want_reward=want_reward, want_extras=want_extras))
    order = rng.permutation(len(calls))
    return [calls[k] for k in order]


def assert_sample_coverage(calls):
    assert len(calls) >= 600
    seen = {(c["s_ops"], c["e_ops"], c["flags"], c["mask"], c["kind"]) for c in calls}
    assert seen == set(itertools.product(range(8), range(8), (0, 1), MASK_KINDS, (0, 1)))
    assert {(c["s_ops"], c["e_ops"]) for c in calls} == set(itertools.product(range(8), range(8)))
    assert {c["flags"] for c in calls} == {0, 1} and {c["mask"] for c in calls} == set(MASK_KINDS) and {c["kind"] for c in calls} == {0, 1}
    for handle in HANDLE_KINDS:
        subsets = {(c["want_reward"], c["want_extras"]) for c in calls if c["handle"] == handle}
        want = set(itertools.product((False, True), (False, True))) if handle in ("both", "extras") else {(False, False), (True, False)}
        assert subsets == want, (handle, subsets)
        # every pair of operations meets every output at least once on the handles that have the array the output reads
    for s_ops, e_ops in itertools.product(range(8), range(8)):   # every pair meets every output and both kinds under a random mask
        mine = [c for c in calls if (c["s_ops"], c["e_ops"]) == (s_ops, e_ops) and c["mask"] == "random"]
        assert {c["kind"] for c in mine if c["want_reward"] and c["handle"] in ("both", "pbrs")} == {0, 1}, (s_ops, e_ops)
        assert {c["flags"] for c in mine if c["want_extras"]} == {0, 1}, (s_ops, e_ops)


@pytest.mark.parametrize("name", sorted(OP_MAPS))
def test_every_operation_pair(oracle_mod, name):
    """All 64 (strategy_ops, extras_ops) x LLE_SHAPING_HONOUR_AUTO_RESET off / on x env_mask none / random / all-zero x reward_kind 0 / 1
    (768 calls), on handles with pbrs_cols and extras_cols, with one of them, and with neither (the shaped term is then 0 and reward_out is
    still written), each call from fresh random reached words, random evcount bytes and one of three position arrays in which every cell of
    the map holds every agent.  n is not a multiple of 256 / G."""
    text, n = OP_MAPS[name]
    batch = Batch(oracle_mod, [text], n)
    assert n % (THREADS // group_of(batch.A)) != 0 and n > THREADS // group_of(batch.A)
    every = list(range(batch.L))
    some = [batch.L - 1, 0, batch.L - 1]   # a duplicate, a source left out (there are at least two, one is left out when there are three)
    handles = {"both": Handle(batch, some, every[::-1]), "pbrs": Handle(batch, every, []), "extras": Handle(batch, [], some[:2]),
               "neither": Handle(batch, [], [])}
    calls = op_sample(31 + len(name))
    assert_sample_coverage(calls)
    rng = np.random.default_rng(len(name))
    positions = [covering_positions(batch, shift, rng) for shift in (1, 7, 11)]
    for p in positions:
        assert_every_cell_holds_every_agent(batch, p)
    for k, c in enumerate(calls):
        batch.write(pos=positions[k % 3], evcount=random_evcount(batch, rng))
        h = handles[c["handle"]]
        h.preset(random_words(batch, rng), random_words(batch, rng))
        h.call(c["s_ops"], c["e_ops"], c["flags"], c["kind"], make_mask(c["mask"], batch, rng), random_base(batch, c["kind"], rng),
               c["want_reward"], c["want_extras"], where=f"{name} call {k} on `{c['handle']}`")
    for h in handles.values():
        h.assert_launched()


# ---------------------------------------------------------------------------------------------- wide masks, group shapes
def wide_lists(n_sources, rng):
    """pbrs_cols of 64 entries over 32 sources: the HIGHEST source 8 times, others 7, 6, 5, 4, 3, 3 and 2 (six of them) times, sixteen once, three
    not at all; extras_cols of 64 entries with repeats, shuffled, some sources missing."""
    assert n_sources == 32
    ids = [int(v) for v in rng.permutation(31)]          # the sources below the highest, in a seeded order
    times = [7, 6, 5, 4, 3, 3] + [2] * 6 + [1] * 16
    pbrs = [31] * 8
    for l, t in zip(ids, times):
        pbrs += [l] * t
    unlisted = ids[len(times):]
    assert len(pbrs) == 64 and len(unlisted) == 3
    pbrs = [pbrs[k] for k in rng.permutation(64)]
    extras = [31, 31, 0] + [int(v) for v in rng.integers(0, 32, 61)]
    extras = [extras[k] for k in rng.permutation(64)]
    assert len(set(extras)) < 32 and max(extras.count(l) for l in set(extras)) > 1
    return pbrs, extras, unlisted


def wide_words(batch, unlisted, rng):
    """Preset words of a 32-source map: per 8 environments nothing, everything, bit 31 alone (random_words), then the unlisted sources
    alone, then random words."""
    w = random_words(batch, rng)
    w[3::8] = sum(1 << l for l in unlisted)
    return w


def drive_wide(h, batch, unlisted, rng, where):
    """A dozen calls that cover the marks, the clears, the flag, masks and both kinds on a handle with 64 + 64 columns."""
    seen_before, seen_after, words_seen = set(), set(), set()
    plan = [(MARK_POS, MARK_POS, 0, 0, "none"), (MARK_POS, MARK_POS, 0, 1, "none"), (CLEAR | MARK_POS, CLEAR | MARK_POS, 0, 0, "none"),
            (MARK_STARTS | MARK_POS, MARK_POS, HONOUR_AUTO_RESET, 1, "random"), (0, MARK_POS, 0, 0, "none"), (MARK_POS, 0, HONOUR_AUTO_RESET, 0, "random"),
            (CLEAR | MARK_STARTS, CLEAR | MARK_STARTS, 0, 1, "none"), (MARK_STARTS, CLEAR, 0, 0, "random"), (0, 0, 0, 0, "none"),
            (CLEAR, MARK_STARTS | MARK_POS, HONOUR_AUTO_RESET, 1, "none")]
    for k, (s_ops, e_ops, flags, kind, mask) in enumerate(plan):
        batch.write(evcount=random_evcount(batch, rng))
        ws = wide_words(batch, unlisted, rng)
        h.preset(ws, wide_words(batch, unlisted, rng))
        last = h.call(s_ops, e_ops, flags, kind, make_mask(mask, batch, rng), random_base(batch, kind, rng), True, True, where=f"{where} call {k}")
        seen_before |= set(last["before"].tolist())
        seen_after |= set(last["after"].tolist())
        words_seen |= set(h.read()[0].reshape(-1).tolist())
        if s_ops == MARK_POS and flags == 0 and mask == "none":
            only_unlisted = (ws == sum(1 << l for l in unlisted)).all(axis=1)
            assert only_unlisted.any() and (last["before"][only_unlisted] == 0).all(), "bits of unlisted sources must not count"
    return seen_before, seen_after, words_seen


@pytest.mark.parametrize("n_agents", AGENT_COUNTS)
def test_group_shapes_and_wide_masks(oracle_mod, n_agents):
    """Lane groups with idle lanes and full ones (A = 1 .. 16) on a 32-source map with crossing beams, 64 pbrs_cols (one source eight times,
    others fewer, three not at all) and 64 shuffled extras_cols with repeats: source ids up to 31, both packed 16-bit counts from 0 to
    A * 64 (1 024 with 16 agents), the cross-lane sum over every group size.  One map per batch (cell table in LDS, ragged last
    workgroup) and two maps at 41 environments each (global memory)."""
    rng = np.random.default_rng(100 + n_agents)
    text = instantiation_maps.build(n_agents, 32, crossing=True, seed=5)
    pbrs, extras, unlisted = wide_lists(32, rng)
    batch = Batch(oracle_mod, [text], 300)
    assert batch.L == 32 and batch.n % (THREADS // group_of(n_agents)) != 0
    h = Handle(batch, pbrs, extras)
    crossing = (h.ref.cells[0].sum(axis=0) >= 2)
    assert crossing.any(), "no cell under two beams"
    pos = covering_positions(batch, 5, rng)
    assert_every_cell_holds_every_agent(batch, pos)
    batch.write(pos=pos)
    before, after, words = drive_wide(h, batch, unlisted, rng, f"A={n_agents}")
    size = n_agents * 64
    assert {0, size} <= before and {0, size} <= after, f"the counts never reach 0 and {size} on both sides of the mark"
    assert {0, 0xFFFFFFFF, 0x80000000} <= words, "bit 31 alone, all 32 bits and no bit must occur in the strategy array after a call"
    # bit 31 reached ALONE by a mark: a handle that lists only source 31, cleared, every agent over the whole map
    alone = Handle(batch, [31], [31, 0], gamma=0.99, reward_value=0.5)
    alone.preset(random_words(batch, rng), random_words(batch, rng))
    alone.call(CLEAR | MARK_POS, CLEAR | MARK_POS, 0, 0, None, random_base(batch, 0, rng), True, True, where=f"A={n_agents} source 31")
    ws, _ = alone.read()
    on31 = h.ref.cells[0][31] & (h.ref.cells[0].sum(axis=0) == 1)
    assert on31.any() and (ws == 0x80000000).sum() >= on31.sum() * n_agents
    h.assert_launched()
    # two maps (the same beams, other starts), 41 environments each: a workgroup spans both, the table stays in global memory
    two = Batch(oracle_mod, [text, instantiation_maps.build(n_agents, 32, crossing=True, seed=5, variant=1)], 82)
    g = Handle(two, pbrs, extras)
    assert g.kernel.endswith("false>") and h.kernel.endswith("true>")
    cells = rng.integers(0, two.H * two.W, (two.n, two.A))
    two.write(pos=np.stack([cells // two.W, cells % two.W], axis=2))
    drive_wide(g, two, unlisted, rng, f"A={n_agents} two maps")
    g.assert_launched()
    RAN_AGENT_COUNTS.add(n_agents)


# ---------------------------------------------------------------------------------------------- table placement
def edge_map(h, w):
    """Two agents; beams down the LAST COLUMN (source 0 at (0, w - 1)) and along the LAST ROW (the source at (h - 1, 0)), which cross in
    the last cell; two more beams inside."""
    return _grid(h, w, {(0, w - 1): "L0S", (h - 1, 0): "L1E", (1, 1): "S0", (1, 3): "S1", (3, 1): "X", (3, 3): "X", (5, 0): "L0E", (7, w - 2): "L1N"})


@pytest.mark.parametrize("h,w,lds", [(64, 64, True), (64, 65, False), (65, 64, False), (17, 255, False)], ids=["64x64", "64x65", "65x64", "17x255"])
def test_table_placement(oracle_mod, h, w, lds):
    """The cell table in LDS at exactly 16 KiB (64 x 64) and in global memory just past it (64 x 65, 65 x 64) and with W = 255 (17 x 255),
    one map per batch; beam tiles in the last row and the last column, whose last cell lies under two beams."""
    rng = np.random.default_rng(h * w)
    batch = Batch(oracle_mod, [edge_map(h, w)], 150)
    hd = Handle(batch, [3, 0, 3], [0, 1, 2, 3])
    assert hd.kernel == f"shaping_kernel<2,{'true' if lds else 'false'}>" and (h * w * 4 <= LDS_TABLE_MAX_BYTES) == lds
    table = hd.ref.cells[0]
    assert table[:, h - 1, :].any(axis=0).sum() >= w - 1 and table[:, :, w - 1].any(axis=0).sum() >= h - 1 and table[:, h - 1, w - 1].sum() == 2
    beam_cells = np.argwhere(table.any(axis=0))
    pos = np.zeros((batch.n, 2, 2), np.uint8)
    pick = beam_cells[rng.integers(0, len(beam_cells), (batch.n, 2))]
    anywhere = np.stack([rng.integers(0, h, (batch.n, 2)), rng.integers(0, w, (batch.n, 2))], axis=2)
    pos[:] = np.where((rng.random((batch.n, 2)) < 0.6)[..., None], pick, anywhere)
    pos[0] = (h - 1, w - 1)                 # the last cell of the table
    pos[1] = [(h - 1, 1), (1, w - 1)]       # the last row, the last column
    pos[2] = [(0, 0), (h - 1, w - 2)]
    pos[3] = [(h, 0), (0, w)]               # just outside
    pos[4] = 255
    last_row = (pos[..., 0] == h - 1).sum()
    last_col = (pos[..., 1] == w - 1).sum()
    assert last_row >= 3 and last_col >= 3
    batch.write(pos=pos)
    for k, (s_ops, e_ops, flags, kind, mask) in enumerate([(CLEAR | MARK_POS, CLEAR | MARK_POS, 0, 0, "none"), (MARK_POS, MARK_POS, 0, 1, "random"),
                                                            (MARK_STARTS | MARK_POS, MARK_POS, HONOUR_AUTO_RESET, 0, "random")]):
        batch.write(evcount=random_evcount(batch, rng))
        hd.preset(random_words(batch, rng), random_words(batch, rng))
        last = hd.call(s_ops, e_ops, flags, kind, make_mask(mask, batch, rng), random_base(batch, kind, rng), True, True, where=f"{h}x{w} call {k}")
        if k == 0:
            assert last["after"][0] == 2 * 3 and last["after"][4] == 0   # both agents in the crossing of the last cell: 2 x (3 twice + 0)
    hd.assert_launched()


MULTI_MAPS = [mapgen.generate(seed=100 + s, height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2) for s in range(4)]


@pytest.mark.parametrize("per,lds", [(64, True), (128, True), (37, False)], ids=["64-per-map-lds", "128-per-map-lds", "37-per-map-global"])
def test_four_maps_each_block_reads_its_own_table(oracle_mod, per, lds):
    """Four maps with different beams: with envs_per_map a multiple of 256 / G every workgroup loads the table of ITS block into LDS (128:
    two workgroups per map), with 37 a workgroup spans two maps and reads global memory.  Every agent of block m stands on a cell whose
    set of sources in map m differs from the one in map m - 1 and in map m + 1."""
    rng = np.random.default_rng(per)
    batch = Batch(oracle_mod, MULTI_MAPS, 4 * per)
    hd = Handle(batch, [0, 1, 2, 3, 1], [3, 2, 1, 0])
    assert hd.kernel == f"shaping_kernel<4,{'true' if lds else 'false'}>"
    tables = hd.ref.cells   # [map][source][H, W]
    pos = np.zeros((batch.n, batch.A, 2), np.uint8)
    for m in range(4):
        differs = np.ones((batch.H, batch.W), bool)
        for other in (m - 1, m + 1):
            if 0 <= other < 4:
                differs &= (tables[m] != tables[other]).any(axis=0)
        cells = np.argwhere(differs & tables[m].any(axis=0))   # ... and that lies under a beam of map m
        assert len(cells) >= 1, f"map {m}: no cell tells it from its neighbours"
        pos[m * per:(m + 1) * per] = cells[rng.integers(0, len(cells), (per, batch.A))]
    batch.write(pos=pos)
    for k, (s_ops, e_ops, flags, kind, mask) in enumerate([(CLEAR | MARK_POS, CLEAR | MARK_POS, 0, 1, "none"), (CLEAR | MARK_STARTS, MARK_STARTS, 0, 0, "none"),
                                                            (MARK_POS, MARK_POS, HONOUR_AUTO_RESET, 0, "random")]):
        batch.write(evcount=random_evcount(batch, rng))
        hd.preset(random_words(batch, rng), random_words(batch, rng))
        hd.call(s_ops, e_ops, flags, kind, make_mask(mask, batch, rng), random_base(batch, kind, rng), True, True, where=f"four maps x {per} call {k}")
    hd.assert_launched()


# ---------------------------------------------------------------------------------------------- arithmetic
PARAMS = [(0.9, 0.3), (0.7, 0.7), (0.99, 0.5), (0.95, 0.1)]


def cell_options(ref, weights):
    """{gain: (i, j)} over the cells of map 0: the entries one agent gains by standing there with nothing reached = the sum of the weights
    (times listed) of the sources of the cell.  Gain 0: a cell without a listed source."""
    table = ref.cells[0]
    options = {}
    for i in range(ref.H):
        for j in range(ref.W):
            gain = sum(weights.get(l, 0) for l in range(ref.L) if table[l, i, j])
            options.setdefault(gain, (i, j))
    return options


def split_gain(need, n_agents, gains):
    """`need` entries as the gains of n_agents agents, greedily the largest first (gains: descending, 0 among them); None when it does not
    come out even."""
    out = []
    for _ in range(n_agents):
        g = next(g for g in gains if g <= need)
        need -= g
        out.append(g)
    return out if need == 0 else None


def construct_counts(ref, pairs, rng):
    """Words and positions of len(pairs) environments such that environment e has exactly pairs[e][0] listed entries reached before a
    MARK_POS and pairs[e][1] after it.  Agents gain through the cell they stand on (a subset-sum over the agents' options); the preset
    entries avoid what the marks will reach."""
    weights = {l: ref.pbrs_cols.count(l) for l in set(ref.pbrs_cols)}
    options = cell_options(ref, weights)
    gains = sorted(options, reverse=True)
    A, table = ref.A, ref.cells[0]
    words = np.zeros((len(pairs), A), np.uint32)
    pos = np.zeros((len(pairs), A, 2), np.uint8)
    unlisted = [l for l in range(ref.L) if l not in weights]
    for e, (before, after) in enumerate(pairs):
        split, marked = split_gain(after - before, A, gains), set()
        assert split is not None, f"{after - before} entries cannot be gained by {A} agents in one mark"
        for a, g in enumerate(split):
            i, j = options[g]
            pos[e, a] = (i, j)
            marked |= {(a, l) for l in range(ref.L) if table[l, i, j] and l in weights}
        free = [(a, l) for a in range(A) for l in weights if (a, l) not in marked]
        order = rng.permutation(len(free))
        free = sorted((free[k] for k in order), key=lambda al: -weights[al[1]])
        need = before
        for a, l in free:
            if weights[l] <= need:
                need -= weights[l]
                words[e, a] |= np.uint32(1 << l)
        assert need == 0, f"no preset with exactly {before} entries"
        for a in range(A):   # bits of unlisted sources: they must not count
            for l in unlisted:
                if rng.random() < 0.3:
                    words[e, a] |= np.uint32(1 << l)
    return words, pos


def arithmetic_columns(ref_cells, size, n_agents, n_sources):
    """pbrs_cols of size / n_agents entries with the heavy sources on crossing beams (the two sources of a crossing cell are gained at once)
    and enough sources listed once that every count can be preset."""
    n_cols = size // n_agents
    both = np.argwhere(ref_cells.sum(axis=0) == 2)
    i, j = both[0]
    pair = [int(l) for l in np.nonzero(ref_cells[:, i, j])[0]]
    others = [l for l in range(n_sources) if l not in pair]
    if n_cols == 3:
        return pair + others[:1]
    if n_cols == 8:
        return [pair[0]] * 4 + [pair[1]] * 2 + others[:2]
    assert n_cols == 64
    cols = [pair[0]] * 8 + [pair[1]] * 8
    for l, t in zip(others, [8, 7, 6, 5, 4, 3, 2] + [1] * 13):
        cols += [l] * t
    assert len(cols) == 64
    return cols


def test_products_round_before_the_subtraction(oracle_mod):
    """`gamma * prev - cur` with the product rounded first: every (count before, count after) that tells the documented arithmetic from a
    fused multiply-add after the cast to float32 (shaping_ref.fma_sensitive, exact rationals), for four (gamma, reward_value) at 12, 128
    and 1 024 entries, constructed directly -- `before` entries preset, agents placed so that exactly `after - before` more are marked.  One
    MARK_POS gains at most two sources per agent (16 entries with both listed eight times), so of the pairs at 1 024 entries those further
    apart than the agents can gain in one call cannot occur in any call and are left out; every other pair runs."""
    rng = np.random.default_rng(12)
    batches = {}
    ran, ran_per_param = 0, {p: 0 for p in PARAMS}
    for size, n_agents in ((12, 4), (128, 16), (1024, 16)):
        probe = oracle_mod.OracleWorld(instantiation_maps.build(n_agents, 32, crossing=True, seed=5))
        cells = ShapingRef([probe], 1, [], [], 1.0, 1.0).cells[0]
        cols = arithmetic_columns(cells, size, n_agents, 32)
        weights = {l: cols.count(l) for l in set(cols)}
        for gamma, value in PARAMS:
            pairs = shaping_ref.fma_sensitive_pairs(gamma, value, size)
            if not pairs:
                continue
            if n_agents not in batches:
                batches[n_agents] = Batch(oracle_mod, [probe.map_str], 150)
            batch = batches[n_agents]
            h = Handle(batch, cols, [], gamma, value)
            assert h.ref.A * len(cols) == size
            gains = sorted(cell_options(h.ref, weights), reverse=True)
            assert gains[0] == cols.count(cols[0]) + max(cols.count(c) for c in cols if c != cols[0]) and {0, 1} <= set(gains)   # the heaviest two share a cell
            reachable = [p for p in pairs if split_gain(p[1] - p[0], n_agents, gains) is not None]
            if size < 1024:   # only at 1 024 entries are there pairs further apart than 16 agents x 2 sources x 8 repeats
                assert reachable == pairs
            assert reachable, f"no sensitive pair of gamma {gamma}, value {value}, {size} entries can be constructed"
            assert len(reachable) <= batch.n
            # the environments after the sensitive ones: random pairs within reach
            filler = [(b, min(size, b + int(rng.integers(0, n_agents + 1)))) for b in rng.integers(0, size + 1, batch.n - len(reachable))]
            words, pos = construct_counts(h.ref, reachable + [(int(b), int(a)) for b, a in filler], rng)
            batch.write(pos=pos, evcount=random_evcount(batch, rng))
            for kind in (0, 1):
                h.preset(words, random_words(batch, rng))
                base = np.zeros(batch.n, np.float32) if kind == 0 else random_base(batch, 1, rng)
                last = h.call(MARK_POS, 0, 0, kind, None, base, True, False, where=f"gamma {gamma} value {value} size {size} kind {kind}")
                got = list(zip(last["before"].tolist(), last["after"].tolist()))
                assert got[:len(reachable)] == reachable and len(got) == batch.n, "the constructed counts are not the intended ones"
            for e, (b, a) in enumerate(reachable):
                documented, fused = shaping_ref.shaped_terms(gamma, value, size, b, a)
                assert documented != fused and float(np.float32(last["p"][e])) == float(documented)
            ran += len(reachable)
            ran_per_param[(gamma, value)] += len(reachable)
    assert all(v > 0 for v in ran_per_param.values()), ran_per_param
    assert ran >= 30, ran


def test_kind0_adds_in_float32(oracle_mod):
    """reward_kind 0 is base + float(p) added in float32, not float(base + p): bases from {+-0, +-1, 3, 1e-40 (denormal), 1e30, 2^24, +-inf}
    against random counts; at least 100 cases in which the two differ must occur (counted with exact rationals)."""
    rng = np.random.default_rng(13)
    batch = Batch(oracle_mod, [LEVELS[6]], 197)
    sensitive = 0
    seen_bases = set()
    for gamma, value in PARAMS:
        h = Handle(batch, [0, 1, 2, 2], [], gamma, value)
        for k in range(3):
            cells = rng.integers(0, batch.H * batch.W, (batch.n, batch.A))
            batch.write(pos=np.stack([cells // batch.W, cells % batch.W], axis=2), evcount=random_evcount(batch, rng))
            h.preset(random_words(batch, rng), None)
            base = random_base(batch, 0, rng)
            last = h.call(MARK_POS, 0, 0, 0, None, base, True, False, where=f"gamma {gamma} value {value} round {k}")
            sensitive += sum(shaping_ref.double_rounding_sensitive(b, p) for b, p in zip(base, last["p"]))
            seen_bases |= set(base.view(np.uint32).tolist())
    assert seen_bases == set(BASES.view(np.uint32).tolist())
    assert sensitive >= 100, sensitive


# ---------------------------------------------------------------------------------------------- masked and repeated calls
def test_repeated_calls_and_two_handles(oracle_mod):
    """The same MARK_POS call twice: the second leaves the arrays alone and rewards gamma * cur - cur.  Two handles with different columns
    on one batch do not disturb each other, and freeing one leaves the other working."""
    rng = np.random.default_rng(14)
    batch = Batch(oracle_mod, [LEVELS[6]], 197)
    pos = covering_positions(batch, 3, rng)
    batch.write(pos=pos, evcount=random_evcount(batch, rng))
    h1, h2 = Handle(batch, [0, 1, 2], [2, 1], 0.9, 0.3), Handle(batch, [2, 2], [0], 0.7, 0.7)
    for h in (h1, h2):
        h.preset(random_words(batch, rng), random_words(batch, rng))
    kept = h2.read()
    base = np.zeros(batch.n, np.float32)
    h1.call(MARK_POS, MARK_POS, 0, 0, None, base, True, True, where="first")
    once = h1.read()
    last = h1.call(MARK_POS, MARK_POS, 0, 0, None, base, True, True, where="second")
    twice = h1.read()
    assert np.array_equal(once[0], twice[0]) and np.array_equal(once[1], twice[1]), "MARK_POS is idempotent on the arrays"
    assert np.array_equal(last["before"], last["after"])
    cur = (last["size"] - last["after"]).astype(np.float64) * 0.3
    assert np.array_equal(last["p"], 0.9 * cur - cur) and (last["p"] != 0).any()
    assert all(np.array_equal(a, b) for a, b in zip(kept, h2.read())), "a call on one handle changed the other handle's arrays"
    h2.call(CLEAR | MARK_POS, MARK_STARTS, 0, 1, make_mask("random", batch, rng), random_base(batch, 1, rng), True, True, where="the other handle")
    assert all(np.array_equal(a, b) for a, b in zip(twice, h1.read()))
    h1.views = None
    h1.sh.free()
    h2.preset(random_words(batch, rng), random_words(batch, rng))
    h2.call(MARK_POS, MARK_POS, HONOUR_AUTO_RESET, 0, None, random_base(batch, 0, rng), True, True, where="after freeing the first handle")


# ---------------------------------------------------------------------------------------------- stream capture
def test_update_inside_a_stream_capture(oracle_mod):
    """The header promises that lle_shaping_update is safe inside a stream capture: exactly one update (CLEAR | MARK_POS on both arrays,
    both outputs) is captured into a graph -- a single kernel node, no parallel branch --, replayed once, and once more after `pos` was
    rewritten.  Both replays equal the reference on the positions live at replay time."""
    rng = np.random.default_rng(15)
    batch = Batch(oracle_mod, [LEVELS[6]], 197)
    h = Handle(batch, [2, 0, 2], [0, 1, 2])
    ops = CLEAR | MARK_POS
    batch.write(pos=covering_positions(batch, 1, rng), evcount=random_evcount(batch, rng))
    base = random_base(batch, 0, rng)
    args, reward, extras, keep = h.device_args(ops, ops, 0, 0, None, base, True, True)
    side = torch.cuda.Stream(device=batch.bw.device)
    side.wait_stream(torch.cuda.current_stream(batch.bw.device))
    with torch.cuda.stream(side):   # warm-up on the side stream: the kernel's code object is loaded outside the capture
        h.sh.update(args, batch.bw._stream())
    side.synchronize()
    torch.cuda.current_stream(batch.bw.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        h.sh.update(args, batch.bw._stream())   # (the current stream is the capturing one)
    for k, shift in enumerate((7, 11)):
        batch.write(pos=covering_positions(batch, shift, rng))
        before = (random_words(batch, rng), random_words(batch, rng))
        h.preset(*before)
        reward.full.fill_(CANARY)
        extras.full.fill_(CANARY)
        want = h.expect(before, ops, ops, 0, 0, None, base, True)
        graph.replay()
        torch.cuda.synchronize(batch.bw.device)
        h.compare(f"replay {k}", before, want, reward, extras, None, 0)
    del keep


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_abi(oracle_mod):
    """The documented LLE_ERR_* paths of lle_shaping_create / lle_shaping_update / lle_shaping_reached: the status (NULL from create) and a
    non-empty lle_shaping_last_error; after every refused update the arrays and the canary-filled outputs are unchanged."""
    from lle_amd import shaping
    from lle_amd.shaping import ShapingConfig, UpdateArgs
    L = shaping.lib()
    rng = np.random.default_rng(16)
    batch = Batch(oracle_mod, [LEVELS[6]], 70)
    bw = batch.bw
    st = bw._stream()
    maps = (C.c_void_p * 1)(bw.map.h)
    two_maps = (C.c_void_p * 2)(bw.map.h, bw.map.h)

    def config(pbrs, extras, struct_bytes=None, n_pbrs=None, n_extras=None, null_pbrs=False, null_extras=False):
        pc = (C.c_int32 * max(len(pbrs), 1))(*pbrs)
        ec = (C.c_int32 * max(len(extras), 1))(*extras)
        cfg = ShapingConfig(C.sizeof(ShapingConfig) if struct_bytes is None else struct_bytes, len(pbrs) if n_pbrs is None else n_pbrs,
                            None if null_pbrs else pc, len(extras) if n_extras is None else n_extras, 0, None if null_extras else ec, 0.9, 0.3)
        cfg._keep = (pc, ec)
        return cfg

    def refused_create(why, batch_h, maps_p, n_maps, cfg, needle=None):
        got = L.lle_shaping_create(batch_h, maps_p, n_maps, None if cfg is None else C.byref(cfg), st)
        if got:
            L.lle_shaping_free(got)
            raise AssertionError(f"lle_shaping_create accepted {why}")
        msg = L.lle_shaping_last_error().decode()
        assert msg and (needle is None or needle in msg), f"{why}: message `{msg}`"

    good = config([0, 1], [2])
    refused_create("a NULL batch", None, maps, 1, good, "NULL")
    refused_create("NULL maps", bw.h, None, 1, good, "NULL")
    refused_create("a NULL config", bw.h, maps, 1, None, "NULL")
    refused_create("a NULL map in the list", bw.h, (C.c_void_p * 1)(None), 1, good, "NULL map")
    refused_create("a wrong struct_bytes", bw.h, maps, 1, config([0], [0], struct_bytes=C.sizeof(ShapingConfig) - 8), "struct_bytes")
    refused_create("n_maps 2 on a batch of one map", bw.h, two_maps, 2, good, "n_maps")
    refused_create("n_maps 0", bw.h, maps, 0, good, "n_maps")
    refused_create("65 pbrs_cols", bw.h, maps, 1, config([0, 1, 2] * 21 + [0, 1], []), "LLE_SHAPING_MAX_COLS")
    refused_create("65 extras_cols", bw.h, maps, 1, config([], [0] * 65), "LLE_SHAPING_MAX_COLS")
    refused_create("a negative pbrs count", bw.h, maps, 1, config([0], [0], n_pbrs=-1), "LLE_SHAPING_MAX_COLS")
    refused_create("a negative extras count", bw.h, maps, 1, config([0], [0], n_extras=-1), "LLE_SHAPING_MAX_COLS")
    refused_create("pbrs id -1", bw.h, maps, 1, config([0, -1], []), "pbrs_cols: not a laser_id")
    refused_create("pbrs id n_sources", bw.h, maps, 1, config([batch.L], []), "pbrs_cols: not a laser_id")
    refused_create("extras id -1", bw.h, maps, 1, config([], [-1]), "extras_cols: not a laser_id")
    refused_create("extras id n_sources", bw.h, maps, 1, config([], [0, batch.L]), "extras_cols: not a laser_id")
    refused_create("a source listed 9 times", bw.h, maps, 1, config([1] * 9, []), "LLE_SHAPING_MAX_REPEATS")
    refused_create("NULL pbrs_cols with a positive count", bw.h, maps, 1, config([0], [], null_pbrs=True))
    refused_create("NULL extras_cols with a positive count", bw.h, maps, 1, config([], [0], null_extras=True))
    eight = L.lle_shaping_create(bw.h, maps, 1, C.byref(config([1] * 8, [0] * 64)), st)   # the limits themselves are accepted
    assert eight, L.lle_shaping_last_error().decode()
    L.lle_shaping_free(eight)

    h = Handle(batch, [0, 1, 2], [0, 1])
    bare = Handle(batch, [0], [])
    for hd in (h, bare):
        hd.preset(random_words(batch, rng), random_words(batch, rng))
    batch.write(pos=np.stack([rng.integers(0, batch.H, (batch.n, batch.A)), rng.integers(0, batch.W, (batch.n, batch.A))], axis=2),
                evcount=random_evcount(batch, rng))

    def refused_update(why, code, hd=h, kind=0, offset_base=False, no_base=False, want_extras=True, **fields):
        before = hd.read()
        base = random_base(batch, 0 if kind not in (0, 1) else kind, rng)
        args, reward, extras, keep = hd.device_args(MARK_POS | CLEAR, MARK_POS | CLEAR, 0, kind if kind in (0, 1) else 0, None, base, True,
                                                    want_extras and hd.E > 0)
        if want_extras and hd.E == 0:   # extras_out on a handle without extras columns
            extras = Canaried(batch.n * batch.A, bw.device)
            args.extras_out = extras.out.data_ptr()
        args.reward_kind = kind
        if offset_base:
            shifted = torch.zeros(batch.n * 4 + 8, dtype=torch.float32, device=bw.device)
            assert shifted.data_ptr() % 16 == 0
            args.base_reward = shifted.data_ptr() + 4
            keep = keep + (shifted,)
        if no_base:
            args.base_reward = None
        for k, v in fields.items():
            setattr(args, k, v)
        rc = L.lle_shaping_update(hd.sh.h, C.byref(args), st)
        torch.cuda.synchronize(bw.device)
        msg = L.lle_shaping_last_error().decode()
        assert rc == code and msg, f"{why}: status {rc}, message `{msg}`"
        after = hd.read()
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), f"{why}: a refused update changed the arrays"
        assert (reward.host() == CANARY).all(), f"{why}: a refused update wrote reward_out"
        if extras is not None:
            assert (extras.host() == CANARY).all(), f"{why}: a refused update wrote extras_out"
        del keep

    refused_update("a wrong struct_bytes", LLE_ERR_ARG, struct_bytes=C.sizeof(UpdateArgs) + 8)
    refused_update("an unknown strategy op", LLE_ERR_ARG, strategy_ops=8 | MARK_POS)
    refused_update("an unknown extras op", LLE_ERR_ARG, extras_ops=16)
    refused_update("an unknown flag", LLE_ERR_ARG, flags=2 | HONOUR_AUTO_RESET)
    refused_update("reward_kind 2", LLE_ERR_ARG, kind=2)
    refused_update("reward_kind -1", LLE_ERR_ARG, kind=-1)
    refused_update("reward_out without base_reward", LLE_ERR_NULL, no_base=True)
    refused_update("kind 1 with base_reward at a 4-byte offset", LLE_ERR_ARG, kind=1, offset_base=True)
    refused_update("extras_out on a handle without extras columns", LLE_ERR_ARG, hd=bare)
    assert L.lle_shaping_update(None, C.byref(UpdateArgs(C.sizeof(UpdateArgs))), st) == LLE_ERR_NULL and L.lle_shaping_last_error()
    assert L.lle_shaping_update(h.sh.h, None, st) == LLE_ERR_NULL and L.lle_shaping_last_error()
    for which in (2, -1):
        assert L.lle_shaping_reached(h.sh.h, which) is None and L.lle_shaping_last_error().decode()
        with pytest.raises(RuntimeError, match="which"):
            h.sh.reached(which)
    # ... and the handles still work
    h.call(MARK_POS, MARK_POS, 0, 1, None, random_base(batch, 1, rng), True, True, where="after the refusals")
    bare.call(MARK_POS, 0, 0, 0, None, random_base(batch, 0, rng), True, False, where="after the refusals")


# ---------------------------------------------------------------------------------------------- every kernel
def test_every_kernel_this_file_meant_to_reach_was_launched():
    """lle_shaping_debug_launched names the kernel of every handle the tests above created (each test also asserts its own); once the
    group-shape test has run for every agent count, those are both table placements of every group size: all ten instantiations."""
    from lle_amd import shaping
    launched = set(shaping.launched_kernels())
    assert INTENDED <= launched, f"meant to run and did not: {sorted(INTENDED - launched)}"
    if RAN_AGENT_COUNTS == set(AGENT_COUNTS):
        assert INTENDED == set(shaping.compiled_kernels()) and len(INTENDED) == 10
