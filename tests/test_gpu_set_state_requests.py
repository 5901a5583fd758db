"""Refused and lived-in set_state requests by class (tests/set_state_requests.py) through world_kernel<AM, LM, MODE_SET_STATE>.

Every case: create the batch, apply the variant's layout (two maps, per-environment sources), bring it to the lived-in states of
step_states (set_state, the explicit step, two sampled steps without auto-reset), then the SECOND request of every env in one launch
-- err, evcount and the ordered events (0 and all zero after any refusal), pos, alive / arrived / occupant bits, gems, beams, avail,
done and the whole observation against the oracle --, the masked reset of the envs the reference leaves unusable (the others
bit-identical in every buffer), one sampled step with auto-reset.  Equality, no tolerance: every quantity is integral.  The oracle
decides everywhere; no output is compared with another kernel's.

The envs over which the reference panicked inside its rollback are held to err == 0x42 alone after the request (at most 5 % of a
case, asserted on the CPU: tests/test_set_state_requests_cpu.py, which also asserts the coverage of the batches); they are in the
reset mask, so they are compared again afterwards.

Every case asserts that world_kernel<AM,LM,2> (set_state) and world_kernel<AM,LM,1> (reset) of its instantiation are among
lle_debug_launched() (`-s` prints them).  That registry is cumulative for the process and cannot be emptied per case: an
instantiation notes itself at its FIRST launch only (lle_amd/csrc/kernels.hip debug_reset_launched), so after a reset the kernels
an earlier test launched would never appear again.  Run alone, this module's assertion is exact; within the whole suite it says that the
process has launched the kernel, and what the kernel computed is what every case compares."""
import functools
import time

import numpy as np
import pytest

from tests import set_state_requests as sr
from tests import step_states as ss
from tests.parity_util import assert_state_equal, legal_colours, unpack_engine

pytestmark = pytest.mark.gpu

ALL = ("pos", "bits", "gems", "beams", "avail", "actions", "err", "evcount", "events", "done", "obs")
CASES = ([(name, "single") for name in ss.MAP_NAMES] + [(name, "two-maps") for name in ss.MAP_NAMES] +
         [(name, "per-env") for name in ss.MAP_NAMES if name != "gems32"])
PER_INSTANTIATION = ["nested", "im_7_7x", "im_13_12x", "im_3_20"]   # <4,4>, <8,8>, <16,16>, <16,32>


@functools.lru_cache(maxsize=None)
def _blocks(name):
    """Two blocks of one two-map batch: the map and its variant-1 twin where instantiation_maps can build one, else the same text twice."""
    variants = (0, 1) if ss.has_twin(name) else (0, 0)
    per = ss.block_size(min(ss.build_case(name, v).n for v in variants))
    return [sr.build(name, v, per, ss.ENV_OFFSET + m * per) for m, v in enumerate(variants)]


@functools.lru_cache(maxsize=None)
def _per_env(name):
    from oracle import oracle
    from lle_amd import _capi
    from tests.test_gpu_env_sources import Mirror
    case = ss.build_case(name)
    m = _capi.Map(case.text)
    L = m.n_sources
    rng = np.random.default_rng(300 + ss.MAP_NAMES.index(name))
    colours = legal_colours(m, rng.integers(0, case.A, size=(case.n, L), dtype=np.uint8))
    enabled = rng.integers(0, 1 << L, size=case.n, dtype=np.int64)
    r = sr.reference_run(oracle, name, case, sources=lambda ob: Mirror(ob, case.n, L).apply(colours, enabled, None), rng=rng, seed_key=7)
    r.colours, r.enabled = colours, enabled
    return r


def _cat(rs, key, of=lambda r: r):
    import torch
    return torch.from_numpy(np.concatenate([getattr(of(r), key) for r in rs]))


def _engines(bw, rs, names=ALL):
    """Per block: (unpack_engine of its slice, the raw slices)."""
    host = bw.host_buffers(names)
    out, lo = [], 0
    for r in rs:
        bufs = {k: v[lo:lo + r.case.n] for k, v in host.items()}
        out.append((unpack_engine(bufs, *r.ob.dims), bufs))
        lo += r.case.n
    return out


def _live_in(bw, rs, tag):
    """step_states' protocol up to its second sampled step, checked at the end (tests/test_gpu_step_states.py checks every step of it)."""
    import torch
    case_of = lambda r: r.lived_in.case  # noqa: E731
    bw.set_state(_cat(rs, "pos", case_of), _cat(rs, "gems", case_of), _cat(rs, "alive", case_of))
    for k, rec in enumerate(rs[0].lived_in.steps):
        if rec["actions"] is not None:
            bw.step(torch.from_numpy(np.concatenate([r.lived_in.steps[k]["actions"] for r in rs])).cuda())
        else:
            bw.step(sample=True, seed=ss.SEED, t=rec["t"], env_offset=ss.ENV_OFFSET)
    for m, (r, (eng, bufs)) in enumerate(zip(rs, _engines(bw, rs))):
        assert_state_equal(eng, r.before["dump"], f"{tag}: lived-in state, block {m}")
        assert np.array_equal(bufs["done"] != 0, r.before["done"]), f"{tag}: done of the lived-in state, block {m}"


def _second_request(bw, rs, tag):
    bw.set_state(_cat(rs, "pos"), _cat(rs, "gems"), _cat(rs, "alive"))
    for m, (r, (eng, bufs)) in enumerate(zip(rs, _engines(bw, rs))):
        sr.compare_after_request(r, eng, bufs["done"], f"{tag} block {m}")


def _batch(name, variant, **kw):
    """(the batch in its lived-in states, the oracle's records per block)."""
    import torch

    from lle_amd import BatchedWorld
    rs = _blocks(name) if variant == "two-maps" else [_per_env(name)] if variant == "per-env" else [sr.build(name)]
    texts = [r.case.text for r in rs]
    bw = BatchedWorld(texts if variant == "two-maps" else texts[0], sum(r.case.n for r in rs), **kw)
    if variant == "per-env":
        bw.set_sources(torch.from_numpy(rs[0].colours), torch.from_numpy(rs[0].enabled.astype(np.int32)))
        assert int(bw.err.max()) == 0
    _live_in(bw, rs, f"{name} {variant}")
    return bw, rs


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_requests_on_lived_in_states(monkeypatch, case):
    import torch

    from lle_amd import _capi

    name, variant = case
    tag = f"{name} {variant}"
    t_start = time.perf_counter()
    monkeypatch.setenv("LLE_ROW_HEADS", "0")
    bw, rs = _batch(name, variant)
    _second_request(bw, rs, tag)

    before = bw.host_buffers(ALL)
    mask = np.concatenate([r.mask for r in rs])
    bw.reset(torch.from_numpy(mask.astype(np.uint8)).cuda())
    after, lo = bw.host_buffers(ALL), 0
    for m, (r, (eng, bufs)) in enumerate(zip(rs, _engines(bw, rs))):
        sl = slice(lo, lo + r.case.n)
        sr.compare_after_reset(r, eng, bufs["done"], {k: v[sl] for k, v in before.items()}, {k: v[sl] for k, v in after.items()}, f"{tag} block {m}")
        lo += r.case.n

    bw.step(sample=True, auto_reset=True, seed=ss.SEED, t=sr.T_STEP, env_offset=ss.ENV_OFFSET)
    for m, (r, (eng, bufs)) in enumerate(zip(rs, _engines(bw, rs))):
        sr.compare_after_step(r, eng, bufs["done"], f"{tag} block {m}")

    counts = np.sum([sr.outcome_counts(r) for r in rs], axis=0)
    if variant == "per-env":  # (each env's own world decides: the classes are not those of the map's own sources)
        assert 4 * counts[0] >= len(mask) and counts[1] + counts[2] and counts[3] and counts[4], (tag, counts.tolist())  # (0x40, 0x41, 0x42)
    inst = sr.instantiation_of(bw.map)
    launched = _capi.launched_kernels()
    for mode in (2, 1):
        assert f"{inst[:-1]},{mode}>" in launched, f"{tag} was meant to launch {inst[:-1]},{mode}>"
    print(f"\n[set-state-requests] {tag}: {inst[:-1]},2> {inst[:-1]},1> envs={len(mask)} accepted={counts[0]} 0x40-untouched={counts[1]} 0x40-applied={counts[2]} "
          f"0x41={counts[3]} 0x42={counts[4]} panic-excluded={counts[5]} wall={time.perf_counter() - t_start:.2f}s")


@pytest.mark.parametrize("name", PER_INSTANTIATION)
def test_snapshot_and_restore_after_the_requests(monkeypatch, name):
    """snapshot(), a step, restore(): every state buffer, the rows and `done` as before the step -- the ghost bits of the accepted
    requests and those a refused one left alone included (`done` is rebuilt from them) --, and again after observe()."""
    from lle_amd import _capi

    monkeypatch.setenv("LLE_ROW_HEADS", "0")
    bw, rs = _batch(name, "single")
    r = rs[0]
    _second_request(bw, rs, name)
    keys = ("pos", "bits", "gems", "beams", "avail", "obs", "done")
    was = bw.host_buffers(keys)
    keep = ~r.after_request["panicked"]
    ghost_bits = (was["bits"] >> np.uint64(48)).astype(np.int64)
    want_ghost = (r.after_request["ghost"].astype(np.int64) << np.arange(r.case.A)).sum(1)
    assert np.array_equal(ghost_bits[keep], want_ghost[keep]) and ghost_bits.any(), f"{name}: ghost bits after the requests"
    snap = bw.snapshot()
    bw.step(sample=True, auto_reset=True, seed=ss.SEED, t=sr.T_STEP, env_offset=ss.ENV_OFFSET)
    stepped = bw.host_buffers(keys)
    assert not np.array_equal(stepped["bits"], was["bits"]) and not np.array_equal(stepped["done"], was["done"]), f"{name}: the step changed nothing"
    bw.restore(snap)
    for again in (False, True):
        if again:
            bw.observe()
        now = bw.host_buffers(keys)
        for k in keys:
            assert np.array_equal(now[k], was[k]), f"{name}: '{k}' after restore" + (" and observe" if again else "")
        assert np.array_equal(now["done"][keep] != 0, r.after_request["done"][keep])
    inst = sr.instantiation_of(bw.map)
    assert f"{inst[:-1]},3>" in _capi.launched_kernels(), f"{name} was meant to launch {inst[:-1]},3>"


def test_widened_rows_after_the_requests(monkeypatch):
    """A widened batch (float16 rows): the row set_state writes shows the applied state after an accepted request and after a 0x40
    mismatch, the untouched one after dup / oob, the rolled-back one after 0x42 -- the oracle's observation, cast."""
    import torch

    monkeypatch.setenv("LLE_ROW_HEADS", "0")
    name = "nested"
    bw, rs = _batch(name, "single", obs_dtype=torch.float16)
    r = rs[0]
    bw.set_state(_cat(rs, "pos"), _cat(rs, "gems"), _cat(rs, "alive"))
    host = bw.host_buffers(("err", "obs"))
    rec = r.after_request
    keep = ~rec["panicked"]
    assert np.array_equal(host["err"], rec["err"])
    assert host["obs"].dtype == np.float16
    want = rec["obs"].reshape(r.case.n, -1).astype(np.float16)
    assert np.array_equal(host["obs"][keep, :want.shape[1]], want[keep]), f"{name}: widened rows after the requests"
    assert not host["obs"][:, want.shape[1]:].any(), f"{name}: padding of the widened rows"
    for code in (0, 0x40, 0x41, 0x42):
        assert (rec["err"][keep] == code).any(), hex(code)
