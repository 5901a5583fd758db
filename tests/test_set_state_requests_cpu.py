"""Refused and lived-in set_state requests by class (tests/set_state_requests.py) on the host build of the device state machine.

The protocol of tests/test_gpu_set_state_requests.py on tests/hostsim (step_logic.hpp set_state_env / apply_state, the code of
world_kernel<AM, LM, MODE_SET_STATE>): the lived-in states, the second request, the masked reset, the follow-up step -- every env
against the oracle after each of them.  The coverage assertions live here, so a generator that lost a class fails before a GPU is
booked; every class is decided from the oracle's outcomes.

Not compared after the second request: the envs over which the REFERENCE panicked during the call (`set_state(current_state).unwrap()`
inside the 0x42 rollback).  They carry the rollback-panic flag, are held to err == 0x42, are capped at 5 % of a case, and are reset
right after, so everything later is compared again."""
import numpy as np
import pytest

from tests import set_state_requests as sr
from tests import step_states as ss
from tests.parity_util import legal_colours, unpack_engine
from tests.test_step_states_cpu import PER_ENV_MAPS, _bufs, _load_requests

RAW = ("pos", "bits", "gems", "beams", "avail", "actions", "err", "evcount", "events", "done", "obs")


def instantiation(name):
    from lle_amd import _capi
    return sr.instantiation_of(_capi.Map(ss.text_of(name)))


def run_protocol(sb, r, tag):
    """The engine's side on a SimBatch that stands where step_states' protocol left it after its second sampled step."""
    from lle_amd import _capi, _decode
    dims = r.ob.dims
    sb.buf("req_pos")[:] = r.pos
    sb.buf("req_gems")[:] = [_decode.pack_bits(g) for g in r.gems]
    sb.buf("req_alive")[:] = [_decode.pack_bits(a) for a in r.alive]
    sb.set_state()
    sr.compare_after_request(r, unpack_engine(_bufs(sb), *dims), sb.buf("done"), tag)
    before = {k: sb.buf(k).copy() for k in RAW}
    sb.reset(r.mask.astype(np.uint8))
    sr.compare_after_reset(r, unpack_engine(_bufs(sb), *dims), sb.buf("done"), before, {k: sb.buf(k) for k in RAW}, tag)
    sb.step(None, flags=_capi.LLE_STEP_SAMPLE_ACTIONS | _capi.LLE_STEP_AUTO_RESET, seed=ss.SEED, t=sr.T_STEP, env_offset=r.env_offset)
    sr.compare_after_step(r, unpack_engine(_bufs(sb), *dims), sb.buf("done"), tag)


def lived_in(sb, ref, env_offset=ss.ENV_OFFSET):
    """set_state, the explicit step and the sampled steps of step_states on the engine, checked at the end only (every step of it is
    checked by tests/test_step_states_cpu.py)."""
    from lle_amd import _capi
    from tests.parity_util import assert_state_equal
    _load_requests(sb, ref.case)
    sb.set_state()
    for rec in ref.steps:
        if rec["actions"] is not None:
            sb.step(rec["actions"])
        else:
            sb.step(None, flags=_capi.LLE_STEP_SAMPLE_ACTIONS, seed=ss.SEED, t=rec["t"], env_offset=env_offset)
    assert_state_equal(unpack_engine(_bufs(sb), *ref.ob.dims), ref.steps[-1]["dump"], "lived-in state")
    assert np.array_equal(sb.buf("done") != 0, ref.steps[-1]["done"])


@pytest.mark.parametrize("name", ss.MAP_NAMES)
def test_requests_on_lived_in_states(name):
    from tests import hostsim

    r = sr.build(name)
    sb = hostsim.SimBatch(r.case.text, r.case.n)
    lived_in(sb, r.lived_in)
    run_protocol(sb, r, name)


@pytest.mark.parametrize("name", PER_ENV_MAPS)
def test_requests_with_per_env_sources(oracle_mod, name):
    """Per-environment colours and enabled flags first: each env's OWN world decides the outcome of its request."""
    from tests import hostsim
    from tests.test_gpu_env_sources import Mirror

    case = ss.build_case(name)
    sb = hostsim.SimBatch(case.text, case.n)
    L = sb.map.n_sources
    rng = np.random.default_rng(len(name) + 40)
    colours = legal_colours(sb.map, rng.integers(0, case.A, size=(case.n, L), dtype=np.uint8))
    enabled = rng.integers(0, 1 << L, size=case.n, dtype=np.int64)
    sb.set_sources(colours, enabled.astype(np.uint32))
    r = sr.reference_run(oracle_mod, name, case, sources=lambda ob: Mirror(ob, case.n, L).apply(colours, enabled, None), rng=rng, seed_key=7)
    lived_in(sb, r.lived_in)
    run_protocol(sb, r, f"{name} per-env sources")
    counts = sr.outcome_counts(r)
    assert 4 * counts[0] >= case.n and counts[1] + counts[2] and counts[3] and counts[4], counts  # (0x40, 0x41, 0x42)


@pytest.mark.parametrize("name", ss.MAP_NAMES)
def test_coverage_of_every_map(name):
    """Per map: ragged and below 8 192 envs; every class its geometry can show has an env; what the reference leaves untouched is
    untouched in the ORACLE (the engines are held to the oracle, the oracle to this); the panic cap."""
    r = sr.build(name)
    n, f, rec = r.case.n, r.flags, r.after_request
    assert n % 16 == 5 and n < ss.MAX_ENVS
    for cls in sr.structural_classes(name, r.layout):
        assert f.get(cls, np.zeros(n, bool)).any(), f"{name}: no env of class '{cls}'"
    untouched = f.get("0x40-untouched", np.zeros(n, bool)) | f["0x41"]
    for key in sr.STATE_KEYS:
        assert np.array_equal(rec["dump"][key][untouched], r.before["dump"][key][untouched]), f"{name}: the oracle touched '{key}' on a dup / oob request"
    refused = rec["err"] != 0
    assert not rec["ev_count"][refused].any() and not rec["events"][refused].any()
    assert np.array_equal(rec["ghost"][refused], r.before["ghost"][refused])
    # the cap: the only envs whose state after the call is not compared
    panicked = rec["panicked"]
    assert (rec["err"][panicked] == 0x42).all() and (f.get("rollback-panic", np.zeros(n, bool)) == panicked).all()
    assert 20 * int(panicked.sum()) <= n, f"{name}: the reference panicked on {int(panicked.sum())} of {n} envs"
    assert (r.mask | ~panicked).all() and np.array_equal(r.mask, ((rec["err"] == 0x40) & ~f.get("0x40-untouched", np.zeros(n, bool))) | panicked)
    assert not r.panics_after_step.any(), f"{name}: the reference panicked in the reset or the follow-up step"
    # a request that was applied and then refused has a cause this module knows: a death on a void or a beam, a gem left or not taken
    assert "panic-other" not in f, f"{name}: unexplained panic on envs {np.nonzero(f.get('panic-other', []))[0][:8].tolist()}"
    assert "mismatch-other" not in f, f"{name}: unexplained mismatch on envs {np.nonzero(f.get('mismatch-other', []))[0][:8].tolist()}"


@pytest.mark.parametrize("inst", sr.INSTANTIATIONS)
def test_coverage_of_every_instantiation(inst):
    """Per world_kernel instantiation, over its maps: at least a quarter of the envs accepted, every kind of refusal there, and the
    classes that need a lived-in state (revivals, ghosts over dead agents, rollbacks that show / that panic)."""
    names = [m for m in ss.MAP_NAMES if instantiation(m) == inst]
    assert names, inst
    total, counts, n_all = {}, np.zeros(6, np.int64), 0
    for m in names:
        r = sr.build(m)
        counts += sr.outcome_counts(r)
        n_all += r.case.n
        for k, v in r.flags.items():
            total[k] = total.get(k, 0) + int(v.sum())
    print(f"\n[set-state-requests] {inst}: maps={names} envs={n_all} accepted={counts[0]} 0x40-untouched={counts[1]} 0x40-applied={counts[2]} "
          f"0x41={counts[3]} 0x42={counts[4]} panic-excluded={counts[5]} (over a walked-off gem {total.get('panic-collected-gem-under-beam', 0)}, over a corpse on a collected gem "
          f"{total.get('panic-corpse-on-collected-gem', 0)}, over an agent under a re-lit beam {total.get('panic-alive-under-relit-beam', 0)}) events out of agent order={total.get('id-inversion', 0)}")
    assert 4 * counts[0] >= n_all, (inst, counts.tolist(), n_all)
    assert all(counts[1:5]), (inst, counts.tolist())
    for cls in ("revive", "revive-on-own-lit-beam", "revive-with-dead-owner-in-lit-beam", "ghost-from-lived-in", "rollback-visible", "rollback-panic",
                "bury-floor", "bury-exit", "bury-gem", "bury-lit-beam", "event-gem", "event-exit", "event-died-requested-dead", "all-arrived",
                "own-beam-1", "own-beam-2", "mismatch-beam", "mismatch-void", "mismatch-gem-left", "mismatch-gem-under-beam"):
        assert total.get(cls, 0) > 0, f"{inst}: no env of class '{cls}' on {names}"
    # the rollbacks that panic over a corpse on a collected gem, or over a living agent under a beam re-lit over it, need a lived-in
    # state that random requests do not make: three instantiations hold such envs, the batch of im_3_20 (<16,32>) none
    if inst != "world_kernel<16,32>":
        for cls in ("panic-collected-gem-under-beam", "panic-corpse-on-collected-gem", "panic-alive-under-relit-beam"):
            assert total.get(cls, 0) > 0, f"{inst}: no env of class '{cls}' on {names}"


def test_no_lived_in_state_holds_a_corpse_the_rollback_lets_onto_its_uncollected_gem():
    """The one rollback-panic the batches cannot show: a corpse on an uncollected gem under a beam that the rollback lets into the
    gem's tile.  It died there because the beam was lit; the beam's owner would have to stand further up the beam two sampled steps
    later.  Every env of every map is searched for that state (the planter's exact precondition) and none holds it, nor does the
    oracle report such a panic after a random request.  If step_states ever brings one, this fails: require the class then."""
    for name in ss.MAP_NAMES:
        r = sr.build(name)
        assert "panic_corpse" not in r.kinds and "panic-corpse-on-gem" not in r.flags, name


def test_instantiations_of_the_maps():
    """The maps reach all four instantiations of world_kernel, by the product's own map description."""
    assert {instantiation(name) for name in ss.MAP_NAMES} == set(sr.INSTANTIATIONS)
