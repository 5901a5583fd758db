"""The write footprint of every batch launch, byte by byte (tests/arena_footprint.py: guards, whole-arena diff, poison).

No oracle: whether the bytes a call MAY write are right is the other suites' job.  Here every batch lives in the middle of a poisoned
allocation, every ring / output / input tensor of the caller likewise, the whole arena is compared before and after each checked call
against the RULES row of that call, and the output-only buffers the call must not touch are poisoned first, so that a stray write of the
value that was there anyway shows too.  After a call that writes rows, no byte of the first n rows still holds the poison and the row
padding is zero.

One map per lanes-per-environment G -- 1 solo_beams, 2 gems32, 4 long_three_words (chained beam words), 8 config5_32x32 (20 KiB rows:
split over the wavefronts of a workgroup), 16 many_agents -- at n = 5 and n = W + 5 environments, W = 4 * 64 / G one full workgroup, so
that the last wavefront is partly filled (2 W + 5 too on the split-row map); batches of 9 maps x 1 / 3 / 5 / 12 environments on the G = 4
and G = 16 shapes.  Each batch is driven a few sampled steps with auto-reset, then ONE call of each kind is checked.  autotune_ms=0
everywhere: which kernel a case launches never depends on timing.  The last test asserts from lle_debug_launched() that a step_kernel of
every MODE 0-9 and every G, the world kernel and the three partial observer kernels ran under the checker.

Measured on one MI355X: the whole module takes 11 seconds of wall time (WALL_S), no case more than 2.1 s."""
import numpy as np
import pytest

from tests import arena_footprint as af
from tests import step_states as ss
from tests.arena_footprint import POISON, RULES, Guarded, step_rule

pytestmark = pytest.mark.gpu

WALL_S = 11     # wall time of this module on one MI355X, seconds (226 cases; the slowest, the first of the process, 2.1 s)

MAP_OF_G = {1: "solo_beams", 2: "gems32", 4: "long_three_words", 8: "config5_32x32", 16: "many_agents"}
HEADS = ("solo_beams", "gems32", "long_three_words")         # maps whose rows have a head (tests/test_gpu_step_states.py HEAD_MAPS)
PES_HEADS = ("long_three_words",)                            # ... under per-environment sources (PES_HEAD_MAPS)
PARTIAL = ("solo_beams", "gems32", "long_three_words")       # at most 8 beam words and rows that are not split (step_kernel MODE 9)
NO_SOURCES = ("gems32",)
RECOLOUR = ("solo_beams", "many_agents")                     # maps LLE_STEP_RECOLOUR_RESETS serves (long_three_words: LLE_ERR_UNSUPPORTED, a chained beam)
MODE = {"default": 0, "heads": 6, "outputs": 4, "outputs-heads": 7, "per-env": 5, "per-env-heads": 8, "recolour": 5, "rollout": 1,
        "rollout-ring": 1, "planned": 1, "per-env-rollout": 3, "partial": 9, "incremental": 0, "no-obs": 0, "envs-per-wave": None}
P_STEP = ("obs", "reward", "events", "evcount", "err")
STAY = 4


def sizes(g):
    w = 4 * 64 // g
    return [5, w + 5] + ([2 * w + 5] if g == 8 else [])


def variants_of(name):
    v = ["default", "outputs", "rollout", "rollout-ring", "planned", "incremental", "no-obs", "envs-per-wave"]
    if name in HEADS:
        v += ["heads", "outputs-heads"]
    if name not in NO_SOURCES:
        v += ["per-env", "per-env-rollout"]
    if name in PES_HEADS:
        v += ["per-env-heads"]
    if name in RECOLOUR:
        v += ["recolour"]
    if name in PARTIAL:
        v += ["partial"]
    return v


STEP_CASES = [(MAP_OF_G[g], n, v, "int8") for g in MAP_OF_G for n in sizes(g) for v in variants_of(MAP_OF_G[g])]
WIDE = ("float16", "bfloat16", "float32")
STEP_CASES += [(MAP_OF_G[g], n, v, dt) for g in MAP_OF_G for n in sizes(g)[1:2] for v in ("default", "per-env", "rollout-ring")
               if not (v == "per-env" and MAP_OF_G[g] in NO_SOURCES) for dt in WIDE]
STEP_CASES += [("config5_32x32", n, "default", dt) for n in (5, 69) for dt in WIDE]   # the split rows at every size
WORLD_CASES = [(MAP_OF_G[g], n, "int8") for g in MAP_OF_G for n in sizes(g)] + [(MAP_OF_G[g], sizes(g)[1], dt) for g in MAP_OF_G for dt in WIDE]
EXPECTED = set()   # (G, MODE) of the step kernels the cases that ran were meant to launch


def _dtype(name):
    import torch
    return {"int8": None, "float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[name]


def _sources(bw, seed):
    """Legal per-environment colours and enabled masks."""
    import torch

    from tests.parity_util import legal_colours
    rng = np.random.default_rng(seed)
    L = bw.map.n_sources
    colours = legal_colours(list(bw.maps), rng.integers(0, bw.map.n_agents, size=(bw.n_envs, L), dtype=np.uint8))
    enabled = rng.integers(0, 1 << L, size=bw.n_envs, dtype=np.int64).astype(np.int32)
    return torch.from_numpy(colours), torch.from_numpy(enabled)


def _world(texts, n, monkeypatch, heads=False, dtype="int8", pes=False, steps=4, **kw):
    """A guarded batch, driven `steps` sampled steps with auto-reset so that beams are cut and agents have died and arrived."""
    monkeypatch.setenv("LLE_ROW_HEADS", "1" if heads else "0")
    bw, fp = af.guarded_world(texts, n, autotune_ms=0, row_align=128 if heads else None, obs_dtype=_dtype(dtype), **kw)
    if pes:
        bw.set_sources(*_sources(bw, 7))   # (the first call hands every env the map's sources first: not a checked call)
        assert int(bw.err.max()) == 0
    for _ in range(steps):
        bw.step(sample=True, auto_reset=True, seed=11, env_offset=3)
    return bw, fp


def _guarded_input(t, what):
    g = Guarded(t.numel() * t.element_size(), what, device="cuda")
    view = g.tensor(t.dtype, tuple(t.shape))
    view.copy_(t)
    return g, view


def _outputs(bw, multi=False):
    import torch
    n, A, G = bw.n_envs, bw.map.n_agents, bw.map.n_gems
    spec = dict(state=(torch.float32, (n, 3 * A + G)), reward=(torch.float32, (n, 4 if multi else 1)), done=(torch.uint8, (n,)),
                available=(torch.uint8, (n, A, 5)), alive=(torch.uint8, (n, A)), arrived=(torch.uint8, (n, A)))
    guards = {k: Guarded(int(np.prod(shape)) * dt.itemsize, f"the `{k}` output", device=bw.device) for k, (dt, shape) in spec.items()}
    return guards, {k: guards[k].tensor(*spec[k]) for k in spec}


def _assert_filled(g, mask=None, zero_pad=False):
    """No POISON byte is left in the output (inside `mask` when given); with zero_pad the bytes outside the mask are zero."""
    host = g.host()
    view = host[g.lo:g.lo + g.nbytes]
    inside = view if mask is None else view[mask]
    assert not (inside == POISON).any(), f"{g.what}: {int((inside == POISON).sum())} byte(s) inside the announced size were not written"
    if zero_pad and mask is not None:
        assert not view[~mask].any(), f"{g.what}: the row padding is not zero"
    assert g.violations(host) == [], g.violations(host)


def _ring(bw, slots):
    import torch
    n, m, item = bw.n_envs, bw.map, bw.obs_dtype.itemsize
    pitch = bw._desc["actions"][4][0]
    row = m.obs_stride * item
    g = {"obs": Guarded(slots * n * row, "the observation ring", device=bw.device, row_bytes=row),
         "actions": Guarded(slots * n * pitch, "the action ring", device=bw.device), "reward": Guarded(slots * n * 4, "the reward ring", device=bw.device)}
    ring = {"slots": slots, "obs_rows": g["obs"].tensor(bw.obs_dtype, (slots, n, m.obs_stride)),
            "actions_rows": g["actions"].tensor(torch.uint8, (slots, n, pitch)), "reward": g["reward"].tensor(torch.uint8, (slots, n, 4))}
    return g, ring


def _check_ring(bw, g, slots, targeted, sampled, plan=None):
    m, item, n = bw.map, bw.obs_dtype.itemsize, bw.n_envs
    pitch, row = bw._desc["actions"][4][0], m.obs_stride * item
    bad = []
    hosts = {k: v.host() for k, v in g.items()}
    for k, v in g.items():
        bad += v.violations(hosts[k])
    view = {k: hosts[k][v.lo:v.lo + v.nbytes] for k, v in g.items()}
    bad += af.ring_violations(view["obs"], slots, targeted, "the observation ring", record=row)
    bad += af.ring_violations(view["reward"], slots, targeted, "the reward ring", record=4)
    rows = view["obs"].reshape(slots, n, row)
    if any(rows[s][:, m.obs_bytes * item:].any() for s in targeted):
        bad.append("ring: the row padding of a targeted slot is not zero")
    if sampled:
        bad += af.ring_violations(view["actions"], slots, targeted, "the action ring", record=pitch, payload=m.n_agents)
    else:   # the action ring is the launch's INPUT: not a byte of it changes
        if not np.array_equal(view["actions"], plan):
            bad.append(f"ring: {int((view['actions'] != plan).sum())} byte(s) of the planned actions were overwritten")
    assert not bad, "\n  ".join(bad)


def _no_state_change(fp, envs, what):
    hit = [k for k in fp.found if k[0] in af.STATE and k[1] in envs]
    assert not hit, f"{what}: the state of refused environments changed: {hit[:6]}"


# ---------------------------------------------------------------------------------------------- the step launches
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_step_footprint(case, monkeypatch):
    import torch

    from lle_amd import _capi

    name, n, variant, dtype = case
    heads = variant in ("heads", "outputs-heads", "per-env-heads")
    pes = variant in ("per-env", "per-env-heads", "recolour", "per-env-rollout")
    bw, fp = _world(ss.text_of(name), n, monkeypatch, heads=heads, dtype=dtype, pes=pes)
    A = bw.map.n_agents
    if heads:
        assert bw.map.n_beam_words <= 8 and (bw.map.row_head_env_sources if pes else bw.map.row_head)[1] != 0
    if MODE[variant] is not None:
        EXPECTED.add((ss.group_size(A), MODE[variant]))

    if variant in ("default", "heads", "per-env", "per-env-heads", "envs-per-wave"):
        if variant == "envs-per-wave":
            bw.set_envs_per_wave(8)
        # sampled, with auto-reset
        with fp.watch(step_rule(True), poison=P_STEP + ("actions",)):
            bw.step(sample=True, auto_reset=True, seed=5, env_offset=9)
        # given actions, every third env refused by its last agent, no auto-reset
        acts = bw.actions[:, :A].clone()
        acts[::3, A - 1] = 7
        g, given = _guarded_input(acts, "the actions input")
        with fp.watch(step_rule(True), poison=P_STEP + ("actions", "done"), extra=[g]):
            bw.step(given)
        assert torch.equal(given, acts), "the step wrote into its actions input"
        err = bw.err.cpu().numpy()
        refused = set(np.flatnonzero((err >= 1) & (err <= 16)).tolist())
        assert set(range(0, n, 3)) <= refused and (len(refused) < n or n == 5)
        _no_state_change(fp, refused, f"{name} {variant}")
        # LLE_BUF_ACTIONS read where it is: not a byte of it changes
        with fp.watch(step_rule(False), poison=P_STEP + ("done",)):
            bw.step(bw.actions)
    elif variant in ("outputs", "outputs-heads"):
        for multi in (False, True):
            guards, outs = _outputs(bw, multi)
            env_out = bw.make_env_outputs(multi_objective=multi, **outs)
            with fp.watch(step_rule(True), poison=P_STEP + ("actions",), extra=list(guards.values())):
                bw.step(sample=True, auto_reset=True, seed=5, env_out=env_out)
            for g in guards.values():
                _assert_filled(g)
    elif variant == "recolour":
        with fp.watch(step_rule(True, recolour=True), poison=P_STEP + ("actions",)):
            bw.step(sample=True, auto_reset=True, recolour_resets=True, seed=5)
    elif variant in ("rollout", "per-env-rollout"):
        with fp.watch(step_rule(True), poison=P_STEP + ("actions",)):
            bw.rollout(3, auto_reset=True, seed=5)
    elif variant == "rollout-ring":
        g, ring = _ring(bw, 4)
        for pos, steps in ((0, 3), (3, 6)):   # slots 0 1 2, then 3 0 1 2 3 0: the ring wraps
            for v in g.values():
                v.bytes.fill_(POISON)
            with fp.watch(step_rule(True, ring=True), poison=P_STEP + ("actions",)):
                bw.rollout(steps, auto_reset=True, seed=5, ring=ring, ring_pos=pos)
            _check_ring(bw, g, 4, {(pos + j) % 4 for j in range(steps)}, sampled=True)
            bw.actions.fill_(STAY)
    elif variant == "planned":
        g, ring = _ring(bw, 4)
        plan = torch.full_like(ring["actions_rows"], STAY)
        plan[:, ::3, A - 1] = 6                      # refused envs keep their state and go on with the next step
        ring["actions_rows"].copy_(plan)
        bw.actions.fill_(STAY)
        with fp.watch(step_rule(False, ring=True), poison=P_STEP):
            bw.rollout(3, auto_reset=False, ring=ring, ring_pos=2, sample=False)   # slots 2 3 0
        _check_ring(bw, g, 4, {2, 3, 0}, sampled=False, plan=plan.cpu().numpy().reshape(-1))
    elif variant == "partial":
        for k in (3, 5):
            d = bw.obs_desc(_capi.LLE_OBS_PARTIAL, k)
            assert d.supported
            gp = Guarded(int(d.bytes), f"the partial {k} x {k} buffer", device=bw.device)
            gs, outs = _outputs(bw)
            env_out = bw.make_env_outputs(state=outs["state"], partial=gp.bytes, partial_k=k)
            # the partial observation INSTEAD of the layered one (lle_hip.h lle_env_outputs.partial): every byte of `obs` stays
            with fp.watch(step_rule(True, partial=True), poison=P_STEP + ("actions",), extra=[gp, gs["state"]]):
                bw.step(sample=True, auto_reset=True, seed=5, env_out=env_out)
            mask = af.strided_payload_mask(d.bytes, [d.shape[q] for q in range(d.ndim)], [d.stride[q] for q in range(d.ndim)], d.elem_bytes)
            _assert_filled(gp, mask)   # (rows padded to 16 bytes: the header fixes no content for the padding)
            _assert_filled(gs["state"])
    elif variant == "incremental":
        bw.observe()
        with fp.watch(step_rule(True, incremental=True), poison=P_STEP + ("actions",)):
            bw.step(sample=True, auto_reset=True, seed=5, incremental_obs=True)
        bw.observe()
        assert bw.check_obs() == 0
    elif variant == "no-obs":
        with fp.watch(step_rule(True, write_obs=False), poison=P_STEP + ("actions",)):
            bw.step(sample=True, auto_reset=True, seed=5, write_obs=False)
    else:
        raise AssertionError(variant)
    bw.observe()   # (rows and `done` back in line with the state behind the poisoned calls)
    assert dtype != "int8" or bw.check_obs() == 0


# ---------------------------------------------------------------------------------------------- the world-kernel operations
def _requests(bw, start_pos, seed):
    """Even envs ask for the start state (accepted), odd ones for tests/set_state_requests.random_request (mostly refused)."""
    import torch

    from tests import set_state_requests as ssr

    class Dims:
        H, W, A, G = bw.map.height, bw.map.width, bw.map.n_agents, bw.map.n_gems
    rng = np.random.default_rng(seed)
    n, A, G = bw.n_envs, Dims.A, Dims.G
    pos, gems, alive = np.zeros((n, A, 2), np.uint8), np.zeros((n, G), bool), np.ones((n, A), bool)
    pos[:] = start_pos
    for e in range(1, n, 2):
        p, g, a = ssr.random_request(rng, Dims)
        pos[e], gems[e], alive[e] = np.array(p, np.uint8), g, a
    return torch.from_numpy(pos), torch.from_numpy(gems), torch.from_numpy(alive)


@pytest.mark.parametrize("case", WORLD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_world_operations_footprint(case, monkeypatch):
    import torch

    from lle_amd import _capi

    name, n, dtype = case
    bw, fp = _world(ss.text_of(name), n, monkeypatch, dtype=dtype, steps=0)
    start_pos = bw.pos.cpu().numpy().copy()
    P_WORLD = ("obs", "err", "evcount", "events", "done")
    for _ in range(4):
        bw.step(sample=True, auto_reset=True, seed=11)
    # reset, every env
    with fp.watch(RULES["reset"], envs=range(n), poison=P_WORLD + ("reward",)):
        bw.reset()
    for _ in range(4):
        bw.step(sample=True, auto_reset=True, seed=12)
    # reset, a seeded half mask: an unmasked env keeps state and results (still poisoned); its row is rebuilt from its own state
    rng = np.random.default_rng(n)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    mask[0], mask[n - 1] = 1, 0
    g, mask_dev = _guarded_input(torch.from_numpy(mask), "the reset mask")
    with fp.watch(RULES["reset"], envs=np.flatnonzero(mask), poison=P_WORLD + ("reward",), extra=[g]):
        bw.reset(mask_dev)
    assert torch.equal(mask_dev.cpu(), torch.from_numpy(mask))
    bw.observe()
    # set_state: accepted and refused requests
    bw.step(sample=True, seed=13)
    req = _requests(bw, start_pos, n)
    bw.set_state(*req)                # (fills req_* first; the checked call is the launch alone: req_* are its inputs and must not change)
    bw.step(sample=True, seed=13, t=1)
    with fp.watch(RULES["set_state"], poison=P_WORLD + ("reward",)):
        bw._check(_capi.lib().lle_batch_set_state(bw.h, bw._stream()))
    err = bw.err.cpu().numpy()
    assert (err == 0).any() and (err != 0).any(), f"{name}: the requests hold {int((err == 0).sum())} accepted and {int((err != 0).sum())} refused"
    # observe
    with fp.watch(RULES["observe"], poison=("obs", "done", "reward", "events", "evcount", "err")):
        bw.observe()
    for _ in range(2):
        bw.step(sample=True, auto_reset=True, seed=14)
    # stats
    with fp.watch(RULES["stats"], poison=P_WORLD + ("reward",)):
        st = bw.stats(reset=False)
    assert st["env_steps"] > 0
    with fp.watch(RULES["stats"], poison=P_WORLD + ("reward",)):
        bw.stats(reset=True)
    assert bw.stats()["env_steps"] == 0
    bw.observe()
    # snapshot / restore
    with fp.watch(RULES["snapshot"], poison=P_WORLD + ("reward",)):
        snap = bw.snapshot()
    bw.observe()
    bw.step(sample=True, auto_reset=True, seed=15)
    with fp.watch(RULES["restore"], poison=("obs", "done", "reward", "events", "evcount", "err")):
        bw.restore(snap)
    # exits: the same cells in another order (World.exit_pos = ...): tables, init record, hidden env, rows
    with fp.watch(RULES["update_map"], maps={0}, poison=("obs", "reward", "events", "evcount", "err")):
        bw.set_exits(list(reversed(bw.map.positions(_capi.LLE_POS_EXIT))))
    if name in NO_SOURCES:
        return
    # sources of the map: source 0 off, then on again
    for on in (False, True):
        bw.map.set_source(0, enabled=on)
        with fp.watch(RULES["update_map"], maps={0}, poison=("obs", "reward", "events", "evcount", "err")):
            bw.update_sources()
    # ---- per-environment sources (the first call fills every env with the map's sources: not a checked call)
    bw.set_sources(*_sources(bw, 1))
    assert int(bw.err.max()) == 0
    for _ in range(3):
        bw.step(sample=True, auto_reset=True, seed=16)
    colours, enabled = _sources(bw, 2)
    colours[1::4, 0] = 200    # refused per env: LLE_ENV_INVALID_COLOUR, none of its sources changed
    gm, mask_dev = _guarded_input(torch.from_numpy(mask), "the source mask")
    gc, col_dev = _guarded_input(colours, "the colours input")
    ge, en_dev = _guarded_input(enabled, "the enabled input")
    with fp.watch(RULES["set_sources"], envs=np.flatnonzero(mask), poison=("obs", "reward", "events", "evcount"), extra=[gm, gc, ge]):
        bw.set_sources(col_dev, en_dev, mask_dev)
    err = bw.err.cpu().numpy()
    assert n < 8 or ((err == 0x43) & (mask != 0)).any()
    with fp.watch(RULES["reset_sources"], envs=np.flatnonzero(mask), poison=P_WORLD + ("reward",), extra=[gm, gc, ge]):
        bw.set_sources(col_dev, en_dev, mask_dev, reset_first=True)
    assert torch.equal(col_dev.cpu(), colours) and torch.equal(en_dev.cpu(), enabled) and torch.equal(mask_dev.cpu(), torch.from_numpy(mask))
    bw.observe()
    # LLE_OBS_LAYERED with per-environment sources: the world kernel's OBSERVE mode on the caller's buffer (the one observer that may store `done`)
    d = bw.obs_desc(_capi.LLE_OBS_LAYERED, 0)
    if d.supported:
        out = Guarded(int(d.bytes), "layered, per-environment sources", device=bw.device, row_bytes=bw.map.obs_stride * bw.obs_dtype.itemsize)
        with fp.watch(RULES["observer-layered-per-env"], poison=("obs", "reward", "events", "evcount", "err"), extra=[out]):
            bw.observe_as(_capi.LLE_OBS_LAYERED, 0, out=out.bytes)
        _assert_filled(out, af.strided_payload_mask(d.bytes, [d.shape[q] for q in range(d.ndim)], [d.stride[q] for q in range(d.ndim)], d.elem_bytes), zero_pad=True)
        bw.observe()
    bw.step(sample=True, auto_reset=True, seed=17)
    with fp.watch(RULES["snapshot"], poison=P_WORLD + ("reward",)):
        snap = bw.snapshot()
    bw.observe()
    bw.step(sample=True, auto_reset=True, seed=18)
    with fp.watch(RULES["restore-per-env"], poison=("obs", "reward", "events", "evcount")):
        bw.restore(snap)
    with fp.watch(RULES["update_map-per-env"], maps={0}, poison=("obs", "reward", "events", "evcount")):
        bw.set_exits(list(reversed(bw.map.positions(_capi.LLE_POS_EXIT))))
    assert dtype != "int8" or bw.check_obs() == 0


# ---------------------------------------------------------------------------------------------- batches of several maps
MULTI_SHAPES = {4: dict(height=9, width=11, n_agents=3, n_lasers=4, n_gems=3, n_voids=2), 16: dict(height=12, width=12, n_agents=12, n_lasers=6, n_gems=4, n_voids=2)}


@pytest.mark.parametrize("per", [1, 3, 5, 12])
@pytest.mark.parametrize("g", [4, 16])
def test_multi_map_footprint(g, per, monkeypatch):
    """9 maps x `per` environments (tests/test_gpu_multi_map.py::test_few_envs_per_map shows these are legal): a wavefront serves one map."""
    import torch

    from lle_amd import _capi
    from tests.test_gpu_multi_map import _maps

    texts = _maps(9, **MULTI_SHAPES[g])
    n = 9 * per
    bw, fp = _world(texts, n, monkeypatch)
    EXPECTED.update({(g, 4), (g, 2)})
    with fp.watch(step_rule(True), poison=P_STEP + ("actions",)):
        bw.step(sample=True, auto_reset=True, seed=5)
    with fp.watch(step_rule(True), poison=P_STEP + ("actions",)):
        bw.rollout(3, auto_reset=True, seed=6)
    gr, ring = _ring(bw, 4)
    with fp.watch(step_rule(True, ring=True), poison=P_STEP + ("actions",)):
        bw.rollout(3, auto_reset=True, seed=7, ring=ring, ring_pos=3)
    _check_ring(bw, gr, 4, {3, 0, 1}, sampled=True)
    bw.actions.fill_(STAY)
    bw.observe()
    mask = (np.random.default_rng(per).random(n) < 0.5).astype(np.uint8)
    mask[0], mask[n - 1] = 1, 0
    gm, mask_dev = _guarded_input(torch.from_numpy(mask), "the reset mask")
    with fp.watch(RULES["reset"], envs=np.flatnonzero(mask), poison=("obs", "err", "evcount", "events", "done", "reward"), extra=[gm]):
        bw.reset(mask_dev)
    bw.observe()
    # map 1 takes its exits in another order: map 0's table slot (and every other map's) holds
    with fp.watch(RULES["update_map-multi"], maps={1}, poison=("obs", "reward", "events", "evcount", "err")):
        bw.set_exits(list(reversed(bw.maps[1].positions(_capi.LLE_POS_EXIT))), map_index=1)
    with fp.watch(RULES["observe"], poison=("obs", "done", "reward", "events", "evcount", "err")):
        bw.observe()


def test_two_map_update_holds_the_other_slot(monkeypatch):
    """Two maps x 21 environments: map 1 takes its exits in another order -- not a byte of map 0's table slot changes, nor of `req_*`,
    `stats` or the state of any env; then map 0 likewise, and map 1's slot holds."""
    from lle_amd import _capi
    from tests.test_gpu_multi_map import _maps

    bw, fp = _world(_maps(2, **MULTI_SHAPES[4]), 42, monkeypatch)
    for m in (1, 0):
        with fp.watch(RULES["update_map-multi"], maps={m}, poison=("obs", "reward", "events", "evcount", "err")):
            bw.set_exits(list(reversed(bw.maps[m].positions(_capi.LLE_POS_EXIT))), map_index=m)
        assert not any(k[0] == "internal:tables" and k[1] != m for k in fp.found), fp.found
    assert bw.check_obs() == 0


# ---------------------------------------------------------------------------------------------- the observers
@pytest.mark.parametrize("dtype", ["int8", "float32"])
@pytest.mark.parametrize("g", sorted(MAP_OF_G))
def test_observers_footprint(g, dtype, monkeypatch):
    """Every kind of tests/observers_ref.kinds() at the partial sizes 3, 7 and 15 into a guarded tensor of exactly desc.bytes; the partial
    sizes also under the `sets` and `bitmap-E2` overrides (and the window / projection kernels); available_actions with both settings of
    walkable_lasers; env_outputs with each pointer alone and all together.  The observers write the caller's tensor ONLY: the whole arena
    holds, its output-only buffers poisoned."""
    import torch

    from lle_amd import _capi
    from tests import observers_ref
    from tests.test_gpu_observers_states import variant

    name = MAP_OF_G[g]
    n = sizes(g)[1]
    bw, fp = _world(ss.text_of(name), n, monkeypatch, dtype=dtype)
    A = bw.map.n_agents
    hold = ("obs", "reward", "events", "evcount", "err", "done")   # neither lle_batch_observe_as nor lle_batch_available_actions reads these
    row = bw.map.obs_stride * bw.obs_dtype.itemsize
    served = []
    for kname, kind, param in observers_ref.kinds(partial_sizes=(3, 7, 15)):
        d = bw.obs_desc(kind, param)
        if not d.supported:
            continue
        served.append(kname)
        mask = af.strided_payload_mask(d.bytes, [d.shape[q] for q in range(d.ndim)], [d.stride[q] for q in range(d.ndim)], d.elem_bytes)
        layered = kind in (_capi.LLE_OBS_LAYERED, _capi.LLE_OBS_LAYERED_PADDED, _capi.LLE_OBS_PERSPECTIVE)
        for var in (("rule", "sets", "bitmap-E2", "window", "project") if kind == _capi.LLE_OBS_PARTIAL else ("rule",)):
            out = Guarded(int(d.bytes), f"{kname} [{var}]", device=bw.device, row_bytes=row)
            with variant(monkeypatch, var):
                with fp.watch(RULES["observer"], poison=hold, extra=[out]):
                    bw.observe_as(kind, param, out=out.bytes)
            # the layered-style rows: "the first C*H*W bytes of a row are the reference's tensor, the rest is zero" (lle_hip.h lle_map_set_row_align)
            _assert_filled(out, mask, zero_pad=layered)
    assert {"layered", "perspective", "state", "normalized-state", "partial3", "partial7", "partial15"} <= set(served), served
    for walkable in (True, False):
        out = Guarded(n * A * 5, f"available_actions({walkable})", device=bw.device)
        with fp.watch(RULES["observer"], poison=hold, extra=[out]):
            bw.available_actions(walkable, out=out.tensor(torch.uint8, (n, A, 5)))
        _assert_filled(out)
    bw.step(sample=True, seed=21)   # (a plain step: `done` and `reward`, which env_outputs reads, hold real values again)
    keys = ["state", "reward", "done", "available", "alive", "arrived"]
    for wanted in [[k] for k in keys] + [keys]:
        guards, outs = _outputs(bw, multi=len(wanted) > 1)
        # (lle_batch_env_outputs READS LLE_BUF_DONE and LLE_BUF_REWARD, observers.hip:619-622: those two go through the diff alone here)
        with fp.watch(RULES["observer"], poison=("obs", "events", "evcount", "err"), extra=list(guards.values())):
            bw.env_outputs(multi_objective=len(wanted) > 1, walkable_lasers=len(wanted) == 1, **{k: outs[k] for k in wanted})
        for k, gk in guards.items():
            if k in wanted:
                _assert_filled(gk)
            else:   # a pointer that was not handed over: its tensor holds the pattern
                assert bool((gk.big == POISON).all()), f"env_outputs({wanted}) wrote `{k}`"
    bw.observe()


def test_policy_act_footprint(monkeypatch):
    """OptimalPolicy.act: "Nothing else of the env is written" (lle_amd/policy.py) -- a three-agent map, the whole rest of the caller's arena."""
    from lle_amd import policy
    from tests.parity_util import EXTRA_MAPS

    text = EXTRA_MAPS["q1"]
    bw, fp = _world(text, 21, monkeypatch, steps=0)
    assert bw.map.n_agents == 3
    for t in range(2):
        bw.step(sample=True, seed=3)
    pol = policy.OptimalPolicy(text, 8)
    with fp.watch(RULES["policy-act"], poison=("obs", "reward", "events", "evcount", "err", "done")):
        steps = pol.act(bw)
    assert tuple(steps.shape) == (21,)
    bw.observe()
    bw.step(bw.actions)
    assert int(bw.err.max()) == 0, "the policy's actions were refused"


def test_checker_is_not_vacuous_on_the_device(monkeypatch):
    """The device plumbing of the checker (offsets of the arena inside its allocation, the host copies): a real step judged by the row of
    `observe` is reported per buffer, a poisoned buffer the wrong row lets nobody write is reported by the poison, and a byte written (by
    torch, from the test) into either guard of the arena, and behind a guarded output, is reported as a guard byte."""
    bw, fp = _world(ss.text_of("long_three_words"), 69, monkeypatch)
    with pytest.raises(AssertionError) as ex:
        with fp.watch(RULES["observe"], poison=("obs", "reward")):
            bw.step(sample=True, auto_reset=True, seed=5)
    text = str(ex.value)
    assert "diff: observe changed" in text and "(actions, env " in text and "more (region, environment, kind) entries" in text and "poison: observe wrote (reward, env 0, payload)" in text
    bw.observe()
    for where in (fp.lo - 1, fp.lo + fp.nbytes):
        fp.big[where] = 0
        with pytest.raises(AssertionError, match="guard: 1 byte"):
            with fp.watch(RULES["observe"]):
                bw.observe()
        fp.big[where] = POISON
    out = Guarded(64, "an output", device=bw.device)
    out.big[out.lo + 64] = 1
    assert len(out.violations()) == 1 and "behind an output" in out.violations()[0]
    with fp.watch(RULES["observe"], poison=("obs", "done")):
        bw.observe()


def test_zz_every_kernel_ran_under_the_checker():
    """Behind the cases (this file's tests run in order): a step_kernel<G, LM, MODE, ML1, LX> of every MODE 0 to 9 and of every G in
    {1, 2, 4, 8, 16}, every (G, MODE) the cases were meant to launch, the world kernel, and the observer kernels that
    tests/test_gpu_observers_states.py names.  The module cannot shrink silently."""
    import re

    from lle_amd import _capi
    from tests.test_gpu_observers_states import PARTIAL_KERNELS

    launched = _capi.launched_kernels()
    steps = {(int(m.group(1)), int(m.group(2))) for m in (re.match(r"step_kernel<(\d+),\d+,(\d+),", k) for k in launched) if m}
    assert {mode for _g, mode in steps} >= set(range(10)), sorted(steps)
    assert {g for g, _mode in steps} >= {1, 2, 4, 8, 16}, sorted(steps)
    assert len(EXPECTED) >= 30 and EXPECTED <= steps, sorted(EXPECTED - steps)
    assert any(k.startswith("world_kernel<") for k in launched), launched
    assert all(any(k.startswith(p) for k in launched) for p in PARTIAL_KERNELS), launched
