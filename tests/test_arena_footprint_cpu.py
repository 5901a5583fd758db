"""tests/arena_footprint.py on a synthetic descriptor set and numpy byte arrays with PLANTED faults: the footprint net is not vacuous.

The synthetic arena follows lle_amd/csrc/capi.cpp make_layout (two table blobs, two init records, the 18 buffers of 7 environments with
an agent pitch of 4 for 3 agents and rows of 40 of 48 bytes -- plus one hidden environment, rounded up to 64 --, the per-environment reset
state, the EnvOutputs copy and the stats sum).  A clean masked reset passes; a byte in the guard in front of the arena and one behind it,
one in a record's pitch padding, one in an unmasked environment's row, one in `internal`, one in `req_pos`, one in a ring slot that was
not targeted and one write of an identical value into a poisoned region are each reported with region, environment and kind.  The refusal
to poison a buffer that launches read, the rules' citations and the exemption list are checked here too.  No GPU."""
import numpy as np
import pytest

from tests import arena_footprint as af

N, A, AS, L, ROW, PITCH, MAPS = 7, 3, 4, 2, 40, 48, 2
N_PAD = (N + 1 + 63) // 64 * 64


def synthetic_desc():
    """name -> (offset, bytes, shape, elem, stride), laid out like capi.cpp make_layout / lle_batch_get_buffer."""
    shapes = {
        "pos": (N_PAD * AS * 2, (N, A, 2), 1, (2 * AS, 2, 1)), "bits": (N_PAD * 8, (N,), 8, (1,)), "gems": (N_PAD * 4, (N,), 4, (1,)),
        "beams": (N_PAD * L * 4, (N, L), 4, (L, 1)), "avail": (N_PAD * AS, (N, A), 1, (AS, 1)), "actions": (N_PAD * AS, (N, A), 1, (AS, 1)),
        "err": (N_PAD, (N,), 1, (1,)), "evcount": (N_PAD, (N,), 1, (1,)), "events": (N_PAD * 2 * AS, (N, 2 * A), 1, (2 * AS, 1)),
        "done": (N_PAD, (N,), 1, (1,)), "obs": (N * PITCH, (N, ROW), 1, (PITCH, 1)), "stats": (4 * 64, (4, 8), 8, (8, 1)),
        "req_pos": (N_PAD * AS * 2, (N, A, 2), 1, (2 * AS, 2, 1)), "req_gems": (N_PAD * 4, (N,), 4, (1,)), "req_alive": (N_PAD * 2, (N,), 2, (1,)),
        "reward": (N_PAD * 4, (N, 4), 1, (4, 1)), "src_colour": (N_PAD * 4, (N, L), 1, (4, 1)), "src_enabled": (N_PAD * 4, (N,), 4, (1,)),
    }
    off = af._align(MAPS * 1024) + af._align(MAPS * af.INIT_RECORD_BYTES)
    desc = {}
    for name in af.BUFFERS:
        nbytes, shape, elem, stride = shapes[name]
        desc[name] = (off, nbytes, list(shape), elem, list(stride))
        off = af._align(off + nbytes)
    for k in af.STATE:
        off = af._align(off + shapes[k][0])
    return desc, off + 2 * af.ALIGN


DESC, NBYTES = synthetic_desc()
AMAP = af.ArenaMap(DESC, N, NBYTES, MAPS, dyn_lines=[True])
MASK = {1, 4}
RESET = af.RULES["reset"]


def arena():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, NBYTES).astype(np.uint8)
    r = AMAP.by_name["obs"]
    rows = a[r.off:r.off + N * PITCH].reshape(N, PITCH)
    rows[:, ROW:] = 0
    return a


def masked_reset(before):
    """What lle_batch_reset(mask) does to the bytes: state and results of the masked envs, the row of every env."""
    after = before.copy()
    for name in af.STATE + af.RESULT:
        r = AMAP.by_name[name]
        for e in MASK:
            after[r.off + e * r.pitch:r.off + (e + 1) * r.pitch] ^= 1   # (whole records: the pitch padding too)
    r = AMAP.by_name["obs"]
    rows = after[r.off:r.off + N * PITCH].reshape(N, PITCH)
    rows[:, :ROW] = 1
    rows[:, ROW:] = 0
    return after


def poisoned(before, names):
    af.check_poisonable(names)
    out = before.copy()
    for name in names:
        off, nbytes = AMAP.span(name)
        out[off:off + nbytes] = af.POISON
    return out


def report(before, after, rule, envs=None, maps=None, poison=()):
    bad, found = af.diff_violations(AMAP, before, after, rule, envs, maps)
    return bad + af.poison_violations(AMAP, after, rule, poison, envs), found


def test_layout_of_the_synthetic_arena():
    assert len(DESC) == 18 and AMAP.by_name["internal:stats_sum"].end == NBYTES
    assert AMAP.by_name["internal:tables"].pitch == 1024 and AMAP.by_name["internal:tables"].count == MAPS
    # every byte has exactly one class
    found = AMAP.classify(np.arange(NBYTES))
    assert sum(found.values()) == NBYTES
    r = AMAP.by_name["pos"]
    assert found[("pos", 0, "payload")] == 2 * A and found[("pos", 0, "padding")] == 2 * (AS - A) and found[("pos", N, "hidden")] == r.pitch
    assert found[("obs", 3, "payload")] == ROW and found[("obs", 3, "padding")] == PITCH - ROW
    assert found[("internal:tables", 1, "internal")] == 1024 and ("internal:gap", None, "internal") in found
    assert found[("internal:init_pos", 2, "internal")] == r.pitch


def test_a_clean_call_passes():
    before = poisoned(arena(), ("obs", "err", "evcount", "events", "done"))
    after = masked_reset(before)
    bad, found = report(before, after, RESET, MASK, poison=("obs",))
    assert bad == [], bad
    assert found[("obs", 0, "payload")] == ROW and ("pos", 1, "payload") in found and ("pos", 0, "payload") not in found
    # the guards around an untouched view hold
    g = af.Guarded(NBYTES, "the arena")
    assert g.lo >= af.MIN_GUARD and g.violations() == []


@pytest.mark.parametrize("side", ["front", "behind"])
def test_guard_byte_is_reported(side):
    g = af.Guarded(NBYTES, "the arena")
    g.big[g.lo - 1 if side == "front" else g.lo + NBYTES] = 0
    bad = g.violations()
    assert len(bad) == 1 and bad[0].startswith("guard:") and ("in front of the arena" if side == "front" else "behind the arena") in bad[0]
    assert ("nearest 1 byte(s) before" in bad[0]) if side == "front" else ("first 0 byte(s) past" in bad[0])


def plant(name, env, byte):
    r = AMAP.by_name[name]
    return r.off + env * r.pitch + byte


@pytest.mark.parametrize("what, rule, at, want", [
    ("pitch padding", af.RULES["observe"], ("avail", 2, A), "(avail, env 2, padding)"),
    ("row padding of a step without rows", af.step_rule(True, write_obs=False), ("obs", 5, ROW + 1), "(obs, env 5, padding)"),
    ("internal", af.RULES["step"], ("internal:tables", 1, 17), "(internal:tables, env 1, internal)"),
    ("reset state of an unmasked env", af.RULES["set_sources"], ("internal:init_beams", 0, 3), "(internal:init_beams, env 0, internal)"),
    ("req_pos", af.RULES["set_state"], ("req_pos", 3, 1), "(req_pos, env 3, payload)"),
    ("state of an unmasked env", RESET, ("bits", 0, 7), "(bits, env 0, payload)"),
    ("hidden env", af.RULES["step"], ("gems", N, 0), f"(gems, env {N}, hidden)"),
    ("a slot behind the hidden env", af.RULES["update_map"], ("gems", N + 1, 0), f"(gems, env {N + 1}, hidden)"),
    ("actions of a step that reads them", af.RULES["step"], ("actions", 6, 0), "(actions, env 6, payload)"),
    ("another map's tables", af.RULES["update_map-multi"], ("internal:tables", 0, 5), "(internal:tables, env 0, internal)"),
])
def test_planted_stray_byte_is_reported(what, rule, at, want):
    before = arena()
    after = masked_reset(before) if rule is RESET else before.copy()
    after[plant(*at)] ^= 0x40
    bad, _found = report(before, after, rule, MASK, maps={1})
    assert len(bad) == 1 and bad[0].startswith("diff:") and want in bad[0] and "1 byte(s)" in bad[0], (what, bad)


def test_unmasked_row_is_reported_under_a_rule_that_masks_rows():
    """No operation of the product masks the rows today (lle_batch_reset rebuilds every row: RULES["reset"]); a rule that does is checked."""
    rule = af.Rule("masked-rows", "synthetic", masked=("obs",), fills=("obs",))
    before = poisoned(arena(), ("obs",))
    after = before.copy()
    r = AMAP.by_name["obs"]
    for e in MASK:
        after[r.off + e * PITCH:r.off + e * PITCH + ROW] = 1
        after[r.off + e * PITCH + ROW:r.off + (e + 1) * PITCH] = 0
    assert report(before, after, rule, MASK, poison=("obs",))[0] == []
    after[plant("obs", 3, 9)] = 1
    bad, _ = report(before, after, rule, MASK, poison=("obs",))
    assert any(b.startswith("diff:") and "(obs, env 3, payload)" in b for b in bad) and any(b.startswith("poison:") and "(obs, env 3, payload)" in b for b in bad), bad


def test_static_line_of_an_incremental_step_is_reported():
    amap = af.ArenaMap(DESC, N, NBYTES, MAPS, dyn_lines=[False])   # (the one line of these rows declared static)
    rule = af.step_rule(True, incremental=True)
    before = arena()
    after = before.copy()
    after[plant("obs", 2, 4)] ^= 1
    bad, _ = af.diff_violations(amap, before, after, rule)
    assert len(bad) == 1 and "(obs, env 2, static)" in bad[0]
    assert af.diff_violations(AMAP, before, after, rule)[0] == []   # (dynamic line: allowed)


def test_identical_value_write_into_a_poisoned_region():
    """A stray write of the value that was there anyway: invisible to the diff of the plain arena, caught once the region is poisoned."""
    plain = arena()
    rule = af.step_rule(True, write_obs=False)
    assert report(plain, plain.copy(), rule)[0] == []                # the diff alone sees nothing
    before = poisoned(plain, ("obs", "reward"))
    after = before.copy()
    where = plant("obs", 4, 12)
    after[where] = plain[where]                                      # the kernel stores the byte the row held before
    for name in ("reward",):                                         # (what the step does write)
        off, nbytes = AMAP.span(name)
        after[off:off + nbytes] = 0
    bad = af.poison_violations(AMAP, after, rule, ("obs", "reward"))
    assert len(bad) == 1 and bad[0].startswith("poison:") and "(obs, env 4, payload) at byte 12" in bad[0], bad


def test_unwritten_output_and_dirty_padding_are_reported():
    before = poisoned(arena(), ("obs", "done"))
    after = masked_reset(before)
    r = AMAP.by_name["obs"]
    after[r.off + 2 * PITCH + 3] = af.POISON          # a byte of row 2 the launch did not write
    after[r.off + 6 * PITCH + ROW] = 1                # padding of row 6 not zero
    bad = af.poison_violations(AMAP, after, RESET, ("obs", "done"), MASK)
    assert any("left 1 byte(s) of `obs` unwritten, first (env 2, byte 3)" in b for b in bad) and any("row padding of env 6 is not zero" in b for b in bad), bad
    assert not any("`done`" in b for b in bad)        # (masked envs written, the others still poisoned)


def test_ring_slot_that_was_not_targeted():
    slots, n, rec = 4, N, 16
    ring = np.full(slots * n * rec, af.POISON, np.uint8)
    rows = ring.reshape(slots, n, rec)
    rows[[3, 0, 1]] = 0                               # ring_pos 3, three steps: slots 3, 0, 1
    assert af.ring_violations(ring, slots, {3, 0, 1}, "the reward ring", record=rec) == []
    rows[2, 5, 7] = 0
    bad = af.ring_violations(ring, slots, {3, 0, 1}, "the reward ring", record=rec)
    assert len(bad) == 1 and "slot 2 of the reward ring" in bad[0] and "first at byte 87" in bad[0]
    rows[2, 5, 7] = af.POISON
    rows[0, 1, 2] = af.POISON
    bad = af.ring_violations(ring, slots, {3, 0, 1}, "the reward ring", record=rec)
    assert len(bad) == 1 and "slot 0" in bad[0] and "(env 1, byte 2)" in bad[0]


def test_refuses_to_poison_what_a_launch_reads():
    for name in af.BUFFERS:
        if name in af.POISONABLE:
            af.check_poisonable([name])
        else:
            with pytest.raises(AssertionError, match="refusing to poison"):
                af.check_poisonable([name])
    assert set(af.POISONABLE) == {"obs", "reward", "events", "evcount", "err", "actions", "done"}
    with pytest.raises(AssertionError, match="refusing to poison"):
        af.check_poisonable(["internal:tables"])


def test_rules_cite_the_code_and_exemptions_stay_inside():
    for name, rule in af.RULES.items():
        assert rule.name == name and any(src in rule.cite for src in ("capi.cpp", "kernels.hip", "step_kernel.hpp", "policy.py")), name
        assert all(k.startswith("internal:") and k in AMAP.by_name for k in rule.internal), name
    # no exemption covers a payload byte or a buffer the operation does not own
    for buf, kind, why in af.EXEMPTIONS:
        assert kind == "padding" and buf in af.BUFFERS and why
        key = (buf, 0, "padding")
        owner = af.RULES["step+actions"] if buf == "actions" else af.RULES["reset_sources"]
        assert AMAP.allowed(owner, key, {0}) and not AMAP.allowed(af.RULES["observe"], key, {0}) and not AMAP.allowed(af.RULES["stats"], key, {0})
        assert not AMAP.allowed(owner, (buf, N, "hidden"), {0}) and (buf == "actions" or not AMAP.allowed(owner, key, {1}))   # (nor another env's)
    assert not AMAP.allowed(af.RULES["step"], ("bits", 0, "padding")) and not AMAP.allowed(af.RULES["step"], ("internal:gap", None, "internal"))
    # the header's contracts as the rows state them
    assert "obs" not in af.step_rule(True, write_obs=False).writes and "obs" not in af.step_rule(True, partial=True).writes
    assert "actions" not in af.RULES["step"].writes and "actions" in af.step_rule(True).writes
    ring = af.step_rule(True, ring=True)
    assert not {"obs", "reward", "actions"} & set(ring.writes)
    assert not any(b.startswith("req_") for r in af.RULES.values() for b in r.writes)


def test_strided_payload_mask():
    m = af.strided_payload_mask(2 * 3 * 8 * 2, (2, 3, 5), (24, 8, 1), 2)   # 2 envs x 3 observers, rows of 5 of 8 fp16
    assert m.sum() == 2 * 3 * 5 * 2 and m[:10].all() and not m[10:16].any() and m[16:26].all()
