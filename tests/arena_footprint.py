"""The write footprint of a launch, byte by byte: which bytes of a batch's arena, and of the caller's tensors, did a call change?

Every other suite asks whether the buffers a call names hold what the oracle says.  This helper asks the opposite question -- did the call
write anything ELSE -- with three detectors that work together around any call:

* guards   the arena, and every ring / output / input tensor of the caller, is a view into the middle of a larger uint8 allocation filled
           with POISON (at least 64 KiB and four observation rows on each side): every guard byte still holds the pattern afterwards;
* diff     the whole arena is copied before the call and compared behind it; every changed byte is classified (`ArenaMap.classify`:
           region, environment, payload / padding / hidden / internal) and must fall inside what the RULES row of the call allows;
* poison   output-only memory (POISONABLE; `check_poisonable` refuses anything else: a poisoned position or beam word would index the
           tables out of bounds) is filled with POISON before the call.  What the call must leave alone still holds the pattern -- a write
           of IDENTICAL values, which the diff cannot see, shows up here --, and what the call must write holds no POISON byte any more.

Plain numpy on host copies (torch only moves the bytes); nothing here knows the oracle.  The detection code is the same for the synthetic
arrays of tests/test_arena_footprint_cpu.py and for the device arena of tests/test_gpu_arena_footprint.py.

The regions come from the batch's 19 LLE_BUF_* descriptors; every arena byte no descriptor covers is `internal`, and the helper names
those parts from lle_amd/csrc/capi.cpp make_layout (lines 81-133): the table blobs and the init records in front of the buffers, behind
them the per-environment reset state (five arrays shaped like pos, bits, gems, beams, avail), the 64-byte EnvOutputs copy and the 64-byte
stats sum, each rounded up to 256 bytes."""
import numpy as np

POISON = 0xA5           # no value any kernel stores: observations are -1 / 0 / 1 in int8 / fp16 / bf16 / fp32, codes and counts are small
MIN_GUARD = 64 * 1024
ALIGN = 256             # capi.cpp:64
INIT_RECORD_BYTES = 192  # sizeof(InitRecord), tables.h:362-368 (16 x u16, u64, u32, 32 x u32, 16 x u8 = 188, aligned to 8)

BUFFERS = ("pos", "bits", "gems", "beams", "avail", "actions", "err", "evcount", "events", "done", "obs", "stats", "req_pos", "req_gems",
           "req_alive", "reward", "src_colour", "src_enabled")
STATE = ("pos", "bits", "gems", "beams", "avail")
RESULT = ("err", "evcount", "events", "done")
ENV_INIT = tuple("internal:init_" + k for k in STATE)   # capi.cpp:122-126: the reset state of every env (per-environment sources)

# Memory a launch never READS (given the condition behind each name): the only regions the poison detector may fill.  Everything else --
# pos, bits, gems, beams, avail, src_*, req_*, stats (flush_stats adds to its slot, kernel_common.hpp:50-53), internal -- is an input of
# some kernel and goes through the diff alone.
POISONABLE = {
    "obs": "the rows are written, never read (the incremental writer skips the static lines, it does not read them)",
    "reward": "output of the step (not around lle_batch_env_outputs, which reads it: observers.hip:622)",
    "events": "output of step / reset / set_state",
    "evcount": "output of step / reset / set_state",
    "err": "output of step / reset / set_state / set_sources",
    "actions": "only when the call samples or takes actions_dev",
    "done": "only without auto_reset (lle_hip.h ties LLE_STEP_AUTO_RESET to what LLE_BUF_DONE says), and not around lle_batch_env_outputs (observers.hip:619)",
}


def check_poisonable(names):
    """The hard rule: never poison anything a launch reads."""
    for name in names:
        assert name in POISONABLE, f"refusing to poison `{name}`: a launch reads it (only {sorted(POISONABLE)} are output-only)"


# ---------------------------------------------------------------------------------------------- exemptions
# Bytes INSIDE a buffer the operation owns whose content no contract fixes.  None covers a payload byte, none reaches outside the buffer.
EXEMPTIONS = (
    ("pos", "padding", "agent-pitch slots at or beyond A: the world kernel stores whole records of AM agents (kernel_common.hpp:61-65, off-grid sentinels kernels.hip:131)"),
    ("avail", "padding", "agent-pitch slots at or beyond A: store_u8_record<AM> (kernel_common.hpp:77-82)"),
    ("actions", "padding", "agent-pitch slots at or beyond A: store_u8_record<AM> of the sampled / given actions (kernels.hip:189,198)"),
    ("events", "padding", "entries at or beyond 2A: the step kernel stores 2G >= 2A event bytes (step_kernel.hpp:595-602), the world kernel 2AM (kernels.hip:368-370)"),
    ("src_colour", "padding", "colour words at or beyond L: whole 32-bit colour words are stored (kernels.hip:326-327, step_kernel.hpp:547)"),
)
_EXEMPT = {(b, k) for b, k, _why in EXEMPTIONS}
assert all(k == "padding" for _b, k, _w in EXEMPTIONS), "no exemption may cover payload bytes"


# ---------------------------------------------------------------------------------------------- the rules table
class Rule:
    """What one operation may change.  `writes` / `internal`: region -> "all" | "masked" | "map" (the environments / the map the call names);
    `fills`: the buffers it writes IN FULL for those environments (after the call no POISON byte is left there); `hidden`: it may rewrite
    the hidden environment (slot n_envs) the reset state is computed on; `obs_lines`: "all", or "dynamic" for the incremental writer."""

    def __init__(self, name, cite, writes=(), masked=(), fills=(), internal=None, hidden=False, obs_lines="all"):
        self.name, self.cite, self.hidden, self.obs_lines = name, cite, hidden, obs_lines
        self.writes = {b: "all" for b in writes}
        self.writes.update({b: "masked" for b in masked})
        self.fills = tuple(fills)
        self.internal = dict(internal or {})
        assert all(b in BUFFERS for b in self.writes) and all(b in self.writes for b in self.fills), name

    def but(self, name, drop=(), add=(), add_masked=(), fills=None, internal=None, obs_lines=None, cite=None):
        r = Rule(name, self.cite + ("; " + cite if cite else ""), hidden=self.hidden, obs_lines=obs_lines or self.obs_lines)
        r.writes = {b: s for b, s in self.writes.items() if b not in drop}
        r.writes.update({b: "all" for b in add})
        r.writes.update({b: "masked" for b in add_masked})
        r.fills = tuple(b for b in (self.fills if fills is None else fills) if b in r.writes)
        r.internal = dict(self.internal)
        r.internal.update(internal or {})
        return r


_STEP = Rule(
    "step", "step_kernel.hpp:591-613 (err, evcount, events, done, reward: every env, a refused one too), :769-785 (the row of every env of the "
    "wavefront, refused or not), :791-808 (state, unconditionally), :820 + kernel_common.hpp:41-55 (the wavefront's stats slot); lane-per-env "
    "step: kernels.hip:355-372,402,422.  Header row corrected: a REFUSED env keeps its state (same bytes rewritten) but its row, events, "
    "evcount, done and reward ARE written",
    writes=STATE + RESULT + ("reward", "stats", "obs"), fills=RESULT + ("reward", "obs"))
_WORLD_MASKED = STATE + RESULT

RULES = {
    # lle_batch_step without actions_dev and without sampling reads LLE_BUF_ACTIONS where it is (step_kernel.hpp:558-560)
    "step": _STEP,
    # sampled (step_kernel.hpp:557) or handed over (step_kernel.hpp:560; kernels.hip:189,198): LLE_BUF_ACTIONS is written
    "step+actions": _STEP.but("step+actions", add=("actions",), fills=_STEP.fills + ("actions",), cite="step_kernel.hpp:557,560"),
    # LLE_STEP_RECOLOUR_RESETS: the fresh colours and the env's reset beams (step_kernel.hpp:541,547)
    "step+recolour": _STEP.but("step+recolour", add=("actions", "src_colour"), fills=_STEP.fills + ("actions",),
                               internal={"internal:init_beams": "all"}, cite="step_kernel.hpp:541,547"),
    # a ring takes obs / actions / reward of every step (step_kernel.hpp:474-483): the batch's own stay
    "rollout-ring": _STEP.but("rollout-ring", drop=("obs", "reward"), cite="step_kernel.hpp:474-483"),
    # lle_batch_reset: kernels.hip:225-235 (masked envs), :355-372 (state and results of the touched envs only), :410-419 -- the row of EVERY env
    # of the launch is rebuilt from its current state, masked or not.  Header row corrected (the header now says so): an unmasked env
    # keeps every byte of its state and results; its row is rewritten with its own observation.
    "reset": Rule("reset", "kernels.hip:225-235,355-372,410-419", writes=("obs",), masked=_WORLD_MASKED, fills=("obs",) + RESULT),
    # lle_batch_set_sources / _reset_sources (after the first call): kernels.hip:267-347 -- colours, flags, the env's reset state, err, done,
    # the state (beams follow enable / disable); with reset_first also avail, evcount, events (kernels.hip:272-281,364-372); rows: every env
    "set_sources": Rule("set_sources", "kernels.hip:267-347,355-362,410-419", writes=("obs",),
                        masked=("pos", "bits", "gems", "beams", "err", "done", "src_colour", "src_enabled"), fills=("obs",),
                        internal={k: "masked" for k in ENV_INIT}),
    "reset_sources": Rule("reset_sources", "kernels.hip:267-347,355-372,410-419", writes=("obs",),
                          masked=_WORLD_MASKED + ("src_colour", "src_enabled"), fills=("obs",) + RESULT, internal={k: "masked" for k in ENV_INIT}),
    # lle_batch_set_state: kernels.hip:236-256 (reads req_*), :355-372, :410-419
    "set_state": Rule("set_state", "kernels.hip:236-256,355-372,410-419", writes=STATE + RESULT + ("obs",), fills=RESULT + ("obs",)),
    # lle_batch_observe: the rows AND `done`, a function of the state (kernels.hip:351).  Header row corrected: not `obs` alone.
    "observe": Rule("observe", "kernels.hip:348-352,410-419", writes=("obs", "done"), fills=("obs", "done")),
    # lle_batch_update_sources / _update_map of a one-map batch with the map's sources: capi.cpp:1261 (the map's blob), :1269 + :542-563 (the hidden
    # env is reset and copied into the map's init record), :1278 -> KMODE_SOURCES: kernels.hip:257-266,355-362 (state, beams follow the flags), rows
    "update_map": Rule("update_map", "capi.cpp:1261-1278,542-563; kernels.hip:257-266,355-362,410-419", writes=("pos", "bits", "gems", "beams", "obs"),
                       fills=("obs",), internal={"internal:tables": "map", "internal:init_records": "all"}, hidden=True),
    # ... of a batch of several maps: KMODE_OBSERVE (capi.cpp:1278): rows and done; every map's init record is refreshed (capi.cpp:545)
    "update_map-multi": Rule("update_map-multi", "capi.cpp:1261-1278,542-563; kernels.hip:348-352", writes=("obs", "done"), fills=("obs", "done"),
                             internal={"internal:tables": "map", "internal:init_records": "all"}, hidden=True),
    # ... with per-environment sources: KMODE_ENV_SOURCES over every env (capi.cpp:1271-1275)
    "update_map-per-env": Rule("update_map-per-env", "capi.cpp:1261-1275,542-563; kernels.hip:267-347",
                               writes=("pos", "bits", "gems", "beams", "err", "done", "src_colour", "src_enabled", "obs"), fills=("obs",),
                               internal=dict({k: "all" for k in ENV_INIT}, **{"internal:tables": "map", "internal:init_records": "all"}), hidden=True),
    # the observers write the caller's tensor only: views and window tables live in allocations of their own (capi.cpp:740,1059), the EnvOutputs
    # struct rides in the kernel arguments (capi.cpp:885-887).  One exception, in the row: LLE_OBS_LAYERED with per-environment sources runs the
    # world kernel's OBSERVE mode on the caller's buffer, which also stores `done` (capi.cpp:1079-1090, kernels.hip:351)
    "observer": Rule("observer", "capi.cpp:1073-1214"),
    "observer-layered-per-env": Rule("observer-layered-per-env", "capi.cpp:1079-1090; kernels.hip:351", writes=("done",)),
    # lle_batch_stats: the sum slot, and the memset of the slots with reset_counters (capi.cpp:216-222,1303-1311)
    "stats": Rule("stats", "capi.cpp:216-222,1303-1311", writes=("stats",), internal={"internal:stats_sum": "all"}),
    # lle_batch_snapshot copies OUT of the arena (capi.cpp:803-816)
    "snapshot": Rule("snapshot", "capi.cpp:803-816"),
    # lle_batch_restore: [pos, actions) in one copy, hidden env included (capi.cpp:826), then KMODE_OBSERVE (capi.cpp:835): rows and done
    "restore": Rule("restore", "capi.cpp:817-836", writes=STATE + ("obs", "done"), fills=("obs", "done"), hidden=True),
    # ... with per-environment sources also [src_colour, EnvOutputs copy) (capi.cpp:829) and KMODE_ENV_SOURCES over every env
    "restore-per-env": Rule("restore-per-env", "capi.cpp:817-836; kernels.hip:267-347", writes=STATE + ("obs", "done", "err", "src_colour", "src_enabled"),
                            fills=("obs",), internal={k: "all" for k in ENV_INIT}, hidden=True),
    # OptimalPolicy.act: "Nothing else of the env is written" (lle_amd/policy.py:256-262)
    "policy-act": Rule("policy-act", "lle_amd/policy.py:256-262", writes=("actions",)),
    # lle_batch_autotune: sampled steps with auto-reset, the counters zeroed, World.reset of every env (capi.cpp:1385-1497)
    "autotune": _STEP.but("autotune", add=("actions",), cite="capi.cpp:1385-1497"),
}


def step_rule(actions_written, write_obs=True, incremental=False, partial=False, recolour=False, ring=False):
    """The RULES row of one step launch.  LLE_STEP_NO_OBS (step_kernel.hpp:769 `write_obs`) and the partial observation "instead of" the
    layered one (lle_hip.h lle_env_outputs.partial; step_kernel.hpp:763-768) leave every byte of `obs` alone; LLE_STEP_INCREMENTAL_OBS writes
    only the lines lle_map_row_dynamic_lines names (lle_hip.h LLE_STEP_INCREMENTAL_OBS)."""
    r = RULES["rollout-ring" if ring else "step+recolour" if recolour else "step+actions" if actions_written else "step"]
    if not ring and (not write_obs or partial):
        r = r.but(r.name + "-no-obs", drop=("obs",), cite="step_kernel.hpp:763-769")
    elif incremental and not ring:
        r = r.but(r.name + "-incremental", obs_lines="dynamic", cite="lle_hip.h LLE_STEP_INCREMENTAL_OBS")
    return r


# ---------------------------------------------------------------------------------------------- regions
class Region:
    def __init__(self, name, off, nbytes, pitch, payload, count, internal=False):
        self.name, self.off, self.nbytes, self.pitch, self.payload, self.count, self.internal = name, int(off), int(nbytes), int(pitch), int(payload), int(count), internal

    @property
    def end(self):
        return self.off + self.nbytes


def _align(x):
    return (x + ALIGN - 1) // ALIGN * ALIGN


class ArenaMap:
    """Every byte of an arena by region.  `desc`: BatchedWorld._desc -- name -> (arena_offset, bytes, shape, elem_bytes, stride in elements)."""

    def __init__(self, desc, n_envs, arena_bytes, n_maps=1, dyn_lines=None):
        self.n, self.nbytes, self.n_maps = int(n_envs), int(arena_bytes), int(n_maps)
        self.dyn_lines = None if dyn_lines is None else np.asarray(dyn_lines, bool)
        regions = []
        for name in BUFFERS:
            off, nbytes, shape, elem, stride = desc[name]
            pitch = int(stride[0]) * int(elem)
            payload = int(np.prod(shape[1:], dtype=np.int64)) * int(elem) if len(shape) > 1 else int(elem)
            assert payload <= pitch or pitch == 0, name
            count = self.n if name != "stats" else int(shape[0])
            assert count * pitch <= nbytes, name
            regions.append(Region(name, off, nbytes, pitch, payload, count))
        regions.sort(key=lambda r: r.off)
        assert all(a.end <= b.off for a, b in zip(regions, regions[1:])), "descriptors overlap"
        self.by_name = {r.name: r for r in regions}
        # in front of the buffers: n_maps table blobs of one stride, then n_maps init records (capi.cpp:111-116)
        first = regions[0].off
        rec = _align(self.n_maps * INIT_RECORD_BYTES)
        assert first % ALIGN == 0 and first >= rec
        internal = []
        if first - rec > 0:
            assert (first - rec) % self.n_maps == 0
            internal.append(Region("internal:tables", 0, first - rec, (first - rec) // self.n_maps, (first - rec) // self.n_maps, self.n_maps, True))
        internal.append(Region("internal:init_records", first - rec, rec, INIT_RECORD_BYTES, INIT_RECORD_BYTES, self.n_maps, True))
        # behind them: the per-environment reset state, the EnvOutputs copy, the stats sum (capi.cpp:122-131)
        off = _align(regions[-1].end)
        for k in STATE:
            src = self.by_name[k]
            internal.append(Region("internal:init_" + k, off, src.nbytes, src.pitch, src.payload, self.n, True))
            off = _align(off + src.nbytes)
        internal.append(Region("internal:env_out", off, ALIGN, 0, 0, 0, True))
        internal.append(Region("internal:stats_sum", off + ALIGN, ALIGN, 0, 0, 0, True))
        assert off + 2 * ALIGN == self.nbytes, f"the arena does not end where capi.cpp make_layout says: {off + 2 * ALIGN} != {self.nbytes}"
        self.regions = sorted(regions + internal, key=lambda r: r.off)
        self.by_name.update({r.name: r for r in internal})

    def span(self, name, envs=None):
        """(offset, bytes) of the first n environments of a buffer (never the hidden environment behind them)."""
        r = self.by_name[name]
        return r.off, r.count * r.pitch

    def classify(self, offsets):
        """{(region, environment or None, kind): count} of the given arena byte offsets.  kind: payload | padding (pitch padding; for `obs` the
        row padding) | static (a line of `obs` the incremental writer must not touch; only with dyn_lines) | hidden (an environment slot at or
        beyond n_envs) | internal (no descriptor covers it)."""
        offsets = np.asarray(offsets, np.int64)
        out = {}
        if offsets.size == 0:
            return out
        assert offsets.min() >= 0 and offsets.max() < self.nbytes
        offsets = np.sort(offsets)
        taken = 0
        for r in self.regions:
            lo, hi = np.searchsorted(offsets, [r.off, r.end])
            if lo == hi:
                continue
            taken += int(hi - lo)
            rel = offsets[lo:hi] - r.off
            if r.pitch == 0:
                out[(r.name, None, "internal" if r.internal else "padding")] = int(rel.size)
                continue
            idx, within = rel // r.pitch, rel % r.pitch
            kind = np.where(within < r.payload, 0, 1)                       # payload / padding
            if r.name == "obs" and self.dyn_lines is not None:
                static = ~self.dyn_lines[np.minimum(within // 128, self.dyn_lines.size - 1)]
                kind = np.where(static, 2, kind)
            kind = np.where(idx >= r.count, 3, kind)                        # hidden
            names = ("payload", "padding", "static", "hidden")
            counts = np.bincount(idx * 4 + kind)
            for code in np.flatnonzero(counts):
                i, label = int(code) // 4, names[int(code) % 4]
                if r.internal and label in ("payload", "padding"):
                    label = "internal"
                key = (r.name, None if r.name == "stats" else i, label)
                out[key] = out.get(key, 0) + int(counts[code])
        rest = int(offsets.size - taken)
        if rest:
            out[("internal:gap", None, "internal")] = rest     # alignment gaps between two regions
        return out

    # ---- what a rule allows
    def allowed(self, rule, key, envs=None, maps=None):
        name, idx, kind = key
        if kind == "hidden":   # the hidden environment (slot n): refresh_init_record resets it (capi.cpp:542-563), restore copies over it
            return rule.hidden and idx == self.n and (name in STATE + RESULT or name in rule.writes or name in rule.internal)
        scope = rule.internal.get(name) if name.startswith("internal:") else rule.writes.get(name)
        if scope is None:
            return False
        if kind == "static":
            return rule.obs_lines != "dynamic"
        if kind == "padding" and name != "obs" and (name, kind) not in _EXEMPT:   # (obs: the row padding is written, as zeros -- DESIGN section 2)
            return False
        if scope == "masked":
            return envs is not None and idx in envs
        if scope == "map":
            return maps is not None and idx in maps
        return True


# ---------------------------------------------------------------------------------------------- the detectors, on host bytes
def guard_violations(host, lo, nbytes, what):
    """`host`: the whole allocation as numpy uint8; the watched view is host[lo : lo + nbytes].  Offsets are relative to the view."""
    bad = []
    before = np.flatnonzero(host[:lo] != POISON)
    behind = np.flatnonzero(host[lo + nbytes:] != POISON)
    if before.size:
        bad.append(f"guard: {before.size} byte(s) in front of {what} written, nearest {int(lo - before[-1])} byte(s) before its start")
    if behind.size:
        bad.append(f"guard: {behind.size} byte(s) behind {what} written, first {int(behind[0])} byte(s) past its end")
    return bad


def diff_violations(amap, before, after, rule, envs=None, maps=None):
    """The changed bytes of the arena that the rule does not allow, one line per (region, environment, kind)."""
    changed = np.flatnonzero(before != after)
    found = amap.classify(changed)
    return [f"diff: {rule.name} changed {c} byte(s) of ({name}, env {idx}, {kind})" for (name, idx, kind), c in sorted(found.items(), key=str)
            if not amap.allowed(rule, (name, idx, kind), envs, maps)], found


def poison_violations(amap, after, rule, poisoned, envs=None):
    """`poisoned`: names of the buffers filled with POISON before the call (all n environments, pitch padding included).  What the rule does
    not allow to be written still holds the pattern; what the rule fills holds none of it (for `obs`: padding included, and the padding is zero)."""
    bad = []
    for name in poisoned:
        r = amap.by_name[name]
        rows = after[r.off:r.off + r.count * r.pitch].reshape(r.count, r.pitch)
        scope = rule.writes.get(name)
        inside = np.zeros(r.count, bool)
        if scope == "all":
            inside[:] = True
        elif scope == "masked" and envs:
            inside[sorted(envs)] = True
        cols = np.ones(r.pitch, bool)
        if name == "obs" and rule.obs_lines == "dynamic" and scope is not None:
            cols = np.repeat(amap.dyn_lines, 128)[:r.pitch]
        must_stay = np.ones((r.count, r.pitch), bool)
        must_stay[np.ix_(inside, cols)] = False
        for e, c in zip(*np.nonzero(must_stay & (rows != POISON))):
            kind = "payload" if c < r.payload else "padding"
            if inside[e] and name != "obs" and kind == "padding" and (name, kind) in _EXEMPT:
                continue
            kind = "static" if (name == "obs" and inside[e]) else kind
            bad.append(f"poison: {rule.name} wrote ({name}, env {int(e)}, {kind}) at byte {int(c)} of the record, which it must leave alone")
            if len(bad) > 20:
                return bad
        if name in rule.fills:
            width = r.pitch if name == "obs" else r.payload
            full = np.zeros((r.count, r.pitch), bool)
            full[np.ix_(inside, cols & (np.arange(r.pitch) < width))] = True
            left = np.nonzero(full & (rows == POISON))
            if left[0].size:
                bad.append(f"poison: {rule.name} left {left[0].size} byte(s) of `{name}` unwritten, first (env {int(left[0][0])}, byte {int(left[1][0])})")
            if name == "obs":
                pad = np.zeros((r.count, r.pitch), bool)
                pad[np.ix_(inside, cols & (np.arange(r.pitch) >= r.payload))] = True
                if (rows[pad] != 0).any():
                    e = int(np.nonzero(pad & (rows != 0))[0][0])
                    bad.append(f"poison: {rule.name}: the row padding of env {e} is not zero")
    return bad


def ring_violations(ring_bytes, slots, targeted, what, record=0, payload=0, written=True):
    """`ring_bytes`: the host bytes of a trajectory ring of `slots` equal slots that held POISON before the launch.  A slot outside `targeted`
    still holds the pattern everywhere; with `written`, a targeted slot holds none in the first `payload` bytes of each `record`."""
    rows = np.asarray(ring_bytes).reshape(slots, -1)
    bad = []
    for s in range(slots):
        if s not in targeted:
            hit = np.flatnonzero(rows[s] != POISON)
            if hit.size:
                bad.append(f"ring: {hit.size} byte(s) of slot {s} of {what} written (first at byte {int(hit[0])}); the launch targets slots {sorted(targeted)}")
        elif written and record:
            rec = rows[s].reshape(-1, record)[:, :payload or record]
            left = np.nonzero(rec == POISON)
            if left[0].size:
                bad.append(f"ring: slot {s} of {what}: {left[0].size} byte(s) left unwritten, first (env {int(left[0][0])}, byte {int(left[1][0])})")
    return bad


def strided_payload_mask(nbytes, shape, stride, elem):
    """Bool per byte of an output described by shape / strides in elements (lle_obs_desc): does it belong to an element of the tensor?"""
    idx = np.zeros(tuple(int(s) for s in shape), np.int64)
    for ax, (s, st) in enumerate(zip(shape, stride)):
        sh = [1] * len(shape)
        sh[ax] = int(s)
        idx = idx + (np.arange(int(s), dtype=np.int64) * int(st)).reshape(sh)
    mask = np.zeros(int(nbytes), bool)
    first = idx.reshape(-1) * int(elem)
    for b in range(int(elem)):
        mask[first + b] = True
    return mask


# ---------------------------------------------------------------------------------------------- torch side: guarded memory
class Guarded:
    """A contiguous view of `nbytes` bytes in the middle of a POISON-filled uint8 allocation (a torch device tensor, or a numpy array when
    `device` is None), 256-byte aligned, with `guard` bytes on each side."""

    def __init__(self, nbytes, what, device=None, row_bytes=0):
        self.nbytes, self.what = int(nbytes), what
        g = _align(max(MIN_GUARD, 4 * int(row_bytes)))
        if device is None:
            self.big = np.full(g + self.nbytes + ALIGN + g, POISON, np.uint8)
            self.lo = g
        else:
            import torch
            self.big = torch.full((g + self.nbytes + ALIGN + g,), POISON, dtype=torch.uint8, device=device)
            self.lo = g + (-(self.big.data_ptr() + g)) % ALIGN
        self.guard = g
        self.bytes = self.big[self.lo:self.lo + self.nbytes]

    def tensor(self, dtype, shape):
        return self.bytes.view(dtype).view(*shape)

    def host(self):
        return self.big if isinstance(self.big, np.ndarray) else self.big.cpu().numpy()

    def violations(self, host=None):
        return guard_violations(self.host() if host is None else host, self.lo, self.nbytes, self.what)


def guarded_world(*args, **kwargs):
    """(BatchedWorld, Footprint): a batch whose arena is the middle of a POISON-filled allocation (BatchedWorld._alloc_arena overridden)."""
    import torch

    from lle_amd import BatchedWorld

    class GuardedWorld(BatchedWorld):
        def _alloc_arena(self, nbytes):
            row = int(self.map.obs_stride) * self.obs_dtype.itemsize
            g = _align(max(MIN_GUARD, 4 * row))
            self.big = torch.full((g + nbytes + ALIGN + g,), POISON, dtype=torch.uint8, device=self.device)
            return self.big[g:g + nbytes + ALIGN]

    bw = GuardedWorld(*args, **kwargs)
    return bw, Footprint(bw, bw.big)


class Footprint:
    """The three detectors around calls on one BatchedWorld whose arena lies in guarded memory (`bw.big`: the POISON-filled allocation,
    `bw._base` the arena inside it).  Usage:

        with fp.watch(rule, envs=None, maps=None, poison=("obs", "reward"), extra=[Guarded, ...]):
            bw.step(...)

    raises AssertionError with every violation found; `fp.found` keeps the classified diff of the last call."""

    def __init__(self, bw, big):
        self.bw, self.big = bw, big
        self.lo = bw._base.data_ptr() - big.data_ptr()
        self.nbytes = int(bw._base.numel())
        assert 0 < self.lo and self.lo + self.nbytes < big.numel()
        row = int(bw.map.obs_stride) * bw.obs_dtype.itemsize
        assert min(self.lo, big.numel() - self.lo - self.nbytes) >= max(MIN_GUARD, 4 * row), "guards of at least 64 KiB and four observation rows"
        dyn = None
        if bw.obs_dtype.itemsize == 1 and len(bw.maps) == 1:
            dyn = bw.map.row_dynamic_lines
        self.amap = ArenaMap(bw._desc, bw.n_envs, self.nbytes, len(bw.maps), dyn)
        self.found = {}

    def poison(self, names):
        check_poisonable(names)
        for name in names:
            off, nbytes = self.amap.span(name)
            self.bw._base[off:off + nbytes].fill_(POISON)

    def watch(self, rule, envs=None, maps=None, poison=(), extra=(), bulk=False):
        """bulk: for arenas of hundreds of megabytes -- guards and diff on the device; the bytes of the first n environments of a buffer the
        rule lets every environment write are counted as (name, None, "bulk") and not enumerated; no poison."""
        return _Watch(self, rule, envs, maps, tuple(poison), tuple(extra), bulk)


class _Watch:
    def __init__(self, fp, rule, envs, maps, poison, extra, bulk=False):
        self.fp, self.rule, self.poison, self.extra, self.bulk = fp, rule, poison, extra, bulk
        self.envs = None if envs is None else {int(e) for e in envs}
        self.maps = None if maps is None else {int(m) for m in maps}
        assert not (bulk and poison)

    def __enter__(self):
        import torch
        fp = self.fp
        fp.poison(self.poison)
        torch.cuda.synchronize(fp.bw.device)
        self.before = fp.bw._base.clone() if self.bulk else fp.bw._base.cpu().numpy()
        return self

    def _exit_bulk(self):
        import torch
        fp, rule = self.fp, self.rule
        bad = []
        if bool((fp.big[:fp.lo] != POISON).any()) or bool((fp.big[fp.lo + fp.nbytes:] != POISON).any()):
            bad += guard_violations(fp.big.cpu().numpy(), fp.lo, fp.nbytes, "the arena")
        neq = self.before != fp.bw._base
        found = {}
        for name, scope in rule.writes.items():
            if scope == "all" and not (name == "obs" and rule.obs_lines != "all"):
                off, nbytes = fp.amap.span(name)
                c = int(neq[off:off + nbytes].sum())
                if c:
                    found[(name, None, "bulk")] = c
                neq[off:off + nbytes] = False
        rest = fp.amap.classify(torch.nonzero(neq).view(-1).cpu().numpy())
        bad += [f"diff: {rule.name} changed {c} byte(s) of ({name}, env {idx}, {kind})" for (name, idx, kind), c in sorted(rest.items(), key=str)
                if not fp.amap.allowed(rule, (name, idx, kind), self.envs, self.maps)]
        found.update(rest)
        fp.found = found
        assert not bad, f"{rule.name} [{rule.cite}]:\n  " + "\n  ".join(bad[:40])

    def __exit__(self, exc_type, exc, tb):
        import torch
        if exc_type is not None:
            return False
        fp = self.fp
        torch.cuda.synchronize(fp.bw.device)
        if self.bulk:
            self._exit_bulk()
            return False
        host = fp.big.cpu().numpy()
        after = host[fp.lo:fp.lo + fp.nbytes]
        bad = guard_violations(host, fp.lo, fp.nbytes, "the arena")
        for g in self.extra:
            bad += g.violations()
        more, fp.found = diff_violations(fp.amap, self.before, after, self.rule, self.envs, self.maps)
        stale = poison_violations(fp.amap, after, self.rule, self.poison, self.envs)
        fp.after = after
        if len(more) > 14:
            more = more[:14] + [f"diff: ... and {len(more) - 14} more (region, environment, kind) entries"]
        bad += more + stale[:14]
        assert not bad, f"{self.rule.name} [{self.rule.cite}]:\n  " + "\n  ".join(bad)
        return False
