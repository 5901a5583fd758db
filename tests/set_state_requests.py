"""Chosen SECOND requests for `World.set_state`: refused and lived-in requests by class (pure numpy + the oracle, no GPU).

tests/step_states.py applies accepted requests to freshly created batches.  This module starts where its protocol has been: every
environment of a map's case has taken its set_state, its explicit step and its two sampled steps without auto-reset -- deaths by
event, arrivals, collected gems, cut and stale beams, corpses -- and THEN gets a second request, chosen by class:

* planted, accepted   revive (an agent that died by an event requested alive: on its own colour's beam, which pre-enter with the CURRENT
                      flags leaves lit; with another dead agent standing in ITS own beam), bury (requested dead on plain floor, on an
                      exit, on an uncollected gem the request marks collected, on a void, on a lit beam of another colour -- the last
                      two die on entering: a death event, not a ghost), events (gem under a beam, exit, death of an agent requested dead,
                      at least A events at once where A >= 7), all-arrived (`done` turns 1), own-beam (the owner alone in its beam, then
                      with a second agent shielded behind it; on the chained maps at offsets 31 and 32 of the beam), gem 31 of `gems32`;
* planted, refused    dup (alone, with a third agent out of the world, with one on a wall: 0x40, nothing touched), oob (i == H, j == W,
                      255, and together with a wall: 0x41, nothing touched), wall / source (0x42, rolled back through a second lossy
                      set_state of the current state: stale beams are re-derived), rollback-panic (a 0x42 whose rollback the reference
                      cannot complete: a collected gem under a beam with nobody on it; a corpse on a gem under a beam whose tile the
                      rollback treats otherwise than the episode did -- on a collected gem it is now stopped in front of, or on an
                      uncollected one it is now let into, for which no lived-in batch holds a state: the beam's owner would have to step
                      in further up after the death; a living agent under a beam that was re-lit over it), mismatch (0x40
                      AFTER the request was applied, not rolled back: alive on a lit foreign beam, alive on a void, on a gem the request
                      leaves uncollected, a gem under a beam requested collected with nobody on it);
* random              uniform cells over the whole grid, gems with p = 0.3, alive with p = 0.8.

Nothing planted is trusted: every class flag of `Requests.flags` is computed from the ORACLE's outcome (error kind, events, dump before
and after, panic record) and from the map's geometry.  After the requests a masked reset of exactly the environments the reference
leaves unusable (0x40 after application: stale availability lists; a recorded panic), then one sampled step with auto-reset.

`done` after an accepted request is done_of(dump, ghost) with the ghost rule of step_states; after a refused one done_of(dump after,
ghost from BEFORE the call): a refused request leaves the bookkeeping as it was (lle_amd/csrc/kernels.hip next to `ghost =`)."""
import functools

import numpy as np

from tests import step_states as ss

CODES = {"InvalidWorldState": 0x40, "OutOfWorldPosition": 0x41, "InvalidAgentPosition": 0x42}
LIVED_IN = ss.FOLLOW_UPS[:2]    # the sampled steps without auto-reset
T_STEP = 3                      # t of the sampled step with auto-reset that ends the protocol
PLANTED_ACCEPTED, PLANTED_REFUSED = 0.40, 0.15   # shares of a case; the rest is random
PANIC_PLANTS = 2                # per kind: the envs whose state after the call is not compared stay few
STATE_KEYS = ("pos", "alive", "arrived", "occupant", "gems", "beams", "avail")
INSTANTIATIONS = ["world_kernel<4,4>", "world_kernel<8,8>", "world_kernel<16,16>", "world_kernel<16,32>"]


def instantiation_of(m):
    """kernel_variant of lle_amd/csrc/kernels.hip for a _capi.Map (its beam WORDS count: chained maps pad)."""
    A, L = m.n_agents, m.n_beam_words
    return INSTANTIATIONS[0 if A <= 4 and L <= 4 else 1 if A <= 8 and L <= 8 else 2 if A <= 16 and L <= 16 else 3]


class Layout:
    """step_states.Geometry plus what the request planters and the classifier ask of a map."""

    def __init__(self, w):
        g = self.geo = ss.Geometry(w)
        self.H, self.W, self.A, self.G = g.H, g.W, g.A, g.G
        self.sources = {(s[0], s[1]) for s in g.sources}
        self.walls = sorted(set(w.wall_pos) - self.sources)
        self.wall_set = set(self.walls)
        self.gem_index = {c: k for k, c in enumerate(g.gems)}
        self.direct = [k for k, c in enumerate(g.gems) if c not in g.layers]
        self.under_beam = [k for k, c in enumerate(g.gems) if c in g.layers]
        self.void_set, self.exit_set, self.floor_set = set(g.voids), set(g.exits), set(g.floor)
        plain = [c for c in g.layers if c in g.walk_set and c not in self.void_set]
        # cells under beams of one colour only
        self.own = {a: [c for c in plain if all(col == a for (_s, _k, col) in g.layers[c])] for a in range(self.A)}
        self.one_colour = [(c, g.layers[c][0][2]) for c in plain if len({col for (_s, _k, col) in g.layers[c]}) == 1]

    def foreign(self, a):
        """Cells under one colour of beam, not a's: lit unless that colour's agent stands further up."""
        return [c for c, col in self.one_colour if col != a and c not in self.exit_set and c not in self.gem_index]

    def exit_assignment(self, rng):
        """An exit per agent that does not kill it on entering (no beam over it, or its own colour's), or None."""
        order = [self.geo.exits[int(k)] for k in rng.permutation(len(self.geo.exits))]
        out, used = {}, set()
        for a in range(self.A):
            for c in order:
                if c not in used and all(col == a for (_s, _k, col) in self.geo.layers.get(c, [])):
                    out[a] = c
                    used.add(c)
                    break
            else:
                return None
        return out


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))] if len(seq) else None


class _Planter:
    """Builds the planted requests of one case from the lived-in dump.  A builder returns (fixed cells, agents requested dead, gem
    request) or None when this env / this map cannot hold the request; everybody else goes on plain floor away from the fixed
    cells, requested alive (step_states._scenario)."""

    def __init__(self, lay, rng, d0, ghost0):
        self.lay, self.rng, self.d0 = lay, rng, d0
        self.alive0 = d0["alive"] != 0
        self.by_event = ~self.alive0 & ~ghost0
        self.pos0 = d0["pos"].astype(np.int64)

    # ---- helpers
    def agent(self):
        return int(self.rng.integers(self.lay.A))

    def no_gems(self):
        return [False] * self.lay.G

    def agents_at(self, e, cell):
        return [a for a in range(self.lay.A) if tuple(self.pos0[e, a]) == tuple(cell)]

    # ---- accepted
    def revive_own(self, e):
        cands = [a for a in range(self.lay.A) if self.by_event[e, a] and self.lay.own[a]]
        if not cands:
            return None
        a = _pick(self.rng, cands)
        return {a: _pick(self.rng, self.lay.own[a])}, (), self.no_gems()

    def revive_dead_owner(self, e):
        lay = self.lay
        revived = [a for a in range(lay.A) if self.by_event[e, a]]
        owners = [b for b in range(lay.A) if not self.alive0[e, b] and lay.own[b]]
        pairs = [(a, b) for a in revived for b in owners if a != b]
        if not pairs or not lay.geo.floor:
            return None
        a, b = _pick(self.rng, pairs)
        return {a: _pick(self.rng, lay.geo.floor), b: _pick(self.rng, lay.own[b])}, (b,), self.no_gems()

    def bury_floor(self, e):
        return ({self.agent(): _pick(self.rng, self.lay.geo.floor)}, None, self.no_gems()) if self.lay.geo.floor else None

    def bury_exit(self, e):
        a = self.agent()
        safe = [c for c in self.lay.geo.exits if all(col == a for (_s, _k, col) in self.lay.geo.layers.get(c, []))]
        return ({a: _pick(self.rng, safe)}, None, self.no_gems()) if safe else None

    def bury_gem(self, e):
        """On an uncollected gem the request marks collected: a direct gem, or one under the beam of the buried agent's own colour."""
        lay = self.lay
        cands = [(k, None) for k in lay.direct if not self.d0["gems"][e, k]]
        cands += [(k, a) for k in lay.under_beam for a in range(lay.A) if lay.geo.gems[k] in lay.own[a] and not self.d0["gems"][e, k]]
        if not cands:
            return None
        k, a = _pick(self.rng, cands)
        gems = self.no_gems()
        gems[k] = True
        return {self.agent() if a is None else a: lay.geo.gems[k]}, None, gems

    def bury_void(self, e):
        return ({self.agent(): _pick(self.rng, self.lay.geo.voids)}, None, self.no_gems()) if self.lay.geo.voids else None

    def bury_beam(self, e):
        a = self.agent()
        cells = self.lay.foreign(a)
        return ({a: _pick(self.rng, cells)}, None, self.no_gems()) if cells else None

    def event_gem(self, e):
        cands = [(k, a) for k in self.lay.under_beam for a in range(self.lay.A) if self.lay.geo.gems[k] in self.lay.own[a]]
        if not cands:
            return None
        k, a = _pick(self.rng, cands)
        gems = self.no_gems()
        gems[k] = True
        return {a: self.lay.geo.gems[k]}, (), gems

    def event_exit(self, e):
        got = self.bury_exit(e)
        return (got[0], (), got[2]) if got else None

    def many_events(self, e):
        """At least A events: everybody who finds a harmless exit on it, the rest requested dead on voids and lit foreign beams."""
        lay = self.lay
        fixed = lay.exit_assignment(self.rng)
        if fixed is not None:
            return fixed, (), self.no_gems()
        fixed, dead, used = {}, [], set()
        for a in range(lay.A):
            safe = [c for c in lay.geo.exits if c not in used and all(col == a for (_s, _k, col) in lay.geo.layers.get(c, []))]
            hazard = [c for c in list(lay.geo.voids) + lay.foreign(a) if c not in used]
            if safe:
                fixed[a] = _pick(self.rng, safe)
            elif hazard:
                fixed[a] = _pick(self.rng, hazard)
                dead.append(a)
            else:
                return None
            used.add(fixed[a])
        return fixed, tuple(dead), self.no_gems()

    def all_arrived(self, e):
        fixed = self.lay.exit_assignment(self.rng)
        return (fixed, (), self.no_gems()) if fixed is not None else None

    def _own_beam(self, e, k=None, second=False):
        lay, geo = self.lay, self.lay.geo
        beams = [s for s, src in enumerate(geo.sources) if src[3] < lay.A and self.alive0[e, src[3]] and (k is None or len(geo.beam_cells[s]) > k + second)]
        if not beams:
            return None
        s = _pick(self.rng, beams)
        a, cells = geo.sources[s][3], geo.beam_cells[s]
        if k is None:
            k = int(self.rng.integers(len(cells) - second)) if len(cells) > second else None
        if k is None or cells[k] not in lay.own[a]:
            return None
        fixed = {a: cells[k]}
        if second:
            if lay.A < 2:
                return None
            behind = [c for c in cells[k + 1:] if c in geo.walk_set and len(geo.layers[c]) == 1 and c not in lay.void_set]
            if not behind:
                return None
            fixed[_pick(self.rng, [b for b in range(lay.A) if b != a])] = _pick(self.rng, behind)
        return fixed, (), self.no_gems()

    def own_beam_1(self, e):
        return self._own_beam(e)

    def own_beam_2(self, e):
        return self._own_beam(e, second=True)

    def own_beam_31(self, e):
        return self._own_beam(e, k=31, second=bool(self.rng.integers(2)))

    def own_beam_32(self, e):
        return self._own_beam(e, k=32, second=bool(self.rng.integers(2)))

    def _gem31(self, collected, occupied):
        gems = [bool(v) for v in self.rng.random(self.lay.G) < 0.3]
        gems[31] = collected  # (the fillers stand on plain floor: nobody on another gem)
        return ({0: self.lay.geo.gems[31]} if occupied else {}), (), gems

    def gem31_set_empty(self, e):
        return self._gem31(True, False)

    def gem31_clear_empty(self, e):
        return self._gem31(False, False)

    def gem31_set_agent(self, e):
        return self._gem31(True, True)

    # ---- refused
    def _outside(self, kind):
        lay = self.lay
        i, j = int(self.rng.integers(lay.H)), int(self.rng.integers(lay.W))
        return {"i": (lay.H, j), "j": (i, lay.W), "255": (255, 255), "i255": (255, j), "j255": (i, 255)}[kind]

    def _unwalkable(self):
        pool = self.lay.walls + sorted(self.lay.sources)
        return _pick(self.rng, pool)

    def _two(self):
        ids = [int(v) for v in self.rng.permutation(self.lay.A)[:3]]
        return ids if len(ids) >= 2 else None

    def dup(self, e):
        ids = self._two()
        if not ids:
            return None
        c = _pick(self.rng, self.lay.geo.walkable)
        return {ids[0]: c, ids[1]: c}, (), self.no_gems()

    def dup_oob(self, e):
        ids = self._two()
        if not ids:
            return None
        out = self._outside(_pick(self.rng, ["i", "j", "255"]))
        if len(ids) == 2:
            return {ids[0]: out, ids[1]: out}, (), self.no_gems()
        c = _pick(self.rng, self.lay.geo.walkable)
        return {ids[0]: c, ids[1]: c, ids[2]: out}, (), self.no_gems()

    def dup_wall(self, e):
        ids, wall = self._two(), self._unwalkable()
        if not ids or wall is None:
            return None
        if len(ids) == 2:
            return {ids[0]: wall, ids[1]: wall}, (), self.no_gems()
        c = _pick(self.rng, self.lay.geo.walkable)
        return {ids[0]: c, ids[1]: c, ids[2]: wall}, (), self.no_gems()

    def oob_i(self, e):
        return {self.agent(): self._outside("i")}, (), self.no_gems()

    def oob_j(self, e):
        return {self.agent(): self._outside("j")}, (), self.no_gems()

    def oob_255(self, e):
        return {self.agent(): self._outside(_pick(self.rng, ["255", "i255", "j255"]))}, (), self.no_gems()

    def oob_wall(self, e):
        ids, wall = self._two(), self._unwalkable()
        if not ids or wall is None:
            return None
        return {ids[0]: self._outside(_pick(self.rng, ["i", "j", "255"])), ids[1]: wall}, (), self.no_gems()  # (either agent may be the lower one)

    def wall(self, e):
        return ({self.agent(): _pick(self.rng, self.lay.walls)}, (), self.no_gems()) if self.lay.walls else None

    def source(self, e):
        return ({self.agent(): _pick(self.rng, sorted(self.lay.sources))}, (), self.no_gems()) if self.lay.sources else None

    def panic_gem(self, e):
        """A collected gem under a beam with nobody on it: the rollback's set_state(current) cannot collect it again."""
        lay = self.lay
        if not any(self.d0["gems"][e, k] and not self.agents_at(e, lay.geo.gems[k]) for k in lay.under_beam):
            return None
        return self.wall(e) or self.source(e)

    def _enters(self, e, a, cell):
        """Whether agent a gets into the innermost tile of `cell` in the rollback: the beams are re-derived from where the agents
        stand NOW, so every foreign beam over the cell must have its living owner further up (or on the cell itself)."""
        geo = self.lay.geo

        def cut(s, k):
            owner = geo.sources[s][3]
            return owner < self.lay.A and self.alive0[e, owner] and tuple(self.pos0[e, owner]) in geo.beam_cells[s][:k + 1]

        return all(col == a or cut(s, k) for (s, k, col) in geo.layers.get(cell, []))

    def _corpse_on_gem(self, e, collected):
        lay = self.lay
        return any(bool(self.d0["gems"][e, k]) == collected and
                   any(not self.alive0[e, a] and self._enters(e, a, lay.geo.gems[k]) != collected for a in self.agents_at(e, lay.geo.gems[k]))
                   for k in lay.under_beam)

    def panic_corpse(self, e):
        """A corpse on an UNCOLLECTED gem (it died under a lit beam over the gem, in front of the gem's tile) that the rollback lets
        in, because the beam's owner has since stepped into the beam further up: it collects the gem, which the current state
        does not say."""
        return (self.wall(e) or self.source(e)) if self._corpse_on_gem(e, False) else None

    def panic_corpse_collected(self, e):
        """A corpse on a COLLECTED gem under a beam (it took the gem while the beam was cut, or was requested dead on it) that the
        rollback stops in front of the gem's tile, the beam being lit again: the gem stays uncollected."""
        return (self.wall(e) or self.source(e)) if self._corpse_on_gem(e, True) else None

    def mismatch_beam(self, e):
        got = self.bury_beam(e)
        return (got[0], (), got[2]) if got else None

    def mismatch_void(self, e):
        got = self.bury_void(e)
        return (got[0], (), got[2]) if got else None

    def mismatch_gem_left(self, e):
        if not self.lay.direct:
            return None
        return {self.agent(): self.lay.geo.gems[_pick(self.rng, self.lay.direct)]}, (), self.no_gems()

    def mismatch_gem_under_beam(self, e):
        if not self.lay.under_beam:
            return None
        gems = self.no_gems()
        gems[_pick(self.rng, self.lay.under_beam)] = True
        return {}, (), gems

    def gem31_clear_agent(self, e):
        return self._gem31(False, True)

    def request(self, kind, e):
        """(positions, gems, alive) of a planted request of `kind` for env e, or None."""
        got = getattr(self, kind)(e)
        if got is None:
            return None
        fixed, dead, gems = got
        if any(c is None for c in fixed.values()):
            return None
        if dead is None:  # bury: the one fixed agent is requested dead
            dead = tuple(fixed)
        sc = ss._scenario(self.lay.geo, self.rng, fixed, {}, dead=dead, gems=gems)
        return None if sc is None else sc[:3]


ACCEPTED_KINDS = ["revive_own", "revive_dead_owner", "bury_floor", "bury_exit", "bury_gem", "bury_void", "bury_beam", "event_gem", "event_exit",
                  "many_events", "all_arrived", "own_beam_1", "own_beam_2"]
REFUSED_KINDS = ["dup", "dup_oob", "dup_wall", "oob_i", "oob_j", "oob_255", "oob_wall", "wall", "source", "mismatch_beam", "mismatch_void",
                 "mismatch_gem_left", "mismatch_gem_under_beam"]
PANIC_KINDS = ["panic_gem", "panic_corpse", "panic_corpse_collected"]


def kinds_of(name):
    acc, ref = list(ACCEPTED_KINDS), list(REFUSED_KINDS)
    if name in ss.CHAINED:
        acc += ["own_beam_31", "own_beam_32"]
    if name == "gems32":
        acc += ["gem31_set_empty", "gem31_clear_empty", "gem31_set_agent"]
        ref += ["gem31_clear_agent"]
    return acc, ref


def plant(name, lay, rng, d0, ghost0, n):
    """{env: (kind, positions, gems, alive)}: the kinds in turn over a seeded order of the envs, each on the next env that can hold it."""
    planter = _Planter(lay, rng, d0, ghost0)
    order = [int(e) for e in rng.permutation(n)]
    out = {}

    def place(kind, scan=64):
        tried = 0
        for e in order:
            if e in out:
                continue
            tried += 1
            if tried > scan:
                return False
            req = planter.request(kind, e)
            if req is not None:
                out[e] = (kind,) + req
                return True
        return False

    for kind in PANIC_KINDS:  # (their pre-states are rare: the whole batch is searched)
        for _ in range(PANIC_PLANTS):
            place(kind, scan=n)
    acc, ref = kinds_of(name)
    for kinds, share in ((acc, PLANTED_ACCEPTED), (ref, PLANTED_REFUSED)):
        quota, live = int(share * n), list(kinds)
        while quota > 0 and live:
            for kind in list(live):
                if quota <= 0:
                    break
                if place(kind):
                    quota -= 1
                else:
                    live.remove(kind)
    return out


def random_request(rng, lay):
    pos = np.stack([rng.integers(0, lay.H, size=lay.A), rng.integers(0, lay.W, size=lay.A)], axis=-1)
    return [tuple(int(v) for v in p) for p in pos], [bool(v) for v in rng.random(lay.G) < 0.3], [bool(v) for v in rng.random(lay.A) < 0.8]


def _lit(lay, beams, cell, colour):
    return any(col == colour and beams[s, k] for (s, k, col) in lay.geo.layers.get(cell, []))


def classify_env(name, lay, req, pre, post, ghost0, err, events, panicked):
    """The class flags of ONE env's request, from the oracle's outcome: pre / post = its dump rows before / after the call."""
    pos, gems, alive = req
    A, H, W, geo = lay.A, lay.H, lay.W, lay.geo
    f = set()
    dup = len(set(pos)) < A
    outside = [not (i < H and j < W) for (i, j) in pos]
    on_wall, on_source = [c in lay.wall_set for c in pos], [c in lay.sources for c in pos]
    changed = any(not np.array_equal(pre[k], post[k]) for k in STATE_KEYS)
    if err == 0x40 and dup:
        f |= {"0x40-untouched", "dup"} | ({"dup-with-oob"} if any(outside) else set()) | ({"dup-with-wall"} if any(on_wall) or any(on_source) else set())
    elif err == 0x41:
        f.add("0x41")
        f |= {tag for tag, hit in (("oob-i-is-H", any(i == H for (i, _j) in pos)), ("oob-j-is-W", any(j == W for (_i, j) in pos)),
                                   ("oob-255", any(255 in c for c in pos)), ("oob-with-wall", any(on_wall) or any(on_source))) if hit}
    elif err == 0x42:
        f.add("0x42")
        f |= ({"wall"} if any(on_wall) else set()) | ({"source"} if any(on_source) else set())
        if panicked:
            f.add("rollback-panic")
            at = {k: [a for a in range(A) if tuple(pre["pos"][a]) == geo.gems[k]] for k in range(lay.G)}
            # (the reference does not roll back what it panicked over: the dump after the call shows which part of the current state
            # its inner set_state failed to restore)
            if any(pre["gems"][k] and not at[k] and not post["gems"][k] for k in lay.under_beam):
                f.add("panic-collected-gem-under-beam")
            if any(not pre["gems"][k] and post["gems"][k] and any(not pre["alive"][a] for a in at[k]) for k in range(lay.G)):
                f.add("panic-corpse-on-gem")
            if any(pre["gems"][k] and not post["gems"][k] and any(not pre["alive"][a] for a in at[k]) for k in lay.under_beam):
                f.add("panic-corpse-on-collected-gem")
            if any(pre["alive"][a] and not post["alive"][a] for a in range(A)):
                f.add("panic-alive-under-relit-beam")
            if not f & {"panic-collected-gem-under-beam", "panic-corpse-on-gem", "panic-corpse-on-collected-gem", "panic-alive-under-relit-beam"}:
                f.add("panic-other")
        else:
            f.add("rollback-completed")
            if changed:
                f.add("rollback-visible")
    elif err == 0x40:
        f.add("0x40-applied")
        for a in range(A):
            if alive[a] and not post["alive"][a]:
                f.add("mismatch-void" if pos[a] in lay.void_set else "mismatch-beam" if pos[a] in geo.layers else "mismatch-other")
            k = lay.gem_index.get(pos[a])
            if k is not None and not gems[k] and post["gems"][k]:
                f.add("mismatch-gem-left")
                if name == "gems32" and k == 31:
                    f.add("gem31-clear-agent")
        if any(gems[k] and not post["gems"][k] and geo.gems[k] not in pos for k in lay.under_beam):
            f.add("mismatch-gem-under-beam")
    else:
        assert err == 0
        f.add("accepted")
        died = {a for (ty, a) in events if ty == ss.EV_DIED}
        kinds = {ty for (ty, _a) in events}
        f |= {tag for tag, ty in (("event-gem", ss.EV_GEM), ("event-exit", ss.EV_EXIT), ("event-died", ss.EV_DIED)) if ty in kinds}
        f.add(f"events-{min(len(events), 3)}" + ("+" if len(events) >= 3 else ""))
        if A >= 7 and len(events) >= A:
            f.add("events-A")
        if any(events[q + 1][1] < events[q][1] for q in range(len(events) - 1)):
            f.add("id-inversion")
        if post["arrived"].all():
            f.add("all-arrived")
        by_event = [not pre["alive"][a] and not ghost0[a] for a in range(A)]
        revived = [a for a in range(A) if by_event[a] and post["alive"][a]]
        if revived:
            f.add("revive")
        for a in revived:
            if _lit(lay, post["beams"], pos[a], a):
                f.add("revive-on-own-lit-beam")
            if any(b != a and not pre["alive"][b] and _lit(lay, post["beams"], pos[b], b) for b in range(A)):
                f.add("revive-with-dead-owner-in-lit-beam")
        for a in range(A):
            if alive[a]:
                continue
            if a in died:
                f |= {"event-died-requested-dead", "bury-void" if pos[a] in lay.void_set else "bury-lit-beam"}
            elif pos[a] in lay.floor_set:
                f.add("bury-floor")
            elif pos[a] in lay.exit_set:
                f.add("bury-exit")
            elif pos[a] in lay.gem_index and gems[lay.gem_index[pos[a]]] and not pre["gems"][lay.gem_index[pos[a]]]:
                f.add("bury-gem")
            if a not in died and not pre["alive"].all():
                f.add("ghost-from-lived-in")  # a ghost bit set over a state that was not all alive
        for s, src in enumerate(geo.sources):
            c, cells = src[3], geo.beam_cells[s]
            inside = sorted((cells.index(pos[a]), a) for a in range(A) if pos[a] in cells)
            if c >= A or not inside or inside[0][1] != c or not pre["alive"][c] or not post["alive"][c]:
                continue
            if len(inside) == 1:
                f.add("own-beam-1")
            elif len(inside) == 2 and post["alive"][inside[1][1]]:
                f.add("own-beam-2")
            k = inside[0][0]
            if k % 32 == 31 and len(cells) > k + 1:
                f.add("own-beam-word-end")
            if k >= 32 and k % 32 == 0:
                f.add("own-beam-word-start")
        if name == "gems32":
            here = geo.gems[31] in pos
            f.add(("gem31-set-" if gems[31] else "gem31-clear-") + ("agent" if here else "empty"))
    return f


def structural_classes(name, lay):
    """The classes asserted on one map by itself: what its geometry can show whatever the lived-in states are.  (Revivals and the
    rollbacks that panic need a death by event / a walked-off gem in the lived-in batch: asserted per instantiation and on the maps
    tests/test_set_state_requests_cpu.py names.)"""
    A, geo = lay.A, lay.geo
    out = ["accepted", "0x41", "oob-i-is-H", "oob-j-is-W", "oob-255", "event-exit", "bury-exit", "events-0"]
    unwalkable = bool(lay.walls or lay.sources)
    if unwalkable:
        out += ["0x42", "rollback-completed"]
    if lay.walls:
        out.append("wall")
    if lay.sources:
        out.append("source")
    if any(src[3] < A for src in geo.sources):
        # (the lossy re-derivation shows where a beam can be stale, i.e. where an agent can cut one: not on colour_alias, whose
        # colours have no agent -- its beams are fully lit before and after whatever happens)
        out.append("rollback-visible")
    if A >= 2:
        out += ["0x40-untouched", "dup", "dup-with-oob"] + (["dup-with-wall", "oob-with-wall"] if unwalkable else [])
    if geo.floor:
        out.append("bury-floor")
    if lay.direct:
        out += ["bury-gem", "mismatch-gem-left"]
    if geo.voids:
        out += ["mismatch-void", "bury-void"]
    if any(lay.foreign(a) for a in range(A)):
        out += ["mismatch-beam", "bury-lit-beam", "event-died-requested-dead"]
    if lay.under_beam:
        out.append("mismatch-gem-under-beam")
    if any(geo.gems[k] in lay.own[a] for k in lay.under_beam for a in range(A)):
        # (a gem under the beam of an agent's colour: collected by its event, and -- walked off in the lived-in steps -- what the
        # reference's rollback cannot restore.  Narrower than "a gem under a beam": on colour_alias the gem lies under a colour without
        # an agent, on four_layers under four colours, two of them without an agent -- those beams stay lit over the gem, whoever
        # enters dies in front of the gem's tile, nobody ever collects it, so no rollback can find it collected and walked off)
        out += ["event-gem", "rollback-panic", "panic-collected-gem-under-beam"]
    if any(lay.own[a] for a in range(A)):
        out.append("own-beam-1")
    if any(lay.own[a] and (lay.foreign(a) or geo.voids) for a in range(A)):
        out += ["revive", "revive-on-own-lit-beam"]  # (an agent with a beam of its own and something to die on)
    if A >= 7:
        out.append("events-A")
    if name in ss.CHAINED:
        out += ["own-beam-word-end", "own-beam-word-start"]
    if name == "gems32":
        out += ["gem31-set-empty", "gem31-clear-empty", "gem31-set-agent", "gem31-clear-agent"]
    return out


class Requests:
    """The oracle's side of the protocol for one batch: `lived_in` (the step_states Reference up to the second sampled step), the
    second requests (pos / gems / alive, `kinds`), and the records `before`, `after_request`, `after_reset`, `after_step`."""


def _obs(ob):
    return np.stack([ob.world(e).obs() for e in range(ob.n)])


def reference_run(oracle_mod, name, case, sources=None, rng=None, env_offset=ss.ENV_OFFSET, seed_key=0):
    """Runs the whole protocol on the oracle.  `sources` / `rng`: per-environment sources first (step_states.reference_run)."""
    r = Requests()
    ref = r.lived_in = ss.reference_run(oracle_mod, case, sources=sources, rng=rng, env_offset=env_offset, follow_ups=LIVED_IN)
    ob, n, A, G = ref.ob, case.n, case.A, case.G
    r.ob, r.case, r.name, r.env_offset = ob, case, name, env_offset
    lay = r.layout = Layout(ob.world0)
    d0, ghost0 = ref.steps[-1]["dump"], ref.steps[-1]["ghost"]
    r.before = {"dump": d0, "ghost": ghost0, "done": ref.steps[-1]["done"]}
    prng = np.random.default_rng([ss.MAP_NAMES.index(name), seed_key, 515])
    planted = plant(name, lay, prng, d0, ghost0, n)
    r.pos = np.zeros((n, A, 2), np.uint8)
    r.gems, r.alive = np.zeros((n, G), bool), np.zeros((n, A), bool)
    r.kinds = []
    err, ev_count, events = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 2 * A, 2), np.uint8)
    ghost, panicked = ghost0.copy(), np.zeros(n, bool)
    evs = []
    for e in range(n):
        kind, pos, gems, alive = planted[e] if e in planted else ("random",) + random_request(prng, lay)
        r.kinds.append(kind)
        pos = [tuple(int(v) for v in p) for p in pos]
        r.pos[e], r.gems[e], r.alive[e] = np.array(pos, np.uint8).reshape(A, 2), gems, alive
        w = ob.world(e)
        p0 = w.panics()[0]
        try:
            ev = w.set_state(pos, [bool(v) for v in gems], [bool(v) for v in alive])
            died = {a for (ty, a) in ev if ty == ss.EV_DIED}
            ghost[e] = [not alive[a] and a not in died for a in range(A)]
            ev_count[e] = len(ev)
            if ev:
                events[e, :len(ev)] = ev
        except oracle_mod.OracleError as ex:
            err[e], ev = CODES[ex.kind], []  # (a refused request: no events, the bookkeeping as it was)
        evs.append(ev)
        panicked[e] = w.panics()[0] != p0
    d1 = ob.dump()
    r.panics_after_request = np.array([ob.world(e).panics()[0] for e in range(n)])
    r.after_request = {"err": err, "ev_count": ev_count, "events": events, "dump": d1, "ghost": ghost.copy(), "done": ss.done_of(d1, ghost),
                       "obs": _obs(ob), "panicked": panicked}
    flags = {}
    for e in range(n):
        req = ([tuple(int(v) for v in p) for p in r.pos[e]], r.gems[e], r.alive[e])
        row = lambda d: {k: d[k][e] for k in STATE_KEYS}  # noqa: E731
        for tag in classify_env(name, lay, req, row(d0), row(d1), ghost0[e], int(err[e]), evs[e], bool(panicked[e])):
            flags.setdefault(tag, np.zeros(n, bool))[e] = True
    r.flags = flags
    untouched = flags.get("0x40-untouched", np.zeros(n, bool))
    # ---- the masked reset: the envs the reference leaves with stale availability lists, or in a state it panicked over
    r.mask = ((err == 0x40) & ~untouched) | panicked
    for e in np.nonzero(r.mask)[0]:
        ob.world(int(e)).reset()
    ghost = ghost & ~r.mask[:, None]
    d2 = ob.dump()
    r.after_reset = {"dump": d2, "ghost": ghost.copy(), "done": ss.done_of(d2, ghost), "obs": _obs(ob)}
    # ---- one sampled step with auto-reset
    ostep = ob.step(None, auto_reset=True, seed=ss.SEED, t=T_STEP, env_offset=env_offset)
    ghost = ghost & ((ostep["ev_count"] & 0x80) == 0)[:, None]
    d3 = ob.dump()
    r.after_step = {"ostep": ostep, "dump": d3, "ghost": ghost.copy(), "done": ss.done_of(d3, ghost)}
    r.panics_after_step = np.array([ob.world(e).panics()[0] for e in range(n)]) - r.panics_after_request
    return r


def outcome_counts(r):
    """[accepted, 0x40 untouched, 0x40 applied, 0x41, 0x42, panic-excluded] of a batch."""
    f, n = r.flags, r.case.n
    count = lambda k: int(f.get(k, np.zeros(n, bool)).sum())  # noqa: E731
    return [count("accepted"), count("0x40-untouched"), count("0x40-applied"), count("0x41"), count("0x42"), int(r.after_request["panicked"].sum())]


@functools.lru_cache(maxsize=None)
def build(name, variant=0, n=None, env_offset=ss.ENV_OFFSET):
    """The protocol of a map's case on the oracle (computed once; nobody changes it)."""
    from oracle import oracle as oracle_mod
    oracle_mod.build()
    return reference_run(oracle_mod, name, ss.build_case(name, variant, n), env_offset=env_offset, seed_key=variant)


# ---- the engine's side: `eng` = parity_util.unpack_engine of its buffers, `done` its done bytes
def _rows(d, keep):
    return {k: d[k][keep] for k in STATE_KEYS}


def compare_after_request(r, eng, done, where):
    """Every env after the second request: err; evcount and the ordered events (0 and all zero after any refusal); the full state;
    done; the observation.  The envs over which the reference panicked are held to their error code alone."""
    from tests.parity_util import assert_state_equal
    rec = r.after_request
    keep = ~rec["panicked"]
    bad = np.nonzero(eng["err"] != rec["err"])[0]
    assert not len(bad), f"{where}: err differs in {len(bad)} envs; first env {bad[0]} ({r.kinds[bad[0]]}): engine={eng['err'][bad[0]]:#x} oracle={rec['err'][bad[0]]:#x}"
    assert (eng["err"][~keep] == 0x42).all() and 20 * int((~keep).sum()) <= len(keep), f"{where}: {int((~keep).sum())} of {len(keep)} envs are not compared"
    for key in ("ev_count", "events"):
        bad = np.nonzero((eng[key] != rec[key]).reshape(len(keep), -1).any(1) & keep)[0]
        assert not len(bad), f"{where}: '{key}' differs in {len(bad)} envs; first env {bad[0]} ({r.kinds[bad[0]]}): engine={eng[key][bad[0]].tolist()} oracle={rec[key][bad[0]].tolist()}"
    assert_state_equal(_rows(eng, keep), _rows(rec["dump"], keep), f"{where} after the request")
    assert np.array_equal(np.asarray(done)[keep] != 0, rec["done"][keep]), f"{where}: done after the request, envs {np.nonzero((np.asarray(done) != 0) != rec['done'])[0][:8].tolist()}"
    assert np.array_equal(eng["obs"][keep], rec["obs"][keep]), f"{where}: observation after the request"


def compare_after_reset(r, eng, done, raw_before, raw_after, where):
    """After the masked reset: every env against the oracle again (the panicked ones included: they are in the mask), the masked envs
    report err 0 and no event, the others are bit-identical in every buffer."""
    from tests.parity_util import assert_state_equal
    rec, mask = r.after_reset, r.mask
    assert_state_equal(eng, rec["dump"], f"{where} after the masked reset")
    assert np.array_equal(np.asarray(done) != 0, rec["done"]), f"{where}: done after the masked reset"
    assert np.array_equal(eng["obs"], rec["obs"]), f"{where}: observation after the masked reset"
    assert not eng["err"][mask].any() and not eng["ev_count"][mask].any() and not eng["events"][mask].any(), f"{where}: err / events of the reset envs"
    for key, was in raw_before.items():
        assert np.array_equal(np.asarray(raw_after[key])[~mask], np.asarray(was)[~mask]), f"{where}: '{key}' of an env outside the mask changed"


def compare_after_step(r, eng, done, where):
    from tests.parity_util import assert_state_equal, assert_step_equal
    rec = r.after_step
    assert_step_equal(eng, rec["ostep"], f"{where} follow-up step")
    assert_state_equal(eng, rec["dump"], f"{where} follow-up step")
    assert np.array_equal(np.asarray(done) != 0, rec["done"]), f"{where}: done after the follow-up step"
