"""An array-level numpy restatement of `lle_shaping_update` (include/lle_shaping.h) -- TEST INFRASTRUCTURE for
tests/test_shaping_ref_cpu.py and tests/test_gpu_shaping_states.py.

It is written the way the reference keeps its state, NOT the way the kernel does: the reached state is a boolean array
[n, A, n_cols] with one column per LIST ENTRY (reward_strategy.py:170-175, extras_generators.py:93-98) -- a source listed k times is
k columns --, the potential is `float(size - reached.sum()) * reward_value` over that array, and the rewarded cells of a column are the
oracle's own World.lasers listing filtered by laser_id (tests/oracle_shaping.positions_of), the start cells the oracle world's.
No bit words, no multiplicity masks, no cell table of the product.

Arithmetic, as pinned in tests/oracle_shaping.py: p = gamma * prev - cur in float64, the product rounded before the subtraction
(numpy evaluates the two ufuncs one after the other); kind 0: np.float32(base) + np.float32(p), added in float32; kind 1: the four
base values bit for bit, then np.float32(p).

The device keeps one u32 per (environment, agent) with bit l = source l, for ALL sources of the map: a mark ORs in every source of the
cell, listed or not.  `RefState` therefore carries, next to the listed columns, one column per source that the list does not name
(`rest`); the same operations run on them, they never count, and `to_words` / `from_words` convert to and from the device layout
(duplicated columns of one source are always equal, so the conversion loses nothing).

`fma_sensitive` and `double_rounding_sensitive` say, with exact rationals, whether a case can tell the documented arithmetic from a
fused multiply-add, or from an addition done in float64 and rounded once."""
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

CLEAR, MARK_STARTS, MARK_POS = 1, 2, 4
HONOUR_AUTO_RESET = 1


@dataclass
class RefArray:
    """One reached array: `listed` bool [n, A, n_cols] (the reference's _agents_pos_reached), `rest` bool [n, A, n_unlisted]."""
    listed: np.ndarray
    rest: np.ndarray

    def copy(self):
        return RefArray(self.listed.copy(), self.rest.copy())


@dataclass
class RefState:
    strategy: RefArray
    extras: RefArray

    def copy(self):
        return RefState(self.strategy.copy(), self.extras.copy())


class ShapingRef:
    """worlds: one OracleWorld per map of the batch (map m owns the environments [m * envs_per_map, (m + 1) * envs_per_map))."""

    def __init__(self, worlds, envs_per_map, pbrs_cols, extras_cols, gamma, reward_value):
        self.worlds, self.per = list(worlds), int(envs_per_map)
        w0 = self.worlds[0]
        self.n = self.per * len(self.worlds)
        self.A, self.L = w0.n_agents, w0.n_sources
        self.H, self.W = w0.height, w0.width
        self.pbrs_cols, self.extras_cols = [int(c) for c in pbrs_cols], [int(c) for c in extras_cols]
        self.gamma, self.reward_value = float(gamma), float(reward_value)
        # cells[m][l]: bool [H, W], the positions of get_lasers_of(world, source l); starts[m]: (i, j) per agent
        self.cells = []
        for w in self.worlds:
            assert (w.n_agents, w.n_sources, w.height, w.width) == (self.A, self.L, self.H, self.W)
            per_source = np.zeros((self.L, self.H, self.W), bool)
            for row in w.lasers():
                per_source[row[2], row[0], row[1]] = True
            self.cells.append(per_source)
        self.starts = [[(int(p[0]), int(p[1])) for p in w.start_pos] for w in self.worlds]
        self._start_cache = {}

    # ------------------------------------------------------------------ columns
    def _ids(self, which):
        """(laser_id of every listed column, laser_id of every `rest` column) of array `which` (0 strategy, 1 extras)."""
        cols = self.pbrs_cols if which == 0 else self.extras_cols
        return cols, [l for l in range(self.L) if l not in cols]

    def empty_state(self):
        def arr(which):
            cols, rest = self._ids(which)
            return RefArray(np.zeros((self.n, self.A, len(cols)), bool), np.zeros((self.n, self.A, len(rest)), bool))
        return RefState(arr(0), arr(1))

    def from_words(self, words_s, words_e):
        """The state that the device arrays u32 [n, A] stand for."""
        def arr(which, words):
            words = np.asarray(words).astype(np.uint32).reshape(self.n, self.A)
            cols, rest = self._ids(which)
            pick = lambda ids: np.stack([((words >> np.uint32(l)) & np.uint32(1)).astype(bool) for l in ids], axis=2) if ids else \
                np.zeros((self.n, self.A, 0), bool)  # noqa: E731
            return RefArray(pick(cols), pick(rest))
        return RefState(arr(0, words_s), arr(1, words_e))

    def to_words(self, state):
        """(strategy words, extras words): u32 [n, A], bit l set when a column of source l is reached."""
        out = []
        for which, arr in ((0, state.strategy), (1, state.extras)):
            cols, rest = self._ids(which)
            words = np.zeros((self.n, self.A), np.uint64)
            for ids, block in ((cols, arr.listed), (rest, arr.rest)):
                for c, l in enumerate(ids):
                    words |= block[:, :, c].astype(np.uint64) << np.uint64(l)
            out.append(words.astype(np.uint32))
        return tuple(out)

    # ------------------------------------------------------------------ the marks
    def _hits(self, ids, pos):
        """bool [n, A, len(ids)]: agent a of environment e stands on a rewarded cell of column c; a position outside the grid is on none."""
        pos = np.asarray(pos).astype(np.int64).reshape(self.n, self.A, 2)
        out = np.zeros((self.n, self.A, len(ids)), bool)
        inside = (pos[..., 0] < self.H) & (pos[..., 1] < self.W)
        i, j = np.where(inside, pos[..., 0], 0), np.where(inside, pos[..., 1], 0)
        for m in range(len(self.worlds)):
            sel = slice(m * self.per, (m + 1) * self.per)
            for c, l in enumerate(ids):
                out[sel, :, c] = self.cells[m][l][i[sel], j[sel]] & inside[sel]
        return out

    def _start_hits(self, ids):
        """bool [n, A, len(ids)]: the start cell of agent a in the environment's map is a rewarded cell of column c."""
        key = tuple(ids)
        if key not in self._start_cache:
            self._start_cache[key] = self._start_hits_uncached(ids)
        return self._start_cache[key]

    def _start_hits_uncached(self, ids):
        out = np.zeros((self.n, self.A, len(ids)), bool)
        for m in range(len(self.worlds)):
            for a, (i, j) in enumerate(self.starts[m]):
                for c, l in enumerate(ids):
                    out[m * self.per:(m + 1) * self.per, a, c] = self.cells[m][l][i, j]
        return out

    def _apply(self, which, arr, ops, pos, sel, was_reset):
        """CLEAR -> MARK_STARTS -> (the array `prev` is counted on) -> MARK_POS on the selected environments.  Returns
        (new array, listed columns before the position mark).  An array without listed columns does not exist: it is left alone."""
        cols, rest = self._ids(which)
        new = arr.copy()
        if not cols:
            return new, new.listed.copy()
        clear = sel & (was_reset | bool(ops & CLEAR))
        starts = sel & (was_reset | bool(ops & MARK_STARTS))
        marks = sel & bool(ops & MARK_POS)
        before = None
        for ids, block in ((cols, new.listed), (rest, new.rest)):
            block[clear] = False
            block |= self._start_hits(ids) & starts[:, None, None]
            if ids is cols:
                before = block.copy()
            block |= self._hits(ids, pos) & marks[:, None, None]
        return new, before

    def potential(self, listed):
        """reward_strategy.py:175 per environment: float(size - reached.sum()) * reward_value, float64 [n]."""
        size = self.A * len(self.pbrs_cols)
        return (size - listed.reshape(self.n, -1).sum(axis=1)).astype(np.float64) * np.float64(self.reward_value)

    def update(self, state, pos, evcount, strategy_ops, extras_ops, flags, reward_kind, env_mask, base_reward):
        """One lle_shaping_update.  Returns (new state, (reward, extras)): reward f32 [n, 1 | 5] (None without base_reward), extras
        f32 [n, A, E]; the rows of environments that env_mask leaves out hold what the call would NOT write (zeros here: the caller
        compares the selected rows and checks that the others keep their canary)."""
        sel = np.ones(self.n, bool) if env_mask is None else np.asarray(env_mask).reshape(self.n) != 0
        was_reset = np.zeros(self.n, bool)
        if flags & HONOUR_AUTO_RESET:
            was_reset = (np.asarray(evcount).reshape(self.n).astype(np.uint8) & 0x80) != 0
        new_s, s_before = self._apply(0, state.strategy, strategy_ops, pos, sel, was_reset)
        new_e, _ = self._apply(1, state.extras, extras_ops, pos, sel, was_reset)
        reward = None
        if base_reward is not None:
            prev, cur = self.potential(s_before), self.potential(new_s.listed)
            scaled = np.float64(self.gamma) * prev
            p = (scaled - cur).astype(np.float32)
            size = self.A * len(self.pbrs_cols)   # (for the callers' coverage assertions: the shaped term in float64 and the two counts)
            self.last = dict(p=scaled - cur, before=s_before.reshape(self.n, -1).sum(axis=1), after=new_s.listed.reshape(self.n, -1).sum(axis=1), size=size)
            if reward_kind == 0:
                base = np.asarray(base_reward, np.float32).reshape(self.n)
                with np.errstate(all="ignore"):
                    reward = (base + p).astype(np.float32).reshape(self.n, 1)
            else:
                reward = np.empty((self.n, 5), np.float32)
                reward.view(np.uint32)[:, :4] = np.asarray(base_reward, np.float32).reshape(self.n, 4).view(np.uint32)
                reward[:, 4] = p
            reward[~sel] = 0
        extras = new_e.listed.astype(np.float32)
        extras[~sel] = 0
        return RefState(new_s, new_e), (reward, extras)


# ---------------------------------------------------------------------------------------------- exact arithmetic
def _round_to(frac, mant_bits, min_exp, max_exp):
    """`frac` rounded to the nearest binary float of `mant_bits` significand bits (ties to even), as an exact Fraction; None = overflow."""
    if frac == 0:
        return Fraction(0)
    sign = -1 if frac < 0 else 1
    x = abs(frac)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, min_exp) - (mant_bits - 1))
    q = x / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    r = n * quantum
    return None if r >= Fraction(2) ** (max_exp + 1) else sign * r


def round_f64(frac):
    return _round_to(Fraction(frac), 53, -1022, 1023)


def round_f32(frac):
    return _round_to(Fraction(frac), 24, -126, 127)


def shaped_terms(gamma, value, size, before, after):
    """(documented, fused): float32(gamma * prev - cur) with the product rounded to float64 first, and with an exact product (what
    a fused multiply-add computes), as exact Fractions.  prev / cur = float(size - count) * value, rounded to float64."""
    g, v = Fraction(float(gamma)), Fraction(float(value))
    prev, cur = round_f64((size - before) * v), round_f64((size - after) * v)
    documented = round_f32(round_f64(round_f64(g * prev) - cur))
    fused = round_f32(round_f64(g * prev - cur))
    return documented, fused


def fma_sensitive(gamma, value, size, before, after):
    """True when contracting `gamma * prev - cur` into a fused multiply-add changes the float32 shaped term of a step that takes the
    reached count from `before` to `after` of `size` entries."""
    documented, fused = shaped_terms(gamma, value, size, before, after)
    return documented != fused


def fma_sensitive_pairs(gamma, value, size, brute_force=False):
    """Every (before, after), before <= after <= size, that fma_sensitive accepts.  The candidates are narrowed first: the exact product
    lies within half an ulp of the rounded one, subtraction and both roundings are monotonic, so where the float32 result is the same with
    the product moved one ulp down and one ulp up a fused multiply-add cannot change it.  Every candidate is then decided exactly."""
    if brute_force:
        return [(b, a) for b in range(size + 1) for a in range(b, size + 1) if fma_sensitive(gamma, value, size, b, a)]
    counts = np.arange(size + 1)
    pot = (size - counts).astype(np.float64) * np.float64(value)
    scaled = (np.float64(gamma) * pot)[:, None]
    cur = pot[None, :]
    mid = (scaled - cur).astype(np.float32)
    lo = (np.nextafter(scaled, -np.inf) - cur).astype(np.float32)
    hi = (np.nextafter(scaled, np.inf) - cur).astype(np.float32)
    cand = np.argwhere(((mid != lo) | (mid != hi)) & (counts[:, None] <= counts[None, :]))
    return [(int(b), int(a)) for b, a in cand if fma_sensitive(gamma, value, size, int(b), int(a))]


def double_rounding_sensitive(base, p):
    """True when `float32(base) + float32(p)` in float32 (the documented kind-0 reward) differs from float32(float64(base) + p), the
    sum taken in float64 and rounded once more.  base: a float32 value, p: the float64 shaped term; non-finite bases are not."""
    base, p = float(np.float32(base)), float(p)
    if not np.isfinite(base) or not np.isfinite(p):
        return False
    documented = round_f32(Fraction(base) + round_f32(Fraction(p)))
    once = round_f64(Fraction(base) + Fraction(p))
    once = None if once is None else round_f32(once)
    return documented != once
