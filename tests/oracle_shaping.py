"""Per-environment numpy restatement of the reference's PotentialShapedLLE (python/lle/env/reward_strategy.py:112-181) and
LaserSubgoal / MultiGenerator (python/lle/env/extras_generators.py:46-101) on top of tests/oracle_env.py -- TEST INFRASTRUCTURE for
tests/test_shaping_cpu.py and tests/test_gpu_shaping.py, like everything that imports oracle/.

The rewarded positions come from the oracle's own World.lasers listing (`OracleWorld.lasers()`: the outer two laser layers of a
cell, src/core/world.rs:159-172) filtered by laser_id (python/lle/env/utils.py:6-11) -- not from the product's cell table.

Arithmetic, pinned: potential = float(entries not reached) * reward_value; p = gamma * previous - current in float64 (Python
floats); SingleObjective underneath: reward[0] = float32(reward[0]) + float32(p), added in float32 (numpy's `reward[0] += p`
on a float32 array); MultiObjective underneath: the float32 reward with float32(p) appended (the reference's np.concat yields
float64 there; the product documents float32).

`run_case` plays a case of tests/golden/kat_shaping.json against an adapter:
    make(case) -> adapter; adapter.extras_shape, adapter.objectives; adapter.reset() -> extras [A, E];
    adapter.step(actions) -> (reward, done, extras).
"""
import json
import os

import numpy as np

from tests.oracle_env import OracleLLE

HERE = os.path.dirname(os.path.abspath(__file__))


def source_at(world, position):
    """World.source_at: the laser_id of the source at `position`."""
    for lid, s in enumerate(world.sources()):
        if (s[0], s[1]) == tuple(position):
            return lid
    raise ValueError(f"Tile at position {tuple(position)} is not a laser source")


def positions_of(world, laser_id):
    """set(laser.pos for laser in get_lasers_of(world, source))."""
    return {(row[0], row[1]) for row in world.lasers() if row[2] == laser_id}


class OracleShapedLLE(OracleLLE):
    """OracleLLE with `pbrs` = None | dict(gamma, reward_value, lasers) -- lasers: laser_ids in the caller's order, None = all -- and
    `extras` = a list of LaserSubgoal source lists (laser_ids; None = all), concatenated like MultiGenerator does."""

    def __init__(self, world, pbrs=None, extras=(), **kw):
        super().__init__(world, **kw)
        every = list(range(world.n_sources))
        self.pbrs = pbrs
        A = world.n_agents
        if pbrs is not None:
            self.gamma, self.reward_value = float(pbrs["gamma"]), float(pbrs["reward_value"])
            ids = every if pbrs.get("lasers") is None else list(pbrs["lasers"])
            self.pos_to_reward = [positions_of(world, l) for l in ids]
            self._reached = np.full((A, len(ids)), False, dtype=bool)
            self._previous_potential = self.compute_potential()
        self.extras_ids = [l for g in extras for l in (every if g is None else list(g))]
        self.extras_pos = [positions_of(world, l) for l in self.extras_ids]
        self.extras_reached = np.full((A, len(self.extras_ids)), False, dtype=bool)
        srcs = world.sources()
        self.extras_meanings = [f"Source {l} at {(srcs[l][0], srcs[l][1])}" for l in self.extras_ids]

    @property
    def objectives(self):
        base = ["gem", "exit", "death", "done"] if self.multi_objective else ["reward"]
        return base + (["PBRS"] if self.multi_objective and self.pbrs is not None else [])

    @property
    def extras_shape(self):
        return (len(self.extras_ids),)

    def compute_potential(self):                    # reward_strategy.py:170-175
        for a, pos in enumerate(self.w.positions()):
            for j, rewarded in enumerate(self.pos_to_reward):
                if tuple(pos) in rewarded:
                    self._reached[a, j] = True
        return float(self._reached.size - self._reached.sum()) * self.reward_value

    def compute_extras(self):                       # extras_generators.py:93-98
        for a, pos in enumerate(self.w.positions()):
            for j, rewarded in enumerate(self.extras_pos):
                if tuple(pos) in rewarded:
                    self.extras_reached[a, j] = True
        return self.extras_reached.astype(np.float32)

    def _strategy_reset(self):                      # reward_strategy.py:177-181
        self.n_arrived = self.n_deads = 0
        if self.pbrs is not None:
            self._reached.fill(False)
            self._previous_potential = self.compute_potential()

    def reset(self, colours=None):                  # env.py:191-203: world, strategy, extras (cleared; computed with the observation)
        self.w.reset()
        self._strategy_reset()
        self.extras_reached.fill(False)
        self.done = False
        if colours is not None:
            for l, c in enumerate(colours):
                self.w.set_source(l, colour=int(c))

    def compute_reward(self, events):               # reward_strategy.py:148-160
        reward = super().compute_reward(events)
        if self.pbrs is None:
            return reward
        current = self.compute_potential()
        p = self.gamma * self._previous_potential - current
        self._previous_potential = current
        if not self.multi_objective:
            reward[0] = np.float32(reward[0]) + np.float32(p)
            return reward
        return np.concatenate([reward, np.array([p], dtype=np.float32)]).astype(np.float32)

    def set_state(self, positions, gems, alive):   # env.py:208-217: the strategy restarts where the agents stand BEFORE the call
        self._strategy_reset()
        events = self.w.set_state(positions, gems, alive)
        self.compute_reward(events)
        self.done = self.n_arrived == self.n_agents or self.n_deads > 0


# ---------------------------------------------------------------------------------------------- tests/golden/kat_shaping.json
def load_cases():
    with open(os.path.join(HERE, "golden", "kat_shaping.json")) as f:
        return json.load(f)["cases"]


def case_generators(case):
    """The LaserSubgoal source lists a Builder would end with (builder.py:100-101,117-146): [positions | None, ...]."""
    gens = []
    if case["pbrs"] is not None and case["pbrs"]["with_extras"]:
        gens.append(case["pbrs"]["lasers"])
    for extra in case["add_extras"]:
        assert extra == "laser_subgoal"
        gens.append(None)
    return gens


def run_case(make_adapter, case):
    ad = make_adapter(case)
    name = case["name"]
    if case["extras_shape"] is not None:
        assert tuple(ad.extras_shape) == tuple(case["extras_shape"]), f"{name}: extras_shape {ad.extras_shape}"
    if case["objectives"] is not None:
        assert list(ad.objectives) == case["objectives"], f"{name}: objectives {ad.objectives}"

    def check_extras(got, op, k):
        got = np.asarray(got, dtype=np.float32)
        assert got.dtype == np.float32 and got.shape[1:] == tuple(ad.extras_shape), f"{name} op {k}: extras {got.shape}"
        if op.get("extras_sums") is not None:
            assert got.sum(axis=1).tolist() == op["extras_sums"], f"{name} op {k}: extras sums {got.sum(axis=1)}"
        if op.get("extras") is not None:
            assert np.array_equal(got, np.array(op["extras"], dtype=np.float32)), f"{name} op {k}: extras {got}"

    for k, op in enumerate(case["script"]):
        if op["op"] == "reset":
            check_extras(ad.reset(), op, k)
        elif op["op"] == "step":
            reward, done, extras = ad.step(op["actions"])
            if op["reward"] is not None:
                want = np.atleast_1d(np.array(op["reward"], dtype=np.float64)).astype(np.float32)  # float32(expected): numpy's weak scalars
                got = np.asarray(reward).reshape(-1)
                assert got.dtype == np.float32 and np.array_equal(got, want), f"{name} op {k}: reward {got} != {want}"
            if op["done"] is not None:
                assert bool(done) == op["done"], f"{name} op {k}: done {done}"
            check_extras(extras, op, k)
        else:
            raise ValueError(op)


class OracleAdapter:
    """A KAT case on the restatement."""

    def __init__(self, case, oracle_mod):
        w = oracle_mod.OracleWorld(case["map"])
        ids = lambda ps: None if ps is None else [source_at(w, p) for p in ps]  # noqa: E731
        pb = case["pbrs"]
        self.env = OracleShapedLLE(w, pbrs=None if pb is None else dict(gamma=pb["gamma"], reward_value=pb["reward_value"], lasers=ids(pb["lasers"])),
                                   extras=[ids(g) for g in case_generators(case)], multi_objective=case["multi_objective"])
        self.extras_shape, self.objectives = self.env.extras_shape, self.env.objectives

    def reset(self):
        self.env.reset()
        return self.env.compute_extras()

    def step(self, actions):
        reward, done = self.env.step(actions)
        return reward, done, self.env.compute_extras()


# maps of the shaping tests beyond the levels and tests/parity_util.py: cell (2, 2) lies under exactly THREE beams (L0 from the north, L1 from the
# west, L2 from the south); World.lasers lists its outer two layers only, so one of the three sources never counts there
SHAPING_MAPS = {
    "three_beam_cell": ". . L0S . .\n. . . . .\nL1E . . . @\n. . . . .\nS0 S1 L2N X X",
    # both agents START on a tile of their own colour's beam: the start-cell masks are non-zero, so a reset (and an auto-reset's
    # previous potential) begins with those sources already reached; agent 1 dies on agent 0's beam once agent 0 has left it
    "start_on_beam": "L0E S0 . . X\n. . . . .\nL1E . S1 . X\n. G . . .",
}
