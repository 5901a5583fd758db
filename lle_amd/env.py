"""BatchedLLE: n lock-stepped `LLE` environments on one MI355X.

The reference's `LLE` (python/lle/env/env.py:39-255) is a thin host class around `World.step`: events -> reward
strategy, `compute_done`, observation / state generators, `available_actions` (optionally without moves into foreign
lasers), `randomize_lasers` on reset.  Every one of those pieces already runs on the GPU behind the C ABI
(include/lle_hip.h); this class strings them together with the reference's argument names and meanings and returns
device tensors with a leading env axis.  No marlenv dependency; "rgb-image" frames come from the render kernel
(lle_amd.rendering); potential-based reward shaping and the laser-subgoal extras (`reward_strategy=`, `extras_generator=`) come
from the shaping kernel (lle_amd.shaping, loaded only when one of them is asked for).

    env = BatchedLLE(Map(level=6), 65536, obs_type="layered", randomize_lasers=True)
    obs, state = env.reset()
    step = env.step(actions)            # dict: obs, state, reward, done, available_actions
"""
import os
from enum import IntEnum

import torch

from . import _capi
from .batched import BatchedWorld, _current_stream_handle


class DeathStrategy(IntEnum):
    """python/lle/env/env.py:23-37."""
    END = 0      # the episode ends when an agent dies
    RESPAWN = 1  # (not implemented by the reference either: env.py:106-107)

    @staticmethod
    def from_str(value):
        if value == "end":
            return DeathStrategy.END
        if value == "respawn":
            return DeathStrategy.RESPAWN
        raise ValueError(f"Unknown death strategy: {value}")

_OBS_KINDS = {
    "layered": (_capi.LLE_OBS_LAYERED, 0), "flattened": (_capi.LLE_OBS_LAYERED, 0),
    "partial3x3": (_capi.LLE_OBS_PARTIAL, 3), "partial5x5": (_capi.LLE_OBS_PARTIAL, 5), "partial7x7": (_capi.LLE_OBS_PARTIAL, 7),
    "state": (_capi.LLE_OBS_STATE, 0), "normalized-state": (_capi.LLE_OBS_NORMALIZED_STATE, 0),
    "perspective": (_capi.LLE_OBS_PERSPECTIVE, 0),
    "layered-padded-1": (_capi.LLE_OBS_LAYERED_PADDED, 1), "layered-padded-2": (_capi.LLE_OBS_LAYERED_PADDED, 2),
    "layered-padded-3": (_capi.LLE_OBS_LAYERED_PADDED, 3),
}
_RGB_IMAGE = -1  # the kind of "rgb-image": frames of the render kernel (BatchedWorld.render), not an lle_batch_observe_as kind


# ------------------------------------------------------------------ reward strategies and extras generators (descriptors)
# The reference's classes (python/lle/env/reward_strategy.py, extras_generators.py) hold a World and per-episode numpy state.  Here
# they only DESCRIBE what BatchedLLE computes on the device: same names, same argument order, `world` optional (None = the maps
# of the environment they are handed to).
class SingleObjective:
    """reward_strategy.py:51-75: one scalar reward."""
    objectives = ("reward",)

    def __init__(self, n_agents=None):
        self.n_agents = n_agents


class MultiObjective:
    """reward_strategy.py:78-109: [gem, exit, death, done]."""
    objectives = ("gem", "exit", "death", "done")

    def __init__(self, n_agents=None):
        self.n_agents = n_agents


def _as_map(world):
    """Anything BatchedLLE accepts as ONE map (a Map, a map text), or a lle_amd.World."""
    if isinstance(world, _capi.Map):
        return world
    if isinstance(getattr(world, "_map", None), _capi.Map):
        return world._map
    if isinstance(world, (list, tuple)):
        return _as_map(world[0])
    return _capi.Map(world)


def _source_at(map_, position):
    """World.source_at (lle_amd/world.py): the laser_id of the source at `position`."""
    position = tuple(position)
    if len(position) != 2 or position[0] < 0 or position[1] < 0 or position[0] >= map_.height or position[1] >= map_.width:
        raise IndexError("Position out of bounds")
    for s in map_.sources():
        if (int(s.i), int(s.j)) == (int(position[0]), int(position[1])):
            return int(s.laser_id)
    raise ValueError(f"Tile at position {position} is not a laser source")


def _resolve_sources(map_, sources):
    """laser_ids of `sources`: None = every source of the map; (i, j) positions or objects with `.laser_id` (builder.py:88-99)."""
    n = map_.n_sources
    if sources is None:
        return list(range(n))
    out = []
    for source in sources:
        if isinstance(source, (tuple, list)):
            out.append(_source_at(map_, source))
        elif hasattr(source, "laser_id"):
            lid = int(source.laser_id)
            if not 0 <= lid < n:
                raise ValueError(f"Invalid laser source: laser_id {lid} on a map with {n} sources")
            out.append(lid)
        else:
            raise ValueError(f"Invalid laser source: {source}")
    return out


class PotentialShapedLLE:
    """reward_strategy.py:112-181: potential-based shaping around `strategy` (a SingleObjective or a MultiObjective): crossing the
    beam of a source of `lasers_to_reward` -- (i, j) positions or objects with `.laser_id`; None: every source; a source listed
    twice counts twice, the reference iterates a list -- for the first time in an episode is worth `reward_value`."""

    def __init__(self, strategy, world=None, gamma=0.99, reward_value=0.5, lasers_to_reward=None):
        if not isinstance(strategy, (SingleObjective, MultiObjective)):
            raise ValueError(f"PotentialShapedLLE wraps a SingleObjective or a MultiObjective, got {strategy!r}")
        self.strategy, self.world = strategy, world
        self.gamma, self.reward_value = float(gamma), float(reward_value)
        self.lasers_to_reward = None if lasers_to_reward is None else list(lasers_to_reward)
        if world is not None:
            self.laser_ids(None)  # a position that is not a source raises here, like the reference's constructor

    @property
    def objectives(self):
        return self.strategy.objectives + (("PBRS",) if isinstance(self.strategy, MultiObjective) else ())

    def laser_ids(self, default_map):
        return _resolve_sources(_as_map(self.world) if self.world is not None else default_map, self.lasers_to_reward)


class NoExtras:
    """extras_generators.py:36-43."""
    size, meanings = 0, ()

    def __init__(self, n_agents=None):
        self.n_agents = n_agents

    def columns(self, default_map):
        return []


class LaserSubgoal:
    """extras_generators.py:75-101: per agent and source of `sources` (None: every source of the world), 1.0 once the agent has
    stood on a tile of that source's beam in this episode."""

    def __init__(self, world=None, sources=None):
        self.world = world
        self.sources = None if sources is None else list(sources)
        if world is not None:
            self.columns(None)

    def columns(self, default_map):
        """[(laser_id, meaning)] of the generator's columns."""
        m = _as_map(self.world) if self.world is not None else default_map
        srcs = m.sources()
        return [(l, f"Source {l} at {(int(srcs[l].i), int(srcs[l].j))}") for l in _resolve_sources(m, self.sources)]


def _as_generator(extra):
    if isinstance(extra, (NoExtras, LaserSubgoal, MultiGenerator)):
        return extra
    if isinstance(extra, str) and extra == "laser_subgoal":  # builder.py:138-139
        return LaserSubgoal()
    raise ValueError(f"Invalid extra type: {extra}")  # builder.py:140-141


class MultiGenerator:
    """extras_generators.py:46-71: the columns of `generators` side by side."""

    def __init__(self, *generators):
        self.generators = [_as_generator(g) for g in generators]

    def add(self, *generators):
        self.generators.extend(_as_generator(g) for g in generators)

    def columns(self, default_map):
        return [c for g in self.generators for c in g.columns(default_map)]


class BatchedLLE:
    """Arguments follow `LLE.__init__` / `Builder` (python/lle/env/env.py:72-114, builder.py:30-116):
    obs_type / state_type: ObservationType values ("layered", "flattened", "partial3x3", ..., "state", "normalized-state",
    "perspective", "layered-padded[-k]"; padding_size for plain "layered-padded"); obs_dtype (the layered-style observations in float32 -- the reference's --,
    float16 or bfloat16 instead of int8, straight from the kernels); walkable_lasers; randomize_lasers;
    multi_objective (MultiObjective instead of SingleObjective); death_strategy "end" only, like the reference.
    reward_strategy / extras_generator (env.py:69-80): SingleObjective() / MultiObjective() / PotentialShapedLLE(...) and NoExtras() /
    LaserSubgoal(...) / MultiGenerator(...) / "laser_subgoal" -- the descriptors above.  With a PotentialShapedLLE the reward is
    float32 [n, 1] (shaped) or [n, 5] (MultiObjective underneath, the shaped term last; the reference's np.concat returns float64
    there, here the tensor stays float32); with an extras generator -- any, also one without columns: E = 0 -- step() returns an
    "extras" key, float32 [n, A, E].  Both come
    from ONE launch of the shaping kernel behind the step launch (lle_amd.shaping).  An environment whose step was refused
    (err != 0) keeps its positions and gets the shaped term of unchanged reached flags, gamma * potential - potential.  Without
    the two arguments nothing changes: the shaping library is not even loaded.
    cooperation=True: `env.cooperation` is a CooperationTracker (lle_amd.cooperation) -- the help edges of every environment's current
    state, their OR over its running episode and over its last finished one, each with a degree profile -- kept by ONE launch of the coop
    kernel behind every step (and behind the shaping launch where there is one), reset and set_state.  reset(mask) finishes and clears
    the selected environments and marks their reset state; set_state continues the episode with the new state; a refused step
    (err != 0) marks the unchanged state again, which only counts one more state.  Without the argument the library is not loaded.
    cooperation="temporal": a TemporalCooperationTracker (lle_amd.cooptrails) instead -- everything above plus, by ONE more small launch
    behind the coop launch, the longest trail of help edges in time order that ends at each agent: is_sequential(length), is_mutual,
    is_interdependent(2), longest_trail().  A refused step adds no state to the trails; reset and set_state do as above.
    cooperation="closed-trails": a ClosedTrailCooperationTracker (lle_amd.coopcycles) -- everything above plus, by ONE more small launch
    behind the trails launch, the set of (anchor, current, support) triples of the episode's help trails: is_interdependent(n_agents)
    for 2 <= n_agents <= 6, closed_orders().  Maps of at most 6 agents; more is a ValueError."""

    def __init__(self, maps, n_envs, obs_type="layered", state_type="state", walkable_lasers=True, randomize_lasers=False,
                 multi_objective=False, death_strategy="end", padding_size=0, device=None, seed=0, name=None, incremental_obs=False, obs_dtype=None,
                 reward_strategy=None, extras_generator=None, cooperation=False):
        if isinstance(cooperation, str) and cooperation not in ("temporal", "closed-trails"):
            raise ValueError(f"cooperation: True, False, \"temporal\" or \"closed-trails\", got {cooperation!r}")
        if cooperation == "closed-trails":  # (refused before anything is put on the device)
            first = maps[0] if isinstance(maps, (list, tuple)) else maps
            n_agents = (first if isinstance(first, _capi.Map) else _capi.Map(first)).n_agents
            if n_agents > 6:
                raise ValueError(f"cooperation=\"closed-trails\" serves maps of at most 6 agents, this one has {n_agents}; "
                                 "cooperation=\"temporal\" serves any map")
        if death_strategy == "respawn":
            raise NotImplementedError("Respawn strategy is not implemented yet")  # env.py:106-107
        if death_strategy != "end":
            raise ValueError(f"Unknown death strategy: {death_strategy}")
        self.death_strategy = DeathStrategy.END
        self._name = name
        obs_type, state_type = getattr(obs_type, "value", obs_type), getattr(state_type, "value", state_type)  # ObservationType or its string
        self.obs_type, self.state_type = str(obs_type), str(state_type)
        self._obs_kind = self._kind(self.obs_type, padding_size)
        self._state_kind = self._kind(self.state_type, padding_size)
        # obs_dtype: element type of the layered-style observations (layered, flattened, padded, perspective, partial: values -1 / 0 / 1) --
        # torch.float32 is the reference's (python/lle/observations.py:223), float16 / bfloat16 what a learner's first layer usually reads; every
        # kernel that writes them widens at the store (BatchedWorld(obs_dtype=...)).  The state vector is float32 whatever the type.
        if obs_dtype is not None and all(k[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE) for k in (self._obs_kind, self._state_kind)):
            raise ValueError("obs_dtype is the element type of the layered-style observations: obs_type and state_type are both state vectors")
        self.world = BatchedWorld(maps, n_envs, device=device, obs_dtype=obs_dtype)
        # "rgb-image": uint8 frames (the reference's), or widened at the store to the obs_dtype asked for
        self._render_dtype = self.world.obs_dtype if obs_dtype is not None and self.world.obs_dtype != torch.int8 else torch.uint8
        self.n_envs, self.n_agents, self.n_actions = self.world.n_envs, self.world.map.n_agents, 5
        # the step kernel's own (layered) observation is only written when somebody reads it
        self._needs_layered = _capi.LLE_OBS_LAYERED in (self._obs_kind[0], self._state_kind[0])
        self.walkable_lasers = bool(walkable_lasers)
        self.randomize_lasers = bool(randomize_lasers)
        if self.randomize_lasers:
            # LLE.reset draws `source.set_colour(random.randint(0, n_agents - 1))` (env.py:198-200) and set_colour raises
            # ValueError for a colour that puts another agent's start on the beam (pylaser_source.rs:121-139): on such a
            # map the reference fails at the first reset that draws the pair; a batch draws every pair at once.
            for m in self.world.maps:
                for s in m.sources():
                    for c in range(m.n_agents):
                        if not m.colour_allowed(s.laser_id, c):
                            raise ValueError(f"randomize_lasers: laser source {s.laser_id} at {(s.i, s.j)} cannot be changed to agent ID "
                                             f"{c} since it would cross the start position of another agent")
        self.multi_objective = bool(multi_objective)
        self.reward_strategy, self.extras_generator = reward_strategy, extras_generator
        self._shaping = None
        self._pbrs = reward_strategy if isinstance(reward_strategy, PotentialShapedLLE) else None
        if reward_strategy is not None:
            base = self._pbrs.strategy if self._pbrs is not None else reward_strategy
            if not isinstance(base, (SingleObjective, MultiObjective)):
                raise ValueError(f"Invalid reward strategy: {reward_strategy!r}")
            if self.multi_objective and not isinstance(base, MultiObjective):
                raise ValueError("multi_objective=True contradicts a reward_strategy over SingleObjective")
            self.multi_objective = isinstance(base, MultiObjective)
        self._extras_cols, self._extras_meanings = [], []
        if extras_generator is not None:
            cols = _as_generator(extras_generator).columns(self.world.map)
            self._extras_cols, self._extras_meanings = [c[0] for c in cols], [c[1] for c in cols]
        if self._pbrs is not None or self._extras_cols:
            from . import shaping
            self._ops = shaping
            self._shaping = shaping.Shaping(self.world, self._pbrs.laser_ids(self.world.map) if self._pbrs is not None else [], self._extras_cols,
                                            self._pbrs.gamma if self._pbrs is not None else 0.0, self._pbrs.reward_value if self._pbrs is not None else 0.0)
            self._last_reward = None
            self._shaping_reset(None)  # the batch is created reset (World::new calls reset)
        # incremental_obs: steps write only the lines of the layered rows that dynamic state can change (LLE_STEP_INCREMENTAL_OBS: the
        # others keep their bytes from the last full write) -- same observation, a third fewer bytes on level 6; the caller must not write
        # into `world.obs` itself
        self._incr = bool(incremental_obs)
        self._gen = torch.Generator(device=self.world.device)
        self._gen.manual_seed(int(seed))
        self._seed_value = int(seed)
        self._t = 0
        # auto-resets under randomize_lasers re-colour inside the step kernel (LLE_STEP_RECOLOUR_RESETS) unless a cell
        # of the map carries more than two laser layers (then: a launch of lle_batch_reset_sources per step)
        # or a beam is longer than 32 cells (the in-kernel draw is per beam word)
        self._recolour_in_step = self.randomize_lasers and all(m.max_cell_layers <= 2 and m.n_beam_words == m.n_sources for m in self.world.maps)
        self._fused = None  # output tensors + lle_env_outputs of the one-launch step (step(..., fused=True))
        # ... which also writes a partial k x k OBSERVATION itself when nobody reads the layered one, the sources are the map's own and
        # the map has at most 8 beam words (lle_batch_step_outputs: `partial`)
        self._fused_partial = (self._obs_kind[0] == _capi.LLE_OBS_PARTIAL and not self._needs_layered and not self.randomize_lasers
                               and all(m.n_beam_words <= 8 for m in self.world.maps)
                               and self._state_kind[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE, _capi.LLE_OBS_PARTIAL))
        self._bound = {}    # bound calls over persistent buffers (step(..., persistent=True)): BatchedWorld.bound_*
        self.cooperation = None
        if cooperation:
            from . import cooperation as coop
            self._coop_ops = coop
            if cooperation == "closed-trails":
                from .coopcycles import ClosedTrailCooperationTracker
                self.cooperation = ClosedTrailCooperationTracker(self.world)
            elif isinstance(cooperation, str):
                from .cooptrails import TemporalCooperationTracker
                self.cooperation = TemporalCooperationTracker(self.world)
            else:
                self.cooperation = coop.CooperationTracker(self.world)
            self._coop_temporal = isinstance(cooperation, str)
            if self.randomize_lasers and self._recolour_in_step:
                # the start edges of a map with a start cell on a laser cell depend on the colours an auto-reset draws inside the step
                # kernel (LLE_COOP_HONOUR_AUTO_RESET refuses): such an env is reset on the host ahead of the step, where the tracker
                # sees the reset state itself
                for m in self.world.maps:
                    cells = coop.cell_masks(m)
                    if any(cells[i * m.width + j] for i, j in m.positions(_capi.LLE_POS_START)):
                        self._recolour_in_step = False
            self.cooperation.update(coop.LLE_COOP_CLEAR | coop.LLE_COOP_MARK_POS)  # the batch is created reset (World::new calls reset)

    @staticmethod
    def _kind(name, padding_size):
        if name == "layered-padded":
            return (_capi.LLE_OBS_LAYERED_PADDED, int(padding_size))
        if name == "rgb-image":
            return (_RGB_IMAGE, 0)
        try:
            return _OBS_KINDS[name]
        except KeyError:
            raise ValueError(f"Unknown observation type: {name}") from None

    # ------------------------------------------------------------------ construction the reference's way (env.py:222-243, builder.py)
    @staticmethod
    def from_str(world_string):
        """`LLE.from_str(...)`: a Builder; `.build(n_envs)` makes the batch."""
        return Builder(world_string)

    @staticmethod
    def from_file(path):
        from .world import _LEVEL_NAMES
        name = str(path).lower()
        if name in _LEVEL_NAMES:  # (World.from_file takes the standard levels' names: src/core/levels.rs:10-19)
            return Builder(_capi.Map(level=_LEVEL_NAMES[name])).name(f"LLE-{os.path.basename(str(path))}")
        if not os.path.exists(path):
            raise FileNotFoundError(str(path))
        with open(path) as f:
            return Builder(f.read()).name(f"LLE-{os.path.basename(str(path))}")

    @staticmethod
    def level(level):
        """Load a predefined level between 1 and 6 (env.py:238-243)."""
        return Builder(_capi.Map(level=int(level))).name(f"LLE-lvl{level}")

    @property
    def name(self):
        return self._name if self._name is not None else "LLE"  # (marlenv's default is the class name, env.py:116-120)

    # ------------------------------------------------------------------ reward shaping and extras (lle_amd.shaping)
    @property
    def objectives(self):
        """RewardStrategy.objectives (reward_strategy.py:31,56,88,141): ends in "PBRS" with shaping over MultiObjective."""
        if self._pbrs is not None:
            return list(self._pbrs.objectives)
        return list((MultiObjective if self.multi_objective else SingleObjective).objectives)

    @property
    def extras_shape(self):
        """(E,): env.py:98."""
        return (len(self._extras_cols),)

    @property
    def extras_meanings(self):
        """env.py:99: `Source {laser_id} at {pos}` per column, the positions those of map 0."""
        return list(self._extras_meanings)

    @property
    def _shaped(self):
        return self._pbrs is not None  # (with nothing to reward -- no source, an empty list -- the kernel writes the shaped term 0)

    def _no_extras(self):
        """The extras of a generator without columns (NoExtras, LaserSubgoal on a map without sources): float32 [n, A, 0]."""
        return torch.zeros((self.n_envs, self.n_agents, 0), dtype=torch.float32, device=self.world.device)

    def _reward_width(self):
        return (5 if self._pbrs is not None else 4) if self.multi_objective else 1

    def _shaping_reset(self, env_mask):
        """RewardStrategy.reset + ExtraGenerator.reset followed by the first compute_potential / compute (env.py:194-196,203): both
        arrays cleared and marked at the start cells, for the envs with env_mask != 0.  Runs AHEAD of the world's reset: the mask may
        be the world's own `done`, which that reset rewrites."""
        sh, ops = self._shaping, self._ops
        if env_mask is not None:
            env_mask = env_mask.to(self.world.device, torch.uint8).contiguous()
        both = ops.LLE_SHAPING_CLEAR | ops.LLE_SHAPING_MARK_STARTS
        sh.update(sh.make_args(strategy_ops=both, extras_ops=both, env_mask=env_mask), self.world._stream())

    def _shaping_args(self, base, honour):
        """(args, reward, extras) of the step's shaping launch over `base` (the wrapped strategy's reward): fresh output tensors."""
        sh, ops, n, dev = self._shaping, self._ops, self.n_envs, self.world.device
        shaped = self._shaped
        reward = torch.empty((n, self._reward_width()), dtype=torch.float32, device=dev) if shaped else base
        extras = torch.empty((n, self.n_agents, len(self._extras_cols)), dtype=torch.float32, device=dev) if self._extras_cols else None
        args = sh.make_args(strategy_ops=ops.LLE_SHAPING_MARK_POS, extras_ops=ops.LLE_SHAPING_MARK_POS,
                            flags=ops.LLE_SHAPING_HONOUR_AUTO_RESET if honour else 0, reward_kind=int(self.multi_objective),
                            base_reward=base if shaped else None, reward_out=reward if shaped else None, extras_out=extras)
        return args, reward, extras

    def _shape(self, out, honour):
        """The shaping launch behind a step: `out["reward"]` becomes the shaped reward, `out["extras"]` the extras."""
        args, reward, extras = self._shaping_args(out["reward"], honour)
        self._shaping.update(args, self.world._stream())
        out["reward"] = self._last_reward = reward
        if self.extras_generator is not None:
            out["extras"] = extras if extras is not None else self._no_extras()
        return out

    def _finish(self, out, honour):
        """What step() returns: `out` as it always was without the two arguments; with them the shaped reward and the "extras" key --
        the key whenever a generator was given, [n, A, 0] where it has no column."""
        if self._shaping is not None:
            out = self._shape(out, honour)
        elif self.extras_generator is not None:
            out["extras"] = self._no_extras()
        if self.cooperation is not None:
            self._coop_step(honour)
        return out

    def _coop_step(self, honour):
        """The coop launch behind a step (and behind its shaping launch): the new state is one more state of every environment's
        episode; an environment the step kernel reset first finishes its episode and starts the next at the map's start edges."""
        if self._coop_temporal:  # (the trails launch behind it: an environment whose step was refused has no new state)
            self.cooperation.update(self._coop_ops.LLE_COOP_MARK_POS, honour_auto_reset=honour, skip_refused=True)
        else:
            self.cooperation.update(self._coop_ops.LLE_COOP_MARK_POS, honour_auto_reset=honour)

    def extras(self):
        """ExtraGenerator.compute (extras_generators.py:93-98; Observation.extras of get_observation, env.py:218-223) for every env:
        float32 [n, A, E] -- the agents are marked at their current positions first.  E = 0 without a generator."""
        n, dev = self.n_envs, self.world.device
        if not self._extras_cols:
            return self._no_extras()
        out = torch.empty((n, self.n_agents, len(self._extras_cols)), dtype=torch.float32, device=dev)
        sh = self._shaping
        sh.update(sh.make_args(extras_ops=self._ops.LLE_SHAPING_MARK_POS, extras_out=out), self.world._stream())
        return out

    def __del__(self):
        sh = getattr(self, "_shaping", None)
        if sh is not None:
            sh.free()
        tracker = getattr(self, "cooperation", None)
        if tracker is not None:
            tracker.free()

    # ------------------------------------------------------------------ static description (env.py:72-143)
    @property
    def width(self):
        return self.world.map.width

    @property
    def height(self):
        return self.world.map.height

    @property
    def observation_shape(self):
        """Per-env shape of `get_observation()` (the reference's `observation_shape`, without its tiled agent axis for the
        kinds whose agents all see the same tensor)."""
        return tuple(self._shape_of(self._obs_kind, self.obs_type, state=False))

    @property
    def state_shape(self):
        """LLE.state_shape = get_state().shape (env.py:96): the state generator's observation of agent 0."""
        return tuple(self._shape_of(self._state_kind, self.state_type, state=True))

    def _shape_of(self, kind, name, state):
        k, p = kind
        m, A = self.world.map, self.n_agents
        if k in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE):
            return [3 * A + m.n_gems]
        if k == _RGB_IMAGE:  # (RGBImage.shape is the frame; the observation tiles it per agent, the state is agent 0's)
            frame = [32 * m.height + 1, 32 * m.width + 1, 3]
            return frame if state else [A] + frame
        d = self.world.obs_desc(k, p)
        shape = [int(d.shape[i]) for i in range(1, d.ndim)]
        if state and k in (_capi.LLE_OBS_PARTIAL, _capi.LLE_OBS_PERSPECTIVE):
            shape = shape[1:]  # agent 0's slice
        if name == "flattened":
            n = 1
            for v in shape:
                n *= v
            return [n]
        return shape

    @property
    def agent_state_size(self):
        """StateGenerator.unit_size = 2 (i, j per agent; observations.py:174); other state types have none (env.py:135-140)."""
        if self._state_kind[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE):
            return 2
        raise NotImplementedError(f"State type {self.state_type} does not support `agent_state_size`.")

    # ------------------------------------------------------------------ LLE API, batched
    def seed(self, seed_value):
        """LLE.seed (env.py:245-247): seeds the colour randomisation (v1 maps have a single start per agent)."""
        self._gen.manual_seed(int(seed_value))
        self._seed_value = int(seed_value)
        # the persistent step's bound calls carry the seed of the in-kernel colour draws: bind them again with the new one
        for key in [k for k in self._bound if isinstance(k, tuple) and k[0] == "step"]:
            del self._bound[key]

    @property
    def done(self):
        """bool [n]: LLE.compute_done (env.py:253-254) -- every agent arrived, or somebody died."""
        return self.world.done.view(torch.bool)  # the kernel writes 0 / 1: a view, no launch

    def compute_done(self):
        return self.done

    @property
    def n_arrived(self):
        """int64 [n]: RewardStrategy.n_arrived (reward_strategy.py:22-25,33-39) = agents that have reached an exit this episode."""
        arrived = (self.world.bits >> 16) & 0xFFFF
        return sum((arrived >> a) & 1 for a in range(self.n_agents))

    def reset(self, env_mask=None, seed=None, colours=None):
        """LLE.reset (env.py:189-203) for every env, or those with env_mask != 0: world.reset(), then -- with
        randomize_lasers -- a fresh colour in [0, n_agents) for every source (`colours` u8 [n, L] overrides the draw)."""
        if seed is not None:
            self.seed(seed)
        self._reset_world(env_mask, colours)
        return self._obs_and_state()

    def _reset_world(self, env_mask, colours=None, write_obs=True):
        """world.reset() and, with randomize_lasers, the recolouring of the same envs: one launch either way
        (lle_batch_reset or lle_batch_reset_sources)."""
        w = self.world
        if self._shaping is not None:
            self._shaping_reset(env_mask)
        if self.cooperation is not None and env_mask is not None:
            env_mask = env_mask.to(w.device, torch.uint8).clone()  # (the mask may be the world's own `done`, which the reset rewrites)
        if self.randomize_lasers or colours is not None:
            if colours is None:
                colours = torch.randint(0, self.n_agents, (self.n_envs, w.map.n_sources), generator=self._gen,
                                        device=w.device, dtype=torch.uint8)
            w.set_sources(colours=colours, env_mask=env_mask, reset_first=True, write_obs=write_obs)
        else:
            w.reset(env_mask)
        if self.cooperation is not None:
            self.cooperation.reset(env_mask)  # FINISH | CLEAR, then MARK_POS on the reset state

    def set_state(self, positions, gems_collected, agents_alive=None):
        """LLE.set_state (env.py:208-217) for every env: World.set_state with the reference's semantics (lossy
        re-derivation of the beams, InvalidWorldState rules); `done` is recomputed from the new state.  positions u8
        [n, A, 2], gems_collected bool [n, G], agents_alive bool [n, A] (default: all alive).  Returns the per-env error
        codes (0, or LLE_ENV_*; such an env keeps / gets the state World.set_state leaves it in)."""
        w = self.world
        if agents_alive is None:
            agents_alive = torch.ones((self.n_envs, self.n_agents), dtype=torch.bool, device=w.device)
        if self._shaping is not None and self._shaped:
            # reward_strategy.reset() -- cleared, marked where the agents stand BEFORE the call -- then compute_reward(events) marks
            # them where they stand after it (env.py:213-215); the extras generator is not touched until it computes next
            sh, ops = self._shaping, self._ops
            sh.update(sh.make_args(strategy_ops=ops.LLE_SHAPING_CLEAR | ops.LLE_SHAPING_MARK_POS), w._stream())
            w.set_state(positions, gems_collected, agents_alive)
            sh.update(sh.make_args(strategy_ops=ops.LLE_SHAPING_MARK_POS), w._stream())
        else:
            w.set_state(positions, gems_collected, agents_alive)
        if self.cooperation is not None:
            self.cooperation.mark()  # the episode continues with the new state
        return w.err

    def agents_alive(self):
        """bool [n, A]: the `is-alive-k` entries of Step.info (env.py:174-176)."""
        return ((self.world.bits.unsqueeze(1) >> torch.arange(self.n_agents, device=self.world.device)) & 1).bool()

    def agents_arrived(self):
        """bool [n, A]: the `has-arrived-k` entries of Step.info."""
        return ((self.world.bits.unsqueeze(1) >> (16 + torch.arange(self.n_agents, device=self.world.device))) & 1).bool()

    def _observe(self, kind):
        k, p = kind
        if k == _capi.LLE_OBS_LAYERED:
            return self.world.obs  # written by the step / reset / set_sources kernel itself
        if k == _RGB_IMAGE:
            return self.world.render(dtype=self._render_dtype)  # (n, 32H+1, 32W+1, 3): one launch of the render kernel
        return self.world.observe_as(k, p)

    def get_image(self, env=0):
        """LLE.get_image (python/lle/env/env.py:250-251) of environment `env`: numpy uint8 (32H+1, 32W+1, 3)."""
        img = self.world.render(env_ids=[int(env)])[0]
        torch.cuda.synchronize(self.world.device)
        return img.cpu().numpy()

    def _bound_render(self):
        """A zero-argument callable rendering every env into ONE persistent buffer (`call.out`, overwritten by every call)."""
        w, dt = self.world, self._render_dtype
        d = w.render_desc(dtype=dt)
        buf = torch.empty(int(d.bytes) + 256, dtype=torch.uint8, device=w.device)
        buf = buf[(-buf.data_ptr()) % 256:][: int(d.bytes)]

        def call():
            return w.render(out=buf, dtype=dt)
        call.out = torch.as_strided(buf.view(dt), [int(d.shape[q]) for q in range(4)], [int(d.stride[q]) for q in range(4)])
        return call

    def _bind_observer(self, kind):
        return self._bound_render() if kind[0] == _RGB_IMAGE else self.world.bound_observer(*kind)

    def get_observation(self):
        """The observation of every env with the reference's per-env shape behind the env axis.  Kinds whose agents all
        see the same tensor carry ONE copy (the reference tiles it n_agents times, observations.py:151,266):
        broadcast with `.unsqueeze(1).expand(-1, n_agents, ...)` if the learner wants the tiled layout."""
        obs = self._observe(self._obs_kind)
        if self._obs_kind[0] == _RGB_IMAGE:  # (n, A, 32H+1, 32W+1, 3): the frame broadcast over the agents (observations.py:183-185)
            return obs.unsqueeze(1).expand(-1, self.n_agents, -1, -1, -1)
        return obs.flatten(1) if self.obs_type == "flattened" else obs

    def _obs_and_state(self, state=None):
        """(get_observation(), get_state()) -- or `state` when the caller already has it.  With obs_type == state_type == "rgb-image"
        ONE render launch serves both: the state is the frame, the observation the same frame broadcast over the agents."""
        if state is None and self._obs_kind[0] == _RGB_IMAGE and self._state_kind == self._obs_kind:
            frame = self._observe(self._obs_kind)
            return frame.unsqueeze(1).expand(-1, self.n_agents, -1, -1, -1), frame
        return self.get_observation(), (state if state is not None else self.get_state())

    def get_state(self):
        """LLE.get_state (env.py:205-206): the state generator's observation of agent 0."""
        if self._state_kind[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE):
            w = self.world
            st = torch.empty((self.n_envs, 3 * self.n_agents + w.map.n_gems), dtype=torch.float32, device=w.device)
            w.env_outputs(state=st, normalize_state=self._state_kind[0] == _capi.LLE_OBS_NORMALIZED_STATE)
            return st
        st = self._observe(self._state_kind)
        if self._state_kind[0] in (_capi.LLE_OBS_PARTIAL, _capi.LLE_OBS_PERSPECTIVE):
            st = st[:, 0]
        return st.flatten(1) if self.state_type == "flattened" else st

    def available_actions(self):
        """LLE.available_actions (env.py:146-163): bool [n, n_agents, 5]."""
        return self.world.available_actions(self.walkable_lasers)

    def reward(self):
        """Reward of the last step: SingleObjective float32 [n, 1] or MultiObjective float32 [n, 4]
        (reward_strategy.py:58-75, 90-109)."""
        if self._pbrs is not None:  # (the shaped term is a function of the reached flags BEFORE the step: kept from the step itself)
            if self._last_reward is None:
                raise RuntimeError("reward() under PotentialShapedLLE returns the reward of the last step(): there has been none")
            return self._last_reward
        reward = torch.empty((self.n_envs, 4 if self.multi_objective else 1), dtype=torch.float32, device=self.world.device)
        self.world.env_outputs(reward=reward, multi_objective=self.multi_objective)
        return reward

    def _fresh_outputs(self):
        """(tensors, struct) for ONE step of the one-launch path: like _fused_outputs, allocated anew (the struct travels in the
        launch's kernel arguments: 21.04 us per step against 21.02 with persistent tensors)."""
        keep, self._fused = self._fused, None
        try:
            return self._fused_outputs()
        finally:
            self._fused = keep

    def _fused_outputs(self):
        """Persistent output tensors of the one-launch step and the struct over them (lle_batch_step_outputs passes the struct in the kernel arguments)."""
        if self._fused is None:
            w, n, dev = self.world, self.n_envs, self.world.device
            fused_state = self._state_kind[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE)
            t = {"state": torch.empty((n, 3 * self.n_agents + w.map.n_gems), dtype=torch.float32, device=dev) if fused_state else None,
                 "reward": torch.empty((n, 4 if self.multi_objective else 1), dtype=torch.float32, device=dev),
                 "available": torch.empty((n, self.n_agents, 5), dtype=torch.uint8, device=dev), "partial": None, "partial_buf": None}
            kw = {}
            if self._fused_partial:
                # the partial k x k observation written by the step launch itself (lle_batch_step_outputs, step kernel MODE 9)
                t["partial_buf"], t["partial"] = w.partial_buffer(self._obs_kind[1])
                kw = dict(partial=t["partial_buf"], partial_k=self._obs_kind[1])
            o = w.make_env_outputs(state=t["state"], normalize_state=self._state_kind[0] == _capi.LLE_OBS_NORMALIZED_STATE, reward=t["reward"],
                                   multi_objective=self.multi_objective, available=t["available"], walkable_lasers=True, **kw)
            self._fused = (t, o)
        return self._fused

    def step(self, actions, auto_reset=False, fused=None, persistent=False):
        """LLE.step (env.py:165-187) for every env.  actions: integer tensor [n, n_agents] (Action values).
        By default (fused=None) state / reward / available_actions are written by the step kernel itself (lle_batch_step_outputs:
        ONE launch per step, 21.1 us at 65 536 level-6 envs against 25.1 in two) into tensors allocated for this step -- whenever
        that kernel can serve the env (walkable_lasers; the partial observation too where step kernel MODE 9 covers the map);
        otherwise in two launches.  fused=False forces the two launches (step, then lle_batch_env_outputs).
        fused=True (needs walkable_lasers): the one launch into PERSISTENT tensors that the next step overwrites (no allocation
        per step).
        persistent=True: the two-launch step (any walkable_lasers, any observation / state type) through calls bound once
        (BatchedWorld.bound_*) into persistent tensors that the next step overwrites: the host side of a step is two C-ABI
        calls (three with an observation type other than layered) instead of allocations, descriptor queries and views.
        The reference refuses to step a finished environment (`Cannot step in a done environment`); here such an env
        is the caller's to reset -- or pass auto_reset=True: an env that is done when the step starts is reset first
        (with fresh colours under randomize_lasers), the usual vector-env convention.
        The step kernel's layered observation (`world.obs`) is only refreshed when obs_type or state_type is layered.
        Returns a dict of device tensors: obs, state, reward, done, available_actions, err (per-env error code of
        World.step: 0 or 1 + the agent whose action was not available, the env then being left untouched)."""
        w = self.world
        if actions.dtype is not torch.uint8 or actions.device != w.device or not actions.is_contiguous():
            actions = actions.to(w.device, torch.uint8).contiguous()
        if fused and not self.walkable_lasers:
            raise ValueError("the one-launch step writes available_actions with walkable_lasers only")
        if persistent and not fused:
            return self._step_persistent(actions, auto_reset)
        fresh = None
        if fused is None:  # the default: one launch where the step kernel can write the outputs, into this step's own tensors
            fused = False
            if self.walkable_lasers:
                fresh = self._fresh_outputs()
        env_out = fresh[1] if fresh is not None else (self._fused_outputs()[1] if fused else None)
        # envs the step kernel resets itself are recognised by the shaping launch (LLE_BUF_EVCOUNT bit 7); a host-side reset
        # (_reset_world) resets the shaping state itself
        honour = bool(auto_reset) and (self._recolour_in_step or not self.randomize_lasers)
        if auto_reset:
            if self._recolour_in_step:
                # world.reset() + a fresh colour per source for the envs that are over, inside the step kernel; the draws
                # are keyed by (seed, env, step counter, source), not by the torch generator that reset() uses
                w.step(actions, auto_reset=True, recolour_resets=True, seed=self._seed_value, t=self._t, write_obs=self._needs_layered,
                       env_out=env_out, incremental_obs=self._incr)
            elif self.randomize_lasers:
                # (the kernel reads an env's mask byte before it rewrites its `done`; the step rewrites the observation)
                self._reset_world(w.done, write_obs=False)
                w.step(actions, write_obs=self._needs_layered, env_out=env_out, incremental_obs=self._incr)
            else:
                w.step(actions, auto_reset=True, write_obs=self._needs_layered, env_out=env_out, incremental_obs=self._incr)
        else:
            w.step(actions, write_obs=self._needs_layered, env_out=env_out, incremental_obs=self._incr)
        self._t += 1
        if fused or fresh is not None:
            t = fresh[0] if fresh is not None else self._fused[0]
            if t["partial"] is not None:  # (written by the step launch: no observer launch behind it)
                obs = t["partial"]
                state = t["state"] if t["state"] is not None else (obs[:, 0] if self._state_kind == self._obs_kind else self.get_state())
                if t["state"] is None and self.state_type == "flattened":
                    state = state.flatten(1)
            else:
                obs, state = self._obs_and_state(t["state"])
            out = {"obs": obs, "state": state, "reward": t["reward"],
                   "done": self.done, "available_actions": t["available"].view(torch.bool), "err": w.err}
            return self._finish(out, honour)
        return self._finish(self._outputs(), honour)

    def _step_persistent(self, actions, auto_reset):
        """step(persistent=True): see step()."""
        w, b = self.world, self._bound
        key = ("step", bool(auto_reset))
        if key not in b:
            n, dev = self.n_envs, w.device
            plain_state = self._state_kind[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE)
            if "outs" not in b:
                t = {"state": torch.empty((n, 3 * self.n_agents + w.map.n_gems), dtype=torch.float32, device=dev) if plain_state else None,
                     "reward": torch.empty((n, 4 if self.multi_objective else 1), dtype=torch.float32, device=dev),
                     "available": torch.empty((n, self.n_agents, 5), dtype=torch.uint8, device=dev)}
                b["outs"] = (t, w.bound_env_outputs(state=t["state"], normalize_state=self._state_kind[0] == _capi.LLE_OBS_NORMALIZED_STATE,
                                                    reward=t["reward"], multi_objective=self.multi_objective, available=t["available"],
                                                    walkable_lasers=self.walkable_lasers))
                b["obs"] = None if self._obs_kind[0] == _capi.LLE_OBS_LAYERED else self._bind_observer(self._obs_kind)
                b["state"] = None if plain_state or self._state_kind[0] == _capi.LLE_OBS_LAYERED else (
                    b["obs"] if self._state_kind == self._obs_kind and b["obs"] is not None else self._bind_observer(self._state_kind))
            recolour = auto_reset and self._recolour_in_step
            in_kernel_reset = auto_reset and (recolour or not self.randomize_lasers)
            b[key] = w.bound_step(auto_reset=in_kernel_reset, recolour_resets=recolour, write_obs=self._needs_layered, seed=self._seed_value,
                                  incremental_obs=self._incr)
        if auto_reset and self.randomize_lasers and not self._recolour_in_step:
            self._reset_world(w.done, write_obs=False)
        w.t = self._t
        b[key](actions)
        self._t += 1
        t, outs = b["outs"]
        outs()
        obs = w.obs if b["obs"] is None else b["obs"]()
        if self.obs_type == "flattened":
            obs = obs.flatten(1)
        if self._obs_kind[0] == _RGB_IMAGE:
            obs = obs.unsqueeze(1).expand(-1, self.n_agents, -1, -1, -1)
        if t["state"] is not None:
            state = t["state"]
        elif b["state"] is None:
            state = w.obs
        else:
            state = b["state"].out if b["state"] is b["obs"] else b["state"]()
            if self._state_kind[0] in (_capi.LLE_OBS_PARTIAL, _capi.LLE_OBS_PERSPECTIVE):
                state = state[:, 0]
        if t["state"] is None and self.state_type == "flattened":
            state = state.flatten(1)
        out = {"obs": obs, "state": state, "reward": t["reward"], "done": self.done, "available_actions": t["available"].view(torch.bool),
               "err": w.err}
        if self._shaping is not None:
            # the shaping call bound once, into persistent tensors that the next step overwrites
            skey = ("shape", bool(auto_reset and (self._recolour_in_step or not self.randomize_lasers)))
            if skey not in b:
                b[skey] = self._shaping_args(t["reward"], skey[1])
            args, reward, extras = b[skey]
            self._shaping.update(args, _current_stream_handle(w.device))
            out["reward"] = self._last_reward = reward
            if self.extras_generator is not None:
                out["extras"] = extras if extras is not None else self._no_extras()
        elif self.extras_generator is not None:
            out["extras"] = self._no_extras()
        if self.cooperation is not None:
            self._coop_step(bool(auto_reset and (self._recolour_in_step or not self.randomize_lasers)))
        return out

    def _outputs(self):
        """obs / state / reward / done / available_actions / err after a step: one launch of lle_batch_env_outputs for
        the small tensors (the layered observation was written by the step kernel itself); only a state type other than
        "state" / "normalized-state" or an observation type other than layered costs a further observer launch.
        The tensors are freshly allocated except `obs` (layered), `done` and `err`, which view the world's buffers."""
        w, n, dev = self.world, self.n_envs, self.world.device
        fused_state = self._state_kind[0] in (_capi.LLE_OBS_STATE, _capi.LLE_OBS_NORMALIZED_STATE)
        state = torch.empty((n, 3 * self.n_agents + w.map.n_gems), dtype=torch.float32, device=dev) if fused_state else None
        reward = torch.empty((n, 4 if self.multi_objective else 1), dtype=torch.float32, device=dev)
        avail = torch.empty((n, self.n_agents, 5), dtype=torch.uint8, device=dev)
        w.env_outputs(state=state, normalize_state=self._state_kind[0] == _capi.LLE_OBS_NORMALIZED_STATE, reward=reward,
                      multi_objective=self.multi_objective, available=avail, walkable_lasers=self.walkable_lasers)
        obs, state = self._obs_and_state(state if fused_state else None)
        return {"obs": obs, "state": state, "reward": reward, "done": self.done, "available_actions": avail.view(torch.bool), "err": w.err}


class Builder:
    """`lle.level(6).obs_type("layered").randomize_lasers().build()` of the reference (python/lle/env/builder.py:12-166), for the
    batch: the same chain, and `build(n_envs)` returns a BatchedLLE.  `pbrs` and `add_extras` still refuse: reward shaping and extras
    enter as `build(n_envs, reward_strategy=PotentialShapedLLE(...), extras_generator=LaserSubgoal(...))`, the way LLE.__init__ takes them."""

    def __init__(self, map_or_text):
        self._map = map_or_text
        self._obs_type, self._state_type = "layered", "state"
        self._death_strategy, self._walkable_lasers = "end", True
        self._env_name, self._multi_objective, self._randomize_lasers = "LLE", False, False
        self._padding_size = 0

    def obs_type(self, obs_type):
        from .observations import ObservationType
        self._obs_type = ObservationType.from_str(obs_type).value if isinstance(obs_type, str) else obs_type.value
        return self

    def state_type(self, state_type):
        from .observations import ObservationType
        self._state_type = ObservationType.from_str(state_type).value if isinstance(state_type, str) else state_type.value
        return self

    def walkable_lasers(self, walkable_lasers):
        self._walkable_lasers = bool(walkable_lasers)
        return self

    def death_strategy(self, death_strategy):
        self._death_strategy = death_strategy
        return self

    def name(self, name):
        self._env_name = name
        return self

    def multi_objective(self):
        if not self._multi_objective:
            self._multi_objective = True
            self._env_name = f"{self._env_name}-MO"  # builder.py:74-76
        return self

    def randomize_lasers(self):
        self._randomize_lasers = True
        return self

    def pbrs(self, *args, **kwargs):
        raise NotImplementedError("Builder.pbrs is not implemented: pass reward_strategy=PotentialShapedLLE(SingleObjective(), gamma=..., reward_value=..., "
                                  "lasers_to_reward=...) (and extras_generator=LaserSubgoal(...)) to build() or to BatchedLLE")

    def add_extras(self, *extras):
        if not extras:
            return self
        raise NotImplementedError("Builder.add_extras is not implemented: pass extras_generator=LaserSubgoal(...) or \"laser_subgoal\" to build() or to BatchedLLE")

    def build(self, n_envs=1, device=None, seed=0, obs_dtype=None, reward_strategy=None, extras_generator=None, cooperation=False):
        """(n_envs, device, seed, obs_dtype, cooperation: what a batch needs beyond the reference's builder -- BatchedLLE's arguments of the
        same names; reward_strategy, extras_generator: LLE.__init__'s, env.py:69-80)"""
        return BatchedLLE(self._map, n_envs, obs_type=self._obs_type, state_type=self._state_type, walkable_lasers=self._walkable_lasers,
                          randomize_lasers=self._randomize_lasers, multi_objective=self._multi_objective, death_strategy=self._death_strategy,
                          padding_size=self._padding_size, device=device, seed=seed, name=self._env_name, obs_dtype=obs_dtype,
                          reward_strategy=reward_strategy, extras_generator=extras_generator, cooperation=cooperation)


def level(level):
    """`lle.level(n)` (python/lle/__init__.py)."""
    return BatchedLLE.level(level)


def from_str(world_string):
    return BatchedLLE.from_str(world_string)


def from_file(path):
    return BatchedLLE.from_file(path)
