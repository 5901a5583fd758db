"""ctypes binding of liblle_coopcycles.so (lle_amd/coopcycles/coopcycles.hip, C ABI include/lle_coopcycles.h; INTEGRATION.md section
23) and `ClosedTrailCooperationTracker`: which closed trails of help the episode of every environment holds.

`TemporalCooperationTracker.is_interdependent(n_agents >= 3)` raises: neither the flattened edges nor the trail lengths decide whether
some closed trail of help edges in time order visits exactly n_agents agents (PlanProfile.is_interdependent,
python/lle/characterization/plan/profile.py).  The set of (anchor, current, support) triples of the episode does -- the value the
closed-trail search keeps per record, DESIGN.md sections 4.16 and 4.18 -- and one more small launch behind the trails launch keeps it.

    env = BatchedLLE(Map(level=6), 65536, cooperation="closed-trails")
    env.reset(); env.step(actions, auto_reset=True)
    env.cooperation.is_interdependent(3, last=True)   # bool [n]: the last finished episode closed a trail over exactly 3 agents
    env.cooperation.closed_orders()                   # uint8 [n]: bit k = the running episode closed a trail over exactly k agents

Maps of at most 6 agents.  The module is loaded only when such a tracker is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _binding, cooperation
from ._binding import UpdateArgs  # lle_coopcycles_update_args: the layout of lle_coop_update_args
from .cooptrails import TemporalCooperationTracker

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_coopcycles.so")

# enums of include/lle_coopcycles.h
LLE_COOPCYCLES_FINISH, LLE_COOPCYCLES_CLEAR, LLE_COOPCYCLES_MARK_STARTS, LLE_COOPCYCLES_MARK_POS = 1, 2, 4, 8
LLE_COOPCYCLES_HONOUR_AUTO_RESET, LLE_COOPCYCLES_SKIP_REFUSED = 1, 2
LLE_COOPCYCLES_EPISODE_CLOSED, LLE_COOPCYCLES_LAST_CLOSED, LLE_COOPCYCLES_EPISODE_CPROFILE, LLE_COOPCYCLES_LAST_CPROFILE = range(4)
LLE_COOPCYCLES_MAX_AGENTS, LLE_COOPCYCLES_SMALL_WORDS, LLE_COOPCYCLES_LARGE_WORDS, LLE_COOPCYCLES_WALK_BUDGET = 6, 3, 21, 4096
# bytes of a closed-trail profile row
C_ORDERS, C_STATES, C_DENSE, C_VALID = range(4)

EXPORTS = ["lle_coopcycles_create", "lle_coopcycles_update_map", "lle_coopcycles_free", "lle_coopcycles_update", "lle_coopcycles_buffer",
           "lle_coopcycles_last_error", "lle_coopcycles_debug_launched", "lle_coopcycles_debug_compiled"]


_lib = None


def lib():
    """Load liblle_coopcycles.so (after liblle_hip.so and liblle_coop.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    cooperation.lib()
    L = _binding.load(LIB_PATH, "the closed-trail cooperation tracker")
    vp = C.c_void_p
    _binding.tracker_signatures(L, "lle_coopcycles", [vp, vp, vp], [vp, C.c_int, vp])
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_coopcycles.so this process has launched (lle_coopcycles_debug_launched)."""
    return _binding.names(lib().lle_coopcycles_debug_launched)


def compiled_kernels():
    """Every instantiation the library holds (lle_coopcycles_debug_compiled)."""
    return _binding.names(lib().lle_coopcycles_debug_compiled)


def words_of(n_agents):
    """Words of a value: 3 for maps of up to 4 agents, 21 for 5 or 6."""
    return LLE_COOPCYCLES_SMALL_WORDS if n_agents <= 4 else LLE_COOPCYCLES_LARGE_WORDS


class ClosedTrailCooperationTracker(TemporalCooperationTracker):
    """A TemporalCooperationTracker with one lle_coopcycles behind it: every update / mark / reset issues the coop launch, the trails
    launch and then the coopcycles launch with the same arguments.  Further attributes (torch tensors, VIEWS of the handle's device
    memory, valid until free()):
      episode_closed, last_closed       int32 [W, n]: the packed (anchor, current, support) triples of include/lle_cycles.h, word-major
                                        (W = 3 for maps of up to 4 agents, else 21) -- of the running episode, of the last finished one
      episode_cprofile, last_cprofile   uint8 [n, 4]: closed orders as a bit set (bit k: some closed trail visits exactly k agents),
                                        states whose arcs entered the walk (saturating), dense, valid"""

    def __init__(self, batched_world):
        n_agents = int(batched_world.map.n_agents)
        if n_agents > LLE_COOPCYCLES_MAX_AGENTS:
            raise ValueError(f"cooperation=\"closed-trails\" serves maps of at most {LLE_COOPCYCLES_MAX_AGENTS} agents, this one has {n_agents}")
        self.ch = None
        super().__init__(batched_world)
        L = lib()
        self.ch = L.lle_coopcycles_create(self.world.h, self.h, self.world._stream())
        if not self.ch:
            raise RuntimeError(f"lle_coopcycles_create failed: {L.lle_coopcycles_last_error().decode()}")
        self._closed_update = L.lle_coopcycles_update
        n, self.n_words = self.n_envs, words_of(self.n_agents)
        self.episode_closed = self._closed_view(LLE_COOPCYCLES_EPISODE_CLOSED, (self.n_words, n), "<i4")
        self.last_closed = self._closed_view(LLE_COOPCYCLES_LAST_CLOSED, (self.n_words, n), "<i4")
        self.episode_cprofile = self._closed_view(LLE_COOPCYCLES_EPISODE_CPROFILE, (n, 4), "|u1")
        self.last_cprofile = self._closed_view(LLE_COOPCYCLES_LAST_CPROFILE, (n, 4), "|u1")

    def _closed_view(self, which, shape, typestr):
        return _binding.tracker_view(lib(), "lle_coopcycles", self.ch, which, shape, typestr, self.world.device)

    def _closed_check(self, rc):
        _binding.tracker_check(lib(), "lle_coopcycles", rc)

    # ------------------------------------------------------------------ updates
    def make_closed_args(self, ops, honour_auto_reset=False, env_mask=None, skip_refused=False):
        """An lle_coopcycles_update_args; the caller keeps `env_mask` (a uint8 device tensor) alive."""
        flags = (LLE_COOPCYCLES_HONOUR_AUTO_RESET if honour_auto_reset else 0) | (LLE_COOPCYCLES_SKIP_REFUSED if skip_refused else 0)
        return UpdateArgs(C.sizeof(UpdateArgs), int(ops), flags, 0, None if env_mask is None else env_mask.data_ptr())

    def launch_closed(self, args, stream=None):
        """The coopcycles launch ALONE: it reads LLE_COOP_STEP_EDGES as the last coop launch left it."""
        rc = self._closed_update(self.ch, C.byref(args), self.world._stream() if stream is None else stream)
        if rc != 0:
            self._closed_check(rc)

    def update(self, ops=cooperation.LLE_COOP_MARK_POS, honour_auto_reset=False, env_mask=None, env_sources=None, skip_refused=False):
        """One lle_coop_update, one lle_cooptrails_update and, behind them on the same stream, one lle_coopcycles_update with the same
        operations, flags and mask.  (mark() and reset() come here.)"""
        super().update(ops, honour_auto_reset=honour_auto_reset, env_mask=env_mask, env_sources=env_sources, skip_refused=skip_refused)
        self.launch_closed(self.make_closed_args(ops, honour_auto_reset, self._mask, skip_refused))

    def update_map(self, map_index=0):
        super().update_map(map_index)
        self._closed_check(lib().lle_coopcycles_update_map(self.ch, int(map_index), self.world._stream()))

    # ------------------------------------------------------------------ the closed-trail queries (profile.py), per environment
    def _cprofile(self, last):
        return self.last_cprofile if last else self.episode_cprofile

    def closed_orders(self, last=False):
        """uint8 [n]: bit k (2 <= k <= 6) = some closed trail of the episode visits exactly k distinct agents."""
        return self._cprofile(last)[:, C_ORDERS]

    def closed_exact(self, last=False):
        """bool [n]: no layer of the episode was dropped for running out of its budget -- the absences are certain too."""
        return self._cprofile(last)[:, C_DENSE] == 0

    def is_interdependent(self, n_agents=2, last=False):
        """bool [n]: some closed trail visits exactly n_agents distinct agents (PlanProfile.is_interdependent), from the bit set; False
        below 2, above the map's agents and where the row is not valid."""
        import torch
        p = self._cprofile(last)
        n_agents = int(n_agents)
        if n_agents < 2 or n_agents > self.n_agents:
            return torch.zeros(self.n_envs, dtype=torch.bool, device=p.device)
        return (p[:, C_VALID] != 0) & (((p[:, C_ORDERS] >> n_agents) & 1) != 0)

    def is_mutual(self, last=False):
        """bool [n]: PlanProfile.is_mutual = is_interdependent(2)."""
        return self.is_interdependent(2, last)

    def triples(self, env, last=False):
        """Host set of (anchor, current, frozenset of agents) of environment `env` (synchronises): the decode of lle_amd.cycles.triples,
        for debugging and for tests."""
        from .cycles import triples
        value = self.last_closed if last else self.episode_closed
        return triples([int(w) & 0xFFFFFFFF for w in value[:, int(env)].cpu().tolist()], self.n_agents)

    def free(self):
        if getattr(self, "ch", None):
            try:
                lib().lle_coopcycles_free(self.ch)  # (before the trails and the coop handle: it reads the coop handle's arrays)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.ch = None
        super().free()
