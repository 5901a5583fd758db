"""ctypes binding of liblle_cooptrails.so (lle_amd/cooptrails/cooptrails.hip, C ABI include/lle_cooptrails.h; INTEGRATION.md section
20) and `TemporalCooperationTracker`: how deep the cooperation of every environment's episode is.

The flattened queries of `CooperationTracker` (is_cooperative, is_asymmetric, is_convergent, is_divergent) forget WHEN an agent helped.
The temporal half of the reference's PlanProfile (python/lle/characterization/plan/profile.py) does not: is_sequential(length) asks for
a trail of `length` help edges in time order.  One small vector per environment decides it -- the longest trail that ends at each
agent, DESIGN.md sections 4.13 and 4.15 -- and one more small launch behind the coop launch keeps it.

    env = BatchedLLE(Map(level=6), 65536, cooperation="temporal")
    env.reset(); env.step(actions, auto_reset=True)
    env.cooperation.is_sequential(2, last=True)   # bool [n]: the last finished episode had a chain of two help events
    env.cooperation.longest_trail()               # uint8 [n]: of the running episode, saturating at 15

The module is loaded only when such a tracker is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os

from . import _binding, cooperation
from ._binding import UpdateArgs  # lle_cooptrails_update_args: the layout of lle_coop_update_args
from .cooperation import CooperationTracker

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_cooptrails.so")

# enums of include/lle_cooptrails.h
LLE_COOPTRAILS_FINISH, LLE_COOPTRAILS_CLEAR, LLE_COOPTRAILS_MARK_STARTS, LLE_COOPTRAILS_MARK_POS = 1, 2, 4, 8
LLE_COOPTRAILS_HONOUR_AUTO_RESET, LLE_COOPTRAILS_SKIP_REFUSED = 1, 2
LLE_COOPTRAILS_EPISODE_TRAILS, LLE_COOPTRAILS_LAST_TRAILS, LLE_COOPTRAILS_EPISODE_TPROFILE, LLE_COOPTRAILS_LAST_TPROFILE = range(4)
LLE_COOPTRAILS_SATURATED, LLE_COOPTRAILS_WALK_BUDGET = 15, 4096
# bytes of a temporal profile row
T_LONGEST, T_STATES, T_DENSE, T_VALID = range(4)

EXPORTS = ["lle_cooptrails_create", "lle_cooptrails_update_map", "lle_cooptrails_free", "lle_cooptrails_update", "lle_cooptrails_buffer",
           "lle_cooptrails_last_error", "lle_cooptrails_debug_launched", "lle_cooptrails_debug_compiled"]


_lib = None


def lib():
    """Load liblle_cooptrails.so (after liblle_hip.so and liblle_coop.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    cooperation.lib()
    L = _binding.load(LIB_PATH, "the temporal cooperation tracker")
    vp = C.c_void_p
    _binding.tracker_signatures(L, "lle_cooptrails", [vp, vp, vp], [vp, C.c_int, vp])
    _lib = L
    return L


def launched_kernels():
    """Names of the kernels of liblle_cooptrails.so this process has launched (lle_cooptrails_debug_launched)."""
    return _binding.names(lib().lle_cooptrails_debug_launched)


def compiled_kernels():
    """Every instantiation the library holds (lle_cooptrails_debug_compiled)."""
    return _binding.names(lib().lle_cooptrails_debug_compiled)


class TemporalCooperationTracker(CooperationTracker):
    """A CooperationTracker with one lle_cooptrails behind it: every update / mark / reset issues the coop launch and then the trails
    launch with the same arguments.  Further attributes (torch tensors, VIEWS of the handle's device memory, valid until free()):
      episode_trails, last_trails       int64 [n]: 4 bits per agent, agent a in bits 4 a .. 4 a + 3 = the longest trail of help edges that
                                        ends at a (saturating at 15) -- of the running episode, of the last finished one
      episode_tprofile, last_tprofile   uint8 [n, 4]: longest trail, states whose edges entered the walk (saturating), dense, valid"""

    def __init__(self, batched_world):
        super().__init__(batched_world)
        L = lib()
        self.th = L.lle_cooptrails_create(self.world.h, self.h, self.world._stream())
        if not self.th:
            raise RuntimeError(f"lle_cooptrails_create failed: {L.lle_cooptrails_last_error().decode()}")
        self._trails_update = L.lle_cooptrails_update
        n = self.n_envs
        self.episode_trails = self._trails_view(LLE_COOPTRAILS_EPISODE_TRAILS, (n,), "<i8")
        self.last_trails = self._trails_view(LLE_COOPTRAILS_LAST_TRAILS, (n,), "<i8")
        self.episode_tprofile = self._trails_view(LLE_COOPTRAILS_EPISODE_TPROFILE, (n, 4), "|u1")
        self.last_tprofile = self._trails_view(LLE_COOPTRAILS_LAST_TPROFILE, (n, 4), "|u1")

    def _trails_view(self, which, shape, typestr):
        return _binding.tracker_view(lib(), "lle_cooptrails", self.th, which, shape, typestr, self.world.device)

    def _trails_check(self, rc):
        _binding.tracker_check(lib(), "lle_cooptrails", rc)

    # ------------------------------------------------------------------ updates
    def make_trails_args(self, ops, honour_auto_reset=False, env_mask=None, skip_refused=False):
        """An lle_cooptrails_update_args; the caller keeps `env_mask` (a uint8 device tensor) alive."""
        flags = (LLE_COOPTRAILS_HONOUR_AUTO_RESET if honour_auto_reset else 0) | (LLE_COOPTRAILS_SKIP_REFUSED if skip_refused else 0)
        return UpdateArgs(C.sizeof(UpdateArgs), int(ops), flags, 0, None if env_mask is None else env_mask.data_ptr())

    def launch_trails(self, args, stream=None):
        """The trails launch ALONE: it reads LLE_COOP_STEP_EDGES as the last coop launch left it."""
        rc = self._trails_update(self.th, C.byref(args), self.world._stream() if stream is None else stream)
        if rc != 0:
            self._trails_check(rc)

    def update(self, ops=cooperation.LLE_COOP_MARK_POS, honour_auto_reset=False, env_mask=None, env_sources=None, skip_refused=False):
        """One lle_coop_update and, behind it on the same stream, one lle_cooptrails_update with the same operations, flag and mask.
        skip_refused: LLE_COOPTRAILS_SKIP_REFUSED (after a step: an environment whose step was refused has no new state)."""
        import torch
        if env_mask is not None:
            env_mask = env_mask.to(self.world.device, torch.uint8).contiguous()
        super().update(ops, honour_auto_reset=honour_auto_reset, env_mask=env_mask, env_sources=env_sources)
        self.launch_trails(self.make_trails_args(ops, honour_auto_reset, self._mask, skip_refused))

    def update_map(self, map_index=0):
        super().update_map(map_index)
        self._trails_check(lib().lle_cooptrails_update_map(self.th, int(map_index), self.world._stream()))

    # ------------------------------------------------------------------ the temporal queries (profile.py), per environment
    def trail_lengths(self, last=False):
        """uint8 [n, A]: the longest trail of help edges that ends at each agent, saturating at 15."""
        import torch
        value = self.last_trails if last else self.episode_trails
        shifts = 4 * torch.arange(self.n_agents, device=value.device, dtype=torch.int64)
        return ((value.unsqueeze(1) >> shifts) & 15).to(torch.uint8)

    def _tprofile(self, last):
        return self.last_tprofile if last else self.episode_tprofile

    def longest_trail(self, last=False):
        """uint8 [n]: TemporalCooperationGraph.longest_trail_length of the episode, saturating at 15."""
        return self._tprofile(last)[:, T_LONGEST]

    def trails_exact(self, last=False):
        """bool [n]: no walk of the episode ran out of its budget -- the lengths are exact (up to the saturation), not lower bounds."""
        return self._tprofile(last)[:, T_DENSE] == 0

    def is_sequential(self, length=2, last=False):
        """bool [n]: a trail of at least `length` help edges exists (PlanProfile.is_sequential); False where the row is not valid."""
        if length < 2:
            raise ValueError("A sequence must have at least 2 edges")
        if length > LLE_COOPTRAILS_SATURATED:
            raise ValueError(f"trail lengths saturate at {LLE_COOPTRAILS_SATURATED}: is_sequential({length}) cannot be told from is_sequential({LLE_COOPTRAILS_SATURATED})")
        p = self._tprofile(last)
        return (p[:, T_VALID] != 0) & (p[:, T_LONGEST] >= int(length))

    def is_interdependent(self, n_agents=2, last=False):
        """bool [n]: some closed trail visits exactly n_agents distinct agents (PlanProfile.is_interdependent).  For 2 that is a pair
        of agents with both directions among the flattened edges: whichever of a -> b and b -> a comes first, its helper anchors a closed
        trail through exactly the two.  n_agents >= 3 needs a visited set per (anchor, agent): not built."""
        import torch
        if n_agents >= 3:
            raise NotImplementedError("is_interdependent(n_agents >= 3) is not built for batches: it needs a visited set per (anchor, current agent)")
        rows = self.last_edges if last else self.episode_edges
        if n_agents < 2:
            return torch.zeros(self.n_envs, dtype=torch.bool, device=rows.device)
        agents = torch.arange(self.n_agents, device=rows.device, dtype=torch.int32)
        forth = ((rows.unsqueeze(2) >> agents) & 1).bool()  # [n, h, b]: h helps b
        return (forth & forth.transpose(1, 2)).flatten(1).any(dim=1)

    def is_mutual(self, last=False):
        """bool [n]: PlanProfile.is_mutual = is_interdependent(2)."""
        return self.is_interdependent(2, last)

    def free(self):
        if getattr(self, "th", None):
            try:
                lib().lle_cooptrails_free(self.th)  # (before the coop handle: it reads that handle's arrays)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.th = None
        super().free()
