"""ctypes binding of liblle_coop.so (lle_amd/coop/coop.hip, C ABI include/lle_coop.h) and
`CooperationTracker`: who helps whom in every environment of a batch, one launch per step.

The reference's cooperation analysis (python/lle/characterization/plan/: detect_dependencies, analyser.py:31-60, and the flattened
degree queries of TemporalCooperationGraph, graph.py:92-151) replays one world on the host.  The per-state rule -- an agent standing
on an enabled beam of its own colour helps every other agent standing on a tile of the same source -- is a pure function of the
positions, occupant bits, source colours and enable flags a batch already holds on the device, so the tracker computes it there.

    env = BatchedLLE(Map(level=6), 65536, cooperation=True)
    env.reset(); env.step(actions, auto_reset=True)
    env.cooperation.is_cooperative()          # bool [n]: the running episode has seen a help edge
    env.cooperation.last_profile              # uint8 [n, 8]: the profile of each environment's last finished episode

The module is loaded only when a tracker is asked for.  No fallback: a missing library raises.
"""
import ctypes as C
import os
import weakref

from . import _binding, _capi
from ._binding import UpdateArgs  # lle_coop_update_args

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblle_coop.so")

# enums of include/lle_coop.h
LLE_COOP_FINISH, LLE_COOP_CLEAR, LLE_COOP_MARK_STARTS, LLE_COOP_MARK_POS = 1, 2, 4, 8
LLE_COOP_HONOUR_AUTO_RESET, LLE_COOP_ENV_SOURCES = 1, 2
LLE_COOP_STEP_EDGES, LLE_COOP_EPISODE_EDGES, LLE_COOP_LAST_EDGES, LLE_COOP_EPISODE_PROFILE, LLE_COOP_LAST_PROFILE = range(5)
# bytes of a profile row
P_EDGES, P_VERTICES, P_MAX_HELPERS, P_MAX_BENEFICIARIES, P_ASYMMETRIC, P_STATES, P_ZERO, P_VALID = range(8)

EXPORTS = ["lle_coop_cell_masks", "lle_coop_create", "lle_coop_update_map", "lle_coop_free", "lle_coop_update", "lle_coop_buffer",
           "lle_coop_start_edges", "lle_coop_last_error", "lle_coop_debug_launched", "lle_coop_debug_compiled"]


_lib = None


def lib():
    """Load liblle_coop.so (after liblle_hip.so, which it links against)."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()
    L = _binding.load(LIB_PATH, "the cooperation tracker")
    vp, i32 = C.c_void_p, C.c_int
    _binding.tracker_signatures(L, "lle_coop", [vp, C.POINTER(vp), i32, vp], [vp, i32, vp, vp])
    L.lle_coop_cell_masks.restype = i32
    L.lle_coop_cell_masks.argtypes = [vp, C.POINTER(C.c_uint32), i32]
    L.lle_coop_start_edges.restype = i32
    L.lle_coop_start_edges.argtypes = [vp, i32, C.POINTER(C.c_uint32), i32]
    _lib = L
    return L


_names = _binding.names  # (other modules and tests take it from here)


def launched_kernels():
    """Names of the kernels of liblle_coop.so this process has launched (lle_coop_debug_launched)."""
    return _names(lib().lle_coop_debug_launched)


def compiled_kernels():
    """Every instantiation the library holds (lle_coop_debug_compiled)."""
    return _names(lib().lle_coop_debug_compiled)


def cell_masks(map_):
    """The cell table of a Map (lle_coop_cell_masks; host only): a list of height * width integers, bit l of entry i * width + j
    set when source laser_id l owns a laser tile on (i, j) in the sense of World.lasers (the outer two layers of a cell)."""
    L = lib()
    n = L.lle_coop_cell_masks(map_.h, None, 0)
    if n < 0:
        raise RuntimeError(f"lle_coop_cell_masks failed: {L.lle_coop_last_error().decode()}")
    buf = (C.c_uint32 * max(n, 1))()
    L.lle_coop_cell_masks(map_.h, buf, n)
    return [int(buf[k]) for k in range(n)]


def edges_of_rows(rows):
    """[(helper, beneficiary)] of one environment's rows (row h = bit mask of the beneficiaries of helper h), sorted."""
    return [(h, b) for h, row in enumerate(rows) for b in range(16) if (int(row) >> b) & 1]


class CooperationTracker:
    """One lle_coop over a BatchedWorld.  Attributes (torch tensors, VIEWS of the handle's device memory, valid until free()):
      step_edges, episode_edges, last_edges   int32 [n, A]: row h = bit mask of the beneficiaries of helper h -- of the state last
                                              marked, of the running episode (flattened_edges), of the last finished episode
      episode_profile, last_profile           uint8 [n, 8]: edges, vertices, max_distinct_helpers, max_distinct_beneficiaries,
                                              asymmetric edges, marked states with an edge (saturating), 0, valid
    The tracker is created CLEARED; `mark()` enters the state the batch is in (BatchedLLE does so at construction)."""

    def __init__(self, batched_world):
        L = lib()
        w = self.world = batched_world
        handles = (C.c_void_p * len(w.maps))(*[m.h for m in w.maps])
        self.h = L.lle_coop_create(w.h, handles, len(w.maps), w._stream())
        if not self.h:
            raise RuntimeError(f"lle_coop_create failed: {L.lle_coop_last_error().decode()}")
        self._update = L.lle_coop_update
        self.n_envs, self.n_agents = int(w.n_envs), int(w.map.n_agents)
        n, A = self.n_envs, self.n_agents
        self.step_edges = self._view(LLE_COOP_STEP_EDGES, (n, A), "<i4")
        self.episode_edges = self._view(LLE_COOP_EPISODE_EDGES, (n, A), "<i4")
        self.last_edges = self._view(LLE_COOP_LAST_EDGES, (n, A), "<i4")
        self.episode_profile = self._view(LLE_COOP_EPISODE_PROFILE, (n, 8), "|u1")
        self.last_profile = self._view(LLE_COOP_LAST_PROFILE, (n, 8), "|u1")
        if not hasattr(w, "_coop_trackers"):
            w._coop_trackers = weakref.WeakSet()
        w._coop_trackers.add(self)  # update_map / update_sources of the world refresh the tracker's tables

    def _view(self, which, shape, typestr):
        return _binding.tracker_view(lib(), "lle_coop", self.h, which, shape, typestr, self.world.device)

    def _check(self, rc):
        _binding.tracker_check(lib(), "lle_coop", rc)

    # ------------------------------------------------------------------ updates
    def make_args(self, ops, honour_auto_reset=False, env_mask=None, env_sources=None):
        """An lle_coop_update_args; the caller keeps `env_mask` (a uint8 device tensor) alive.  env_sources None: whether the world
        keeps per-environment sources now (BatchedWorld.set_sources has run)."""
        if env_sources is None:
            env_sources = bool(getattr(self.world, "_env_sources", False))
        flags = (LLE_COOP_HONOUR_AUTO_RESET if honour_auto_reset else 0) | (LLE_COOP_ENV_SOURCES if env_sources else 0)
        return UpdateArgs(C.sizeof(UpdateArgs), int(ops), flags, 0, None if env_mask is None else env_mask.data_ptr())

    def launch(self, args, stream=None):
        rc = self._update(self.h, C.byref(args), self.world._stream() if stream is None else stream)
        if rc != 0:
            self._check(rc)

    def update(self, ops=LLE_COOP_MARK_POS, honour_auto_reset=False, env_mask=None, env_sources=None):
        """One lle_coop_update on the world's current stream: FINISH, CLEAR, MARK_STARTS, MARK_POS in this order on the environments
        with env_mask != 0 (None: all); honour_auto_reset: LLE_COOP_HONOUR_AUTO_RESET (only right after a whole-batch step)."""
        import torch
        if env_mask is not None:
            env_mask = env_mask.to(self.world.device, torch.uint8).contiguous()
        self._mask = env_mask  # (kept alive until the launch has read it)
        self.launch(self.make_args(ops, honour_auto_reset, env_mask, env_sources))

    def mark(self, env_mask=None):
        """The episode continues: the state the batch is in now is one more state of it."""
        self.update(LLE_COOP_MARK_POS, env_mask=env_mask)

    def reset(self, env_mask=None):
        """The selected environments have just been reset: their episode is finished (`last_*`), cleared, and the reset state
        marked.  Call it BEHIND the world's reset."""
        self.update(LLE_COOP_FINISH | LLE_COOP_CLEAR | LLE_COOP_MARK_POS, env_mask=env_mask)

    def update_map(self, map_index=0):
        """After Map.set_source / set_exits pushed to the batch: colour masks, enabled mask and start edges follow."""
        self._check(lib().lle_coop_update_map(self.h, int(map_index), self.world.maps[map_index].h, self.world._stream()))

    def start_edges(self, map_index=0):
        """[(helper, beneficiary)] of the state right after a reset of map `map_index`, as the handle holds them."""
        buf = (C.c_uint32 * 16)()
        n = lib().lle_coop_start_edges(self.h, int(map_index), buf, 16)
        if n < 0:
            self._check(n)
        return edges_of_rows([buf[a] for a in range(n)])

    # ------------------------------------------------------------------ the profile's queries (profile.py:8-77), per environment
    def _profile(self, last):
        return self.last_profile if last else self.episode_profile

    def is_cooperative(self, last=False):
        """bool [n]: the episode has a help edge (PlanProfile.is_cooperative)."""
        return self._profile(last)[:, P_EDGES] > 0

    def is_independent(self, last=False):
        return self._profile(last)[:, P_EDGES] == 0

    def is_asymmetric(self, last=False):
        """bool [n]: some helper is never helped (PlanProfile.is_asymmetric)."""
        return self._profile(last)[:, P_ASYMMETRIC] > 0

    def is_convergent(self, k=2, last=False):
        """bool [n]: one beneficiary is helped by at least k distinct agents; False where k >= n_vertices (profile.py:56-66)."""
        if k < 2:
            raise ValueError(f"Convergence requires at least 2 distinct helpers, got {k}.")
        p = self._profile(last)
        return (p[:, P_VERTICES] > k) & (p[:, P_MAX_HELPERS] >= k)

    def is_divergent(self, k=2, last=False):
        """bool [n]: one helper helps at least k distinct agents; False where k >= n_vertices (profile.py:68-77)."""
        if k < 2:
            raise ValueError(f"Divergence requires at least 2 distinct beneficiaries, got {k}.")
        p = self._profile(last)
        return (p[:, P_VERTICES] > k) & (p[:, P_MAX_BENEFICIARIES] >= k)

    def edges(self, env, which="episode"):
        """Host list of (helper, beneficiary) of environment `env`: which = "step", "episode" or "last" (synchronises)."""
        t = {"step": self.step_edges, "episode": self.episode_edges, "last": self.last_edges}[which]
        return edges_of_rows(t[int(env)].cpu().tolist())

    def free(self):
        if getattr(self, "h", None):
            try:
                lib().lle_coop_free(self.h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass
            self.h = None

    def __del__(self):
        self.free()
