"""The temporal cooperation tracker of include/lle_cooptrails.h restated for ONE environment, in plain Python -- TEST INFRASTRUCTURE for
tests/test_cooptrails_cpu.py, tests/test_gpu_cooptrails.py and tests/test_gpu_cooptrails_states.py.

It keeps the episode as the list of its temporal edges (helper, beneficiary, t) and answers from the DEFINITION of a trail (chained
edges, times non-decreasing, no temporal edge twice): the longest trail that ENDS at an agent is searched backwards from that agent,
memoised over (agent, time, edges of that time already used, edges still allowed).  No trail value, no per-state update, no walk
from a starting agent: it shares no code and no method with either layer_update of the product.

A length is asked for up to a cap (15, the saturation of the tracker): a trail of more edges that ends at an agent has a suffix of
exactly `cap` edges, which is a trail that ends there too, so min(longest, cap) is the longest among the trails of at most cap edges.
"""
import sys

FINISH, CLEAR, MARK_STARTS, MARK_POS = 1, 2, 4, 8
SATURATED = 15


class Episode:
    """Temporal edges with time stamps 0, 1, 2, ... in the order the states are added; a memo that stays valid as states are added (a
    backward search from time t never sees a later edge)."""

    def __init__(self):
        self.into = {}   # (beneficiary, t) -> helpers
        self.n_states = 0
        self._memo = {}

    def add_state(self, edges):
        t = self.n_states
        for h, b in edges:
            if h != b:
                self.into.setdefault((b, t), []).append(h)
        self.n_states += 1

    def temporal_edges(self):
        return [(h, b, t) for (b, t), hs in sorted(self.into.items()) for h in hs]

    def _back(self, agent, t, used, k):
        """The longest trail of at most k edges that ends at `agent` no later than time t, none of its edges in `used` (edges of time t)."""
        if k == 0 or t < 0:
            return 0
        key = (agent, t, used, k)
        got = self._memo.get(key)
        if got is None:
            got = self._back(agent, t - 1, frozenset(), k)  # every edge of the rest is earlier
            for h in self.into.get((agent, t), ()):
                if (h, agent) not in used:
                    got = max(got, 1 + self._back(h, t, used | {(h, agent)}, k - 1))
            self._memo[key] = got
        return got

    def longest_ending_at(self, agent, cap=SATURATED):
        limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(limit, 4 * self.n_states + 1000))  # (one frame per state on the first question of a long episode)
        try:
            return self._back(agent, self.n_states - 1, frozenset(), cap)
        finally:
            sys.setrecursionlimit(limit)


def trail_lengths(temporal_edges, n_agents, cap=SATURATED):
    """[min(longest trail that ends at a, cap)] of a list of (helper, beneficiary, t) with any integer times."""
    times = sorted({t for _h, _b, t in temporal_edges})
    ep = Episode()
    for t in times:
        ep.add_state([(h, b) for h, b, tt in temporal_edges if tt == t])
    return [ep.longest_ending_at(a, cap) for a in range(n_agents)]


def is_mutual(flattened_edges):
    """Some pair of agents has both directions among the (helper, beneficiary) pairs."""
    flat = {(h, b) for h, b in flattened_edges if h != b}
    return any((b, h) in flat for h, b in flat)


def pack(lengths):
    """The u64 of include/lle_cooptrails.h as the int64 a torch view shows."""
    value = sum(min(int(v), SATURATED) << (4 * a) for a, v in enumerate(lengths))
    return value - (1 << 64) if value >= 1 << 63 else value


class EnvRef:
    """The temporal tracker's state of ONE environment and lle_cooptrails_update on it."""

    def __init__(self, n_agents):
        self.A = n_agents
        self.episode = Episode()
        self.count = self.dense = 0
        self.episode_valid = self.last_valid = False
        self.last_lengths, self.last_count, self.last_dense = [0] * n_agents, 0, 0
        self.touched = self.finished = False

    def lengths(self):
        return [self.episode.longest_ending_at(a) for a in range(self.A)]

    def _layer(self, edges):
        edges = {(h, b) for h, b in edges if h != b and h < self.A and b < self.A}
        if edges:
            self.episode.add_state(edges)
            self.count = min(255, self.count + 1)

    def update(self, ops, state_edges=(), start_edges=(), was_reset=False, refused=False):
        """`ops` on this environment.  was_reset: LLE_COOPTRAILS_HONOUR_AUTO_RESET found bit 7 of its event count; refused:
        LLE_COOPTRAILS_SKIP_REFUSED found its error byte set.  state_edges: the (helper, beneficiary) pairs of LLE_COOP_STEP_EDGES;
        start_edges: those of the map's freshly reset world."""
        phases = ([FINISH | CLEAR | MARK_STARTS] if was_reset else []) + [ops & ~MARK_POS if refused else ops]
        self.touched = bool(ops) or was_reset
        self.finished = self.touched and any(o & FINISH for o in phases)
        if not self.touched:
            return
        for o in phases:
            if o & FINISH:
                self.last_lengths, self.last_count, self.last_dense, self.last_valid = self.lengths(), self.count, self.dense, True
            if o & CLEAR:
                self.episode, self.count, self.dense = Episode(), 0, 0
            if o & MARK_STARTS:
                self._layer(start_edges)
            if o & MARK_POS:
                self._layer(state_edges)
        self.episode_valid = True

    def arrays(self):
        """(episode trails, last trails, episode profile, last profile): two integers (as int64) and two lists of four bytes."""
        now = self.lengths()
        return (pack(now) if self.episode_valid else 0, pack(self.last_lengths) if self.last_valid else 0,
                [max(now, default=0), self.count, self.dense, 1] if self.episode_valid else [0] * 4,
                [max(self.last_lengths, default=0), self.last_count, self.last_dense, 1] if self.last_valid else [0] * 4)
