"""The closed-trail cooperation tracker of include/lle_coopcycles.h restated for ONE environment, in plain Python -- TEST INFRASTRUCTURE
for tests/test_coopcycles_cpu.py, tests/test_gpu_coopcycles.py and tests/test_gpu_coopcycles_states.py.

It keeps the episode's value as a frozenset R of triples (anchor, current, frozenset of agents) and extends it per layer with
`tests/cycles_ref.layer_update(R, arcs)` WITHOUT an order: that function enumerates the trails inside a state from the definition and
knows no words, masks or budgets.  The operations and their order are those of tests/cooptrails_ref.EnvRef.

`encode` packs R into the words of the header comment of lle_amd/cycles/cycles_logic.hpp (THE BITS), written from that comment.
The decode direction is the package's own (`lle_amd.cycles.triples`).

The dense mark (a layer dropped for running out of its budget) is NOT restated: the tests keep ordinary states at 5 arcs or fewer,
which stay far inside the budget, and check the dense case by its properties.
"""
from tests import cycles_ref

FINISH, CLEAR, MARK_STARTS, MARK_POS = 1, 2, 4, 8
MAX_AGENTS = 6


def words_of(n_agents):
    return 3 if n_agents <= 4 else 21


def _without_bit(mask, k):
    """`mask` with bit k taken out: the bits above it move down by one."""
    return (mask & ((1 << k) - 1)) | ((mask >> (k + 1)) << k)


def encode(R, n_agents, words=None):
    """The W words (unsigned) of R (W = `words`, or that of the map's agents): a pair (a, c) owns one field, a bitset over the subsets
    of the REMAINING agents of the class (AC = 4 for 3 words, 6 for 21)
      closed field a             2^(AC - 1) bits at bit a * 2^(AC - 1)
      open field (a, c), a != c  2^(AC - 2) bits at bit AC * 2^(AC - 1) + (a * (AC - 1) + c - (c > a)) * 2^(AC - 2)
    bit p of a field = the support whose agent mask is p with a one inserted at bit min(a, c) and then at bit max(a, c)."""
    words = words or words_of(n_agents)
    ac = 4 if words == 3 else 6
    assert n_agents <= ac
    closed_bits, open_bits = 1 << (ac - 1), 1 << (ac - 2)
    value = 0
    for a, c, support in R:
        mask = sum(1 << k for k in support)
        assert (mask >> a) & 1 and (mask >> c) & 1 and mask < 1 << ac
        if a == c:
            value |= 1 << (a * closed_bits + _without_bit(mask, a))
        else:
            p = _without_bit(_without_bit(mask, max(a, c)), min(a, c))
            value |= 1 << (ac * closed_bits + (a * (ac - 1) + c - (c > a)) * open_bits + p)
    return [(value >> (32 * i)) & 0xFFFFFFFF for i in range(words)]


def as_int32(word):
    """An unsigned word as the int32 a torch view shows."""
    return word - (1 << 32) if word >= 1 << 31 else word


def closed_orders(R):
    """The sizes of the supports of the closed triples, sorted."""
    return sorted({len(s) for a, c, s in R if a == c})


def orders_byte(R):
    return sum(1 << k for k in closed_orders(R))


def graph_triples(temporal_edges):
    """R of a whole graph given as (helper, beneficiary, t) with any integer times: one layer per time, in order."""
    R = frozenset()
    for t in sorted({t for _h, _b, t in temporal_edges}):
        R = cycles_ref.layer_update(R, {(h, b) for h, b, tt in temporal_edges if tt == t and h != b})
    return R


_LAYERS = {}


def layer(R, arcs):
    """cycles_ref.layer_update(R, arcs), remembered: the environments of a batch share most (R, arcs) pairs."""
    key = (R, arcs)
    if key not in _LAYERS:
        if len(_LAYERS) > 200000:
            _LAYERS.clear()
        _LAYERS[key] = cycles_ref.layer_update(R, arcs)
    return _LAYERS[key]


class EnvRef:
    """The closed-trail tracker's state of ONE environment and lle_coopcycles_update on it."""

    def __init__(self, n_agents):
        assert 1 <= n_agents <= MAX_AGENTS
        self.A = n_agents
        self.R = frozenset()
        self.flat = frozenset()  # the arcs of the running episode without their times: the flattened edges
        self.count = 0
        self.episode_valid = self.last_valid = False
        self.last_R, self.last_count = frozenset(), 0
        self.touched = self.finished = False
        self.layers = 0  # layers with an arc entered by the most recent update

    def _layer(self, edges):
        arcs = frozenset((h, b) for h, b in edges if h != b and h < self.A and b < self.A)
        if arcs:
            self.flat |= arcs
            self.R = layer(self.R, arcs)
            self.count = min(255, self.count + 1)
            self.layers += 1

    def update(self, ops, state_edges=(), start_edges=(), was_reset=False, refused=False):
        """`ops` on this environment.  was_reset: LLE_COOPCYCLES_HONOUR_AUTO_RESET found bit 7 of its event count; refused:
        LLE_COOPCYCLES_SKIP_REFUSED found its error byte set.  state_edges: the (helper, beneficiary) pairs of LLE_COOP_STEP_EDGES;
        start_edges: those of the map's freshly reset world."""
        phases = ([FINISH | CLEAR | MARK_STARTS] if was_reset else []) + [ops & ~MARK_POS if refused else ops]
        self.touched = bool(ops) or was_reset
        self.finished = self.touched and any(o & FINISH for o in phases)
        self.layers = 0
        if not self.touched:
            return
        for o in phases:
            if o & FINISH:
                self.last_R, self.last_count, self.last_valid = self.R, self.count, True
            if o & CLEAR:
                self.R, self.count, self.flat = frozenset(), 0, frozenset()
            if o & MARK_STARTS:
                self._layer(start_edges)
            if o & MARK_POS:
                self._layer(state_edges)
        self.episode_valid = True

    def orders(self, last=False):
        return closed_orders(self.last_R if last else self.R)

    def arrays(self):
        """(episode words, last words, episode profile, last profile): two lists of W words (as int32) and two lists of four bytes."""
        return ([as_int32(w) for w in encode(self.R, self.A)], [as_int32(w) for w in encode(self.last_R, self.A)],
                [orders_byte(self.R), self.count, 0, 1] if self.episode_valid else [0] * 4,
                [orders_byte(self.last_R), self.last_count, 0, 1] if self.last_valid else [0] * 4)
