"""Chosen start states for the step kernel: `World.set_state` anywhere on the map, then ONE step under every joint action.

The other step suites start every walk at the start cells, so the states a step begins from are whatever a uniform random walk
reaches in a few dozen moves.  This module builds the states on purpose (pure numpy + the oracle, no GPU) and says, from the ORACLE's
outcomes, which classes of steps a batch holds; tests/test_step_states_cpu.py runs it on the host builds of the state machines and
asserts the coverage, tests/test_gpu_step_states.py runs the same batches through the kernels.

One environment per (state, joint action):

* states      seeded draws per map -- distinct walkable cells (never a wall, never a source), every gem collected with p = 0.4, every
              agent alive with p = 0.8 -- kept only when the oracle's world accepts the request (`set_state` on a freshly reset world;
              a placement that kills an agent requested alive is InvalidWorldState: resampled, the tries are bounded), in front of them
              the PLANTED states below;
* actions     A <= 3: the whole product of the agents' available sets (the oracle's masks after its own set_state); A >= 7: 64 seeded
              draws from that product; plus, for every state and every agent a, one joint action in which a is the lowest offender
              (the agents below a act legally, a takes an unavailable direction or a value in 5..7, alternating, the agents above a
              anything in 0..7): the step must be refused with err = 1 + a and leave the environment untouched;
* planted     scenarios built from the map's geometry (sources, beam cells, gems, exits) for the classes random placement misses,
              each validated by the oracle before it is kept -- the class flags of `classify` are computed from the oracle's events and
              dumps, never from an engine:
                cascade      X of beam B1's colour steps onto a cell that B1 shares with a lit beam of another colour (it cuts B1 and dies
                             in the same pass) while Y enters B1 further down: a SECOND move_agents pass in which Y re-lights B1 and dies
                             -- events ordered by pass first (Died X, Died Y with Y < X: not ascending in agent id), a cut and a re-light
                             of the same beam word in one step (X coming from down the beam), chain carries on beams longer than 32 cells;
                             with a third agent behind Y's own beam a THIRD pass;
                q1           the reference's Q1 script on its own start state ([East, North, Stay]), and its two-agent / long-beam analogues;
                arrival      all agents but one on exits, the last one beside its exit: `arrived.all()` turns true in the step;
                targets      two / three agents around one cell, all moving onto it (solve_vertex_conflicts sends them back).  A SECOND round
                             of that loop needs an agent moving onto the cell another one is sent back to, i.e. onto an occupied cell: never
                             available from a state the reference accepts -- only through the stale availability lists a REFUSED set_state
                             leaves behind (world.rs:588-594), which tests/test_step_states_cpu.py and the GPU suite reach on STALE_MAP;
                corpse       an agent requested dead on a lit beam of another colour (it dies on entering: a corpse that is NOT an occupant),
                             a living neighbour walking onto that cell;
                pickups      a gem / an exit taken in the step in which somebody else dies, two deaths, three events;
                last-alive   everybody dead but one, who walks into a beam: a step that leaves nobody alive;
                four layers  an agent on the four-layer cell of `four_layers` -- every neighbour of that cell lies under an always-lit beam of a
                             colour no agent has, so no agent can WALK onto it: the reachable case is a corpse placed there by set_state;
                gem 31       the 32nd gem of `gems32` walked onto while uncollected and while collected.

Maps by lanes per environment (step_kernel's G): registers and single layers, crossings up to four layers, more than 8 sources (the
LDS form of the beams), chained beam words.  `q1_pair`, `gems32` and `solo_beams` are this module's own: the two-agent maps of the other
suites can hold neither a second-pass death out of agent order nor a 32nd gem, and the one-agent map has no beam of its agent's colour."""
import functools
import itertools

import numpy as np

from tests import instantiation_maps as im
from tests.parity_util import EXTRA_MAPS, LONG_MAPS

ACTION_DELTA = np.array([(-1, 0), (1, 0), (0, 1), (0, -1), (0, 0)], np.int64)  # N S E W STAY (src/action.rs:18-26)
DIR_DELTA = [(-1, 0), (0, 1), (1, 0), (0, -1)]                                  # N E S W (direction.rs:20-27)
EV_EXIT, EV_GEM, EV_DIED = 0, 1, 2
STAY = 4

OWN_MAPS = {
    # Q1 without its third agent: colour 2 has no agent (legal, quirk Q5), [East, North] is Died(1) in pass 1 and Died(0) in pass 2
    "q1_pair": "S0 . G X\n. . L2W X\n. S1 . .\n. L1N . .",
    # 32 gems: bit 31 of the gem word
    "gems32": "S0 . . . . . . S1\n" + "G G G G G G G G\n" * 4 + "X X . . . . . .",
    # one agent WITH a beam of its own colour (colour_alias has none: nothing its agent does changes a beam bit there), a foreign beam
    # to die on, a gem under the own beam and one beside it, an exit under the foreign beam and a plain one
    "solo_beams": "S0 . . G X\n. . . . .\nL0E . G . .\n. . . . .\nL1E . . V X",
}
GENERATED = {"im_3_20": (3, 20, False, 320), "im_7_7x": (7, 7, True, 707), "im_13_12x": (13, 12, True, 1312)}

# lanes per environment -> maps
GROUPS = {
    1: ["colour_alias", "solo_beams"],
    2: ["four_layers", "exit_under_beam", "voids_gems", "long_q1", "q1_pair", "gems32"],
    4: ["q1", "nested", "three_beams", "long_crossing", "long_three_words", "im_3_20"],
    8: ["im_7_7x"],
    16: ["im_13_12x", "many_agents"],
}
MAP_NAMES = [name for g in sorted(GROUPS) for name in GROUPS[g]]
GROUP_OF = {name: g for g, names in GROUPS.items() for name in names}
CHAINED = ["long_q1", "long_crossing", "long_three_words"]

N_RANDOM_STATES = {1: 300, 2: 150, 3: 40, 7: 40, 13: 36, 14: 36}
N_DRAWS = 64          # joint actions per state where the product is not enumerated (A >= 7)
MAX_PLANTED = 40      # planted states per map
MAX_TRIES = 400       # draws per accepted random state
MAX_ENVS = 8192


def text_of(name, variant=0):
    if name in GENERATED:
        A, L, cross, seed = GENERATED[name]
        return im.build(A, L, cross, seed=seed, variant=variant)
    for maps in (OWN_MAPS, EXTRA_MAPS, LONG_MAPS):
        if name in maps:
            return maps[name]
    raise KeyError(name)


def has_twin(name):
    """Whether instantiation_maps can build a second placement over the same walls and sources (a two-map batch of distinct maps)."""
    return name in GENERATED


def group_size(n_agents):
    return 1 if n_agents == 1 else 2 if n_agents == 2 else 4 if n_agents <= 4 else 8 if n_agents <= 8 else 16


def ragged(n):
    """The largest 16 m + 5 that is <= n."""
    return (n - 5) // 16 * 16 + 5


def block_size(n):
    """The largest multiple of 16 that is no multiple of 64 and <= n (the blocks of a two-map batch: no workgroup straddles two maps)."""
    p = n // 16 * 16
    return p - 16 if p % 64 == 0 else p


class Geometry:
    """What the planters need to know about a map, all of it from the oracle's world."""

    def __init__(self, w):
        self.H, self.W, self.A, self.G = w.height, w.width, w.n_agents, w.n_gems
        walls = set(w.wall_pos)  # (source cells are wall_pos entries too)
        self.walkable = [(i, j) for i in range(self.H) for j in range(self.W) if (i, j) not in walls]
        self.walk_set = set(self.walkable)
        self.voids, self.gems, self.exits, self.starts = list(w.void_pos), list(w.gem_pos), list(w.exit_pos), list(w.start_pos)
        self.sources = w.sources()
        self.beam_cells = []   # per source: the cells of its beam, nearest first
        self.layers = {}       # cell -> [(source, offset, colour)]
        for s, (i, j, d, colour, _en, length) in enumerate(self.sources):
            di, dj = DIR_DELTA[d]
            cells = [(i + (k + 1) * di, j + (k + 1) * dj) for k in range(length)]
            self.beam_cells.append(cells)
            for k, c in enumerate(cells):
                self.layers.setdefault(c, []).append((s, k, colour))
        special = set(self.layers) | set(self.voids) | set(self.gems) | set(self.exits)
        self.floor = [c for c in self.walkable if c not in special]

    def neighbours(self, c, within=None):
        out = []
        for a in range(4):
            p = (c[0] + int(ACTION_DELTA[a][0]), c[1] + int(ACTION_DELTA[a][1]))
            if p in self.walk_set and (within is None or p in within):
                out.append(p)
        return out


def action_towards(p, c):
    d = (c[0] - p[0], c[1] - p[1])
    for a in range(5):
        if tuple(ACTION_DELTA[a]) == d:
            return a
    raise ValueError((p, c))


def _scenario(geo, rng, fixed, acts, dead=(), gems=None, others_dead=False):
    """A planted candidate: the agents of `fixed` on their cells, everybody else on plain floor away from them, staying.
    Returns (positions, gems, alive, joint action) or None when the map has no room."""
    used = set(fixed.values())
    keep_off = set(used)
    for c in used:
        keep_off.update(geo.neighbours(c))
        for p in geo.neighbours(c):
            keep_off.update(geo.neighbours(p))
    pool = [c for c in geo.floor if c not in keep_off]
    if len(pool) < geo.A - len(fixed):
        pool = [c for c in geo.floor if c not in used] + [c for c in geo.walkable if c not in used and c not in geo.floor]
    if len(pool) < geo.A - len(fixed):
        return None
    order = rng.permutation(len(pool))
    pos, k = [], 0
    for a in range(geo.A):
        if a in fixed:
            pos.append(fixed[a])
        else:
            pos.append(pool[int(order[k])])
            k += 1
    alive = [a not in dead and (a in fixed or not others_dead) for a in range(geo.A)]
    g = [False] * geo.G if gems is None else list(gems)
    return pos, g, alive, [int(acts.get(a, STAY)) for a in range(geo.A)]


def _plant_candidates(name, geo, rng):
    """Candidate scenarios, most specific first.  Nothing here is trusted: `build_case` keeps a candidate only when the oracle
    accepts its state AND its step shows a class that is still wanted."""
    A, out = geo.A, []

    def add(tag, sc):
        if sc is not None:
            out.append((tag,) + sc)

    # the reference's Q1 script and its analogues
    if name == "q1":
        add("q1", (list(geo.starts), [False] * geo.G, [True] * A, [2, 0, 4]))
    if name == "q1_pair":
        add("q1", (list(geo.starts), [False] * geo.G, [True] * A, [2, 0]))
    if name == "long_q1":  # agent 0 walks along its own 38-cell beam under the beam of colour 1 and dies; agent 1, entering further down, re-lights it in pass 2
        add("q1", ([(1, 11), (2, 20)], [False] * geo.G, [True, True], [2, 0]))
        add("q1", ([(1, 11), (0, 33)], [False] * geo.G, [True, True], [2, 1]))
    # cascades: X cuts its own beam B1 on a cell shared with a lit beam of another colour and dies; Y enters B1 further down
    crossings = [c for c, lay in geo.layers.items() if len(lay) >= 2 and c in geo.walk_set]
    n_cascade = 0
    for ci in rng.permutation(len(crossings)):
        c = crossings[int(ci)]
        for (s1, k1, x) in geo.layers[c]:
            if x >= A or all(col == x for (_s, _k, col) in geo.layers[c]) or n_cascade > 900:
                continue
            down = geo.beam_cells[s1][k1 + 1:k1 + 4]
            for p in geo.neighbours(c):
                for d in down:
                    if d not in geo.walk_set:
                        break
                    for q in [d] + geo.neighbours(d):
                        if q == p or q == c or (q == d and p == d):
                            continue
                        others = [y for y in range(A) if y != x]
                        for y in others[:2] + others[-1:]:
                            fixed, acts = {x: p, y: q}, {x: action_towards(p, c), y: action_towards(q, d)}
                            add("cascade", _scenario(geo, rng, fixed, acts))
                            n_cascade += 1
                            # a third pass: Y owns a second beam through d, Z enters that one further down
                            for (s2, k2, col2) in geo.layers.get(d, []):
                                if col2 != y or s2 == s1 or q == d:
                                    continue
                                for e in geo.beam_cells[s2][k2 + 1:k2 + 3]:
                                    for r in geo.neighbours(e):
                                        zs = [z for z in range(A) if z not in (x, y)]
                                        if zs and r not in (p, q, c, d) and e not in (p, q, c, d):
                                            f3 = dict(fixed)
                                            f3[zs[0]] = r
                                            a3 = dict(acts)
                                            a3[zs[0]] = action_towards(r, e)
                                            add("cascade3", _scenario(geo, rng, f3, a3))
    # a long beam cut in its first word by its owner walking in from the side: the change carries into the following words
    for s, cells in enumerate(geo.beam_cells):
        colour = geo.sources[s][3]
        if len(cells) > 32 and colour < A:
            for k in (3, 17, 30):
                side = [p for p in geo.neighbours(cells[k]) if p not in cells]
                if side:
                    add("chain", _scenario(geo, rng, {colour: side[0]}, {colour: action_towards(side[0], cells[k])}))
    tiles = [(c, lay[0][2]) for c, lay in geo.layers.items() if c in geo.walk_set]   # (cell, colour of one beam over it)
    floor = set(geo.floor)
    for trial in range(10):
        # the last agent arrives
        for _attempt in range(6 if len(geo.exits) >= A else 0):  # (an exit under a foreign beam kills: the oracle sorts the attempts)
            ex = [geo.exits[int(k)] for k in rng.permutation(len(geo.exits))[:A]]
            last = int(rng.integers(A))
            beside = [p for p in geo.neighbours(ex[last]) if p not in ex]
            if beside:
                p = beside[int(rng.integers(len(beside)))]
                fixed = {a: (p if a == last else ex[a]) for a in range(A)}
                add("arrival", _scenario(geo, rng, fixed, {last: action_towards(p, ex[last])}))
        # two / three agents onto one cell
        for k in (2, 3):
            if A >= k and geo.floor:
                t = geo.floor[int(rng.integers(len(geo.floor)))]
                nb = geo.neighbours(t, floor)
                if len(nb) >= k:
                    ids = [int(v) for v in rng.permutation(A)[:k]]
                    add("targets", _scenario(geo, rng, {a: nb[q] for q, a in enumerate(ids)}, {a: action_towards(nb[q], t) for q, a in enumerate(ids)}))
        if not tiles:
            continue
        pick = [tiles[int(k)] for k in rng.permutation(len(tiles))[:2]]
        (t1, c1), (t2, c2) = pick[0], pick[-1]
        hostile1 = [a for a in range(A) if a != c1]
        hostile2 = [a for a in range(A) if a != c2]
        if not hostile1:
            continue
        h1 = hostile1[int(rng.integers(len(hostile1)))]
        q1 = geo.neighbours(t1, floor) or geo.neighbours(t1)
        if not q1:
            continue
        q1 = q1[int(rng.integers(len(q1)))]
        death = ({h1: q1}, {h1: action_towards(q1, t1)})
        # everybody else dead: the step leaves nobody alive
        add("last-alive", _scenario(geo, rng, death[0], death[1], others_dead=True))
        if A < 2:
            continue
        # a corpse that is not an occupant, a living neighbour walking onto it
        walkers = [a for a in range(A) if a != h1]
        wk = walkers[int(rng.integers(len(walkers)))]
        add("corpse", _scenario(geo, rng, {h1: t1, wk: q1}, {wk: action_towards(q1, t1)}, dead=(h1,)))
        # a gem / an exit taken while somebody dies; two deaths; three events
        for kind, cells in (("gem", geo.gems), ("exit", geo.exits)):
            plain = [g for g in cells if g not in geo.layers] or list(cells)
            if not plain:
                continue
            g = plain[int(rng.integers(len(plain)))]
            pg = [p for p in geo.neighbours(g) if p not in (q1, t1)]
            if pg:
                pg = pg[int(rng.integers(len(pg)))]
                add("pickup", _scenario(geo, rng, {h1: q1, wk: pg}, {h1: death[1][h1], wk: action_towards(pg, g)}))
                if A >= 3 and kind == "gem" and geo.exits:
                    third = [a for a in range(A) if a not in (h1, wk)][0]
                    x = geo.exits[int(rng.integers(len(geo.exits)))]
                    px = [p for p in geo.neighbours(x) if p not in (q1, t1, pg, g)]
                    if px and x not in (q1, t1, pg, g):
                        add("pickup", _scenario(geo, rng, {h1: q1, wk: pg, third: px[0]},
                                                {h1: death[1][h1], wk: action_towards(pg, g), third: action_towards(px[0], x)}))
        h2s = [a for a in hostile2 if a != h1]
        q2 = [p for p in (geo.neighbours(t2, floor) or geo.neighbours(t2)) if p not in (q1, t1)]
        if h2s and q2 and t2 != t1 and t2 != q1:
            h2 = h2s[int(rng.integers(len(h2s)))]
            add("two-deaths", _scenario(geo, rng, {h1: q1, h2: q2[0]}, {h1: death[1][h1], h2: action_towards(q2[0], t2)}))
    if name == "four_layers":
        for a in range(A):
            add("four-layers", _scenario(geo, rng, {a: (2, 2)}, {}, dead=(a,)))
    if name == "gems32":
        g = geo.gems[31]
        p = geo.neighbours(g)[0]
        for collected in (False, True):
            gems = [False] * geo.G
            gems[31] = collected
            add("gem31", _scenario(geo, rng, {0: p}, {0: action_towards(p, g)}, gems=gems))
    return out


class Case:
    """The environments of one map: request arrays for set_state, the explicit joint action of the first step."""

    def __init__(self, name, text, A, G, pos, gems, alive, actions, state_of, n_planted):
        self.name, self.text, self.A, self.G = name, text, A, G
        self.pos, self.gems, self.alive, self.actions, self.state_of, self.n_planted = pos, gems, alive, actions, state_of, n_planted
        self.n = len(pos)

    def truncated(self, n):
        assert n <= self.n
        return Case(self.name, self.text, self.A, self.G, self.pos[:n].copy(), self.gems[:n].copy(), self.alive[:n].copy(),
                    self.actions[:n].copy(), self.state_of[:n].copy(), self.n_planted)


def _accept(oracle_mod, w, pos, gems, alive):
    """The oracle's availability masks after set_state on a freshly reset world, or None when it refuses the request."""
    w.reset()
    try:
        w.set_state([tuple(int(v) for v in p) for p in pos], [bool(v) for v in gems], [bool(v) for v in alive])
    except oracle_mod.OracleError:
        return None
    return w.available_mask()


def random_state(rng, walkable, A, G):
    idx = rng.permutation(len(walkable))[:A]
    return [walkable[int(k)] for k in idx], rng.random(G) < 0.4, rng.random(A) < 0.8


def joint_actions(rng, masks, parity):
    """The product of the available sets (A <= 3) or N_DRAWS draws from it, then one refusal per agent."""
    A = len(masks)
    sets = [[k for k in range(5) if (m >> k) & 1] for m in masks]
    if A <= 3:
        acts = [list(t) for t in itertools.product(*sets)]
    else:
        acts = [[s[int(rng.integers(len(s)))] for s in sets] for _ in range(N_DRAWS)]
    for a in range(A):
        row = [sets[b][int(rng.integers(len(sets[b])))] for b in range(a)]
        closed = [k for k in range(4) if not (masks[a] >> k) & 1]
        if (a + parity) % 2 == 0 and closed:
            row.append(closed[int(rng.integers(len(closed)))])
        else:
            row.append(5 + int(rng.integers(3)))
        row += [int(rng.integers(8)) for _ in range(a + 1, A)]
        acts.append(row)
    return acts


def apply_states(oracle_mod, ob, case, lo=0, rng=None, record=None):
    """set_state on every world of `ob` (the envs [lo, lo + ob.n) of `case`); `record`, a dict, receives the events the oracle
    returned (ev_count [n], events [n, 2 A, 2], rows beyond the count zero).  With `rng` (worlds that carry their own source colours
    and flags) a request the env's world refuses is replaced, in `case`, by a fresh draw that it accepts and a joint action drawn from
    its masks.  Returns ghost [n, A]: dead without a death event, which LLE's `done` does not count (env.py:208-217)."""
    n, A = ob.n, case.A
    ghost = np.zeros((n, A), bool)
    ev_count, events = np.zeros(n, np.uint8), np.zeros((n, 2 * A, 2), np.uint8)
    geo = None
    for e in range(n):
        w = ob.world(e)
        k = lo + e
        tries = 0
        while True:
            try:
                ev = w.set_state([tuple(int(v) for v in p) for p in case.pos[k]], [bool(v) for v in case.gems[k]], [bool(v) for v in case.alive[k]])
                break
            except oracle_mod.OracleError:
                if rng is None:
                    raise
            tries += 1
            if tries > MAX_TRIES:
                raise RuntimeError(f"{case.name}: env {k} found no state its own sources accept in {MAX_TRIES} draws")
            geo = geo or Geometry(w)
            w.reset()  # (a refused request leaves the reference's world with stale availability lists)
            pos, gems, alive = random_state(rng, geo.walkable, A, case.G)
            case.pos[k], case.gems[k], case.alive[k] = np.array(pos, np.uint8), gems, alive
            case.actions[k] = STAY
        if tries:
            masks = w.available_mask()
            case.actions[k] = [[q for q in range(5) if (m >> q) & 1][int(rng.integers(bin(m & 31).count("1")))] for m in masks]
        died = {a for (ty, a) in ev if ty == EV_DIED}
        ghost[e] = [not case.alive[k][a] and a not in died for a in range(A)]
        ev_count[e] = len(ev)
        if ev:
            events[e, :len(ev)] = ev
    if record is not None:
        record["ev_count"], record["events"] = ev_count, events
    return ghost


def done_of(dump, ghost):
    """LLE.compute_done from the oracle's flags: somebody died by an event, or everybody has arrived."""
    return ((dump["alive"] == 0) & ~ghost).any(1) | (dump["arrived"] != 0).all(1)


def reward_counts(ostep, dump):
    """[gems, exits, deaths, everybody arrived] of a step from the oracle's events (tests/test_gpu_parity.py
    test_reward_counts_and_snapshot); a refused step is no step of the reference (it raises): no event, no bonus."""
    cnt = (ostep["ev_count"] & 0x7F).astype(np.int64)
    valid = np.arange(ostep["events"].shape[1])[None, :] < cnt[:, None]
    ty = ostep["events"][:, :, 0]
    bonus = (dump["arrived"] != 0).all(1) & (ostep["err"] == 0)
    return np.stack([((ty == EV_GEM) & valid).sum(1), ((ty == EV_EXIT) & valid).sum(1), ((ty == EV_DIED) & valid).sum(1), bonus.astype(np.int64)], axis=1)


def classify(case, geo, d0, ostep, d1):
    """Class flags per env (bool [n]) of the explicit step, from the oracle: d0 / d1 = dump() before / after, ostep = step()."""
    A = case.A
    ok = ostep["err"] == 0
    cnt = (ostep["ev_count"] & 0x7F).astype(np.int64)
    valid = np.arange(ostep["events"].shape[1])[None, :] < cnt[:, None]
    ty, ag = ostep["events"][:, :, 0], ostep["events"][:, :, 1].astype(np.int64)
    n_died, n_gem, n_exit = ((ty == EV_DIED) & valid).sum(1), ((ty == EV_GEM) & valid).sum(1), ((ty == EV_EXIT) & valid).sum(1)
    f = {"stepped": ok}
    for a in range(A):
        f[f"refused-by-{a}"] = ostep["err"] == 1 + a
    f["events-0"], f["events-1"], f["events-2"], f["events-3+"] = ok & (cnt == 0), cnt == 1, cnt == 2, cnt >= 3
    f["event-exit"], f["event-gem"], f["event-died"] = n_exit > 0, n_gem > 0, n_died > 0
    f["gem-with-death"], f["exit-with-death"], f["two-deaths"] = (n_gem > 0) & (n_died > 0), (n_exit > 0) & (n_died > 0), n_died >= 2
    f["id-inversion"] = ((ag[:, 1:] < ag[:, :-1]) & valid[:, 1:]).any(1)
    pos0, pos1 = d0["pos"].astype(np.int64), d1["pos"].astype(np.int64)
    act = np.minimum(ostep["actions"].astype(np.int64), 4)
    tgt = pos0 + ACTION_DELTA[act]
    key, here = tgt[..., 0] * 1024 + tgt[..., 1], pos0[..., 0] * 1024 + pos0[..., 1]
    alive0, alive1 = d0["alive"] != 0, d1["alive"] != 0
    mover = alive0 & (act != STAY)
    # a conflict between MOVERS: living agents that leave their cell for the same one (a corpse or an agent that stays does not count)
    mult = ((key[:, :, None] == key[:, None, :]) & mover[:, :, None] & mover[:, None, :]).sum(2).max(1)
    f["same-target-2"], f["same-target-3"] = ok & (mult >= 2), ok & (mult >= 3)
    buried = ~alive0 & (d0["occupant"] == 0)
    f["onto-corpse"] = ok & ((key[:, :, None] == here[:, None, :]) & mover[:, :, None] & buried[:, None, :]).any((1, 2))
    b0, b1 = d0["beams"], d1["beams"]
    if b0.shape[1]:
        pad = (-b0.shape[2]) % 32
        on = np.pad((b0 == 0) & (b1 != 0), ((0, 0), (0, 0), (0, pad))).reshape(b0.shape[0], b0.shape[1], -1, 32).any(3)
        off = np.pad((b0 != 0) & (b1 == 0), ((0, 0), (0, 0), (0, pad))).reshape(b0.shape[0], b0.shape[1], -1, 32).any(3)
        f["beam-off-on"], f["beam-on-off"], f["beam-both-in-word"] = on.any((1, 2)), off.any((1, 2)), (on & off).any((1, 2))
        ch = on | off
        f["chain-carry"] = (ch[:, :, :-1] & ch[:, :, 1:]).any((1, 2)) if ch.shape[2] > 1 else np.zeros(len(ok), bool)
    else:
        for k in ("beam-off-on", "beam-on-off", "beam-both-in-word", "chain-carry"):
            f[k] = np.zeros(len(ok), bool)
    arr0, arr1 = (d0["arrived"] != 0).all(1), (d1["arrived"] != 0).all(1)
    f["last-arrival"] = ok & ~arr0 & arr1
    f["nobody-left-alive"] = ok & alive0.any(1) & ~alive1.any(1)
    f["one-active-agent"] = ok & ((alive0 & (d0["arrived"] == 0)).sum(1) == 1)
    if case.name == "four_layers":
        for a in range(A):
            f[f"four-layer-cell-{a}"] = ok & (pos0[:, a, 0] == 2) & (pos0[:, a, 1] == 2)
    if case.name == "gems32":
        gi, gj = geo.gems[31]
        enters = ((pos1[..., 0] == gi) & (pos1[..., 1] == gj) & ((pos0[..., 0] != gi) | (pos0[..., 1] != gj)) & alive1).any(1)
        f["gem31-taken"] = ok & enters & (d0["gems"][:, 31] == 0) & (d1["gems"][:, 31] != 0)
        f["gem31-already-set"] = ok & enters & (d0["gems"][:, 31] != 0)
    return f


# what a lane group's maps must show between them
CLASSES_ANY = ["stepped", "events-0", "events-1", "event-exit", "event-gem", "event-died", "last-arrival", "nobody-left-alive", "one-active-agent",
               "beam-off-on", "beam-on-off"]
# What ONE agent cannot show: a second event in a step, a second death, events out of order, a shared target, a corpse besides a living
# agent, and a cut and a re-light in one beam word -- a lone owner moves the end of its beam one way per step (re-light at the cell it
# leaves, cut at the cell it enters, a prefix pattern before and after); the other direction in the same step takes a second agent's
# re-light in a later pass.
CLASSES_TWO = ["events-2", "gem-with-death", "exit-with-death", "two-deaths", "id-inversion", "same-target-2", "onto-corpse", "beam-both-in-word"]
CLASSES_THREE = ["events-3+", "same-target-3"]


def required_classes(n_agents_max):
    return CLASSES_ANY + (CLASSES_TWO if n_agents_max >= 2 else []) + (CLASSES_THREE if n_agents_max >= 3 else [])


def structural_classes(name, A):
    """Classes asserted on one map by itself."""
    out = [f"refused-by-{a}" for a in range(A)]
    if name in CHAINED:
        out.append("chain-carry")
    if name == "four_layers":
        out += [f"four-layer-cell-{a}" for a in range(A)]
    if name == "gems32":
        out += ["gem31-taken", "gem31-already-set"]
    return out


def run_oracle(oracle_mod, case, sources=None, rng=None, record=None):
    """An oracle batch with the case's states applied: (ob, ghost, dump after set_state).  `sources(ob)` may re-colour / switch the
    worlds' sources first (then `rng` replaces what an env's world refuses); `record`: see apply_states."""
    ob = oracle_mod.OracleBatch(case.text, case.n)
    if sources is not None:
        sources(ob)
    ghost = apply_states(oracle_mod, ob, case, 0, rng, record)
    return ob, ghost, ob.dump()


def coverage(oracle_mod, case):
    """{class: number of envs} of the case's explicit step, from the oracle alone."""
    ob, _ghost, d0 = run_oracle(oracle_mod, case)
    ostep = ob.step(case.actions, want_obs=False)
    flags = classify(case, Geometry(ob.world0), d0, ostep, ob.dump())
    return {k: int(v.sum()) for k, v in flags.items()}


@functools.lru_cache(maxsize=None)
def _built(name, variant):
    from oracle import oracle as oracle_mod
    oracle_mod.build()
    text = text_of(name, variant)
    w = oracle_mod.OracleWorld(text)
    geo = Geometry(w)
    A, G = geo.A, geo.G
    rng = np.random.default_rng([GROUP_OF[name], MAP_NAMES.index(name), variant, 2024])
    # ---- planted states: candidates the oracle accepts, stepped by the oracle, kept while they show a class that is still wanted
    cands = [c for c in _plant_candidates(name, geo, rng) if _accept(oracle_mod, w, c[1], c[2], c[3]) is not None]
    planted = []
    if cands:
        probe = Case(name, text, A, G, np.array([c[1] for c in cands], np.uint8).reshape(len(cands), A, 2), np.array([c[2] for c in cands], bool).reshape(len(cands), G),
                     np.array([c[3] for c in cands], bool).reshape(len(cands), A), np.array([c[4] for c in cands], np.uint8).reshape(len(cands), A),
                     np.arange(len(cands)), 0)
        ob, _ghost, d0 = run_oracle(oracle_mod, probe)
        ostep = ob.step(probe.actions, want_obs=False)
        flags = classify(probe, geo, d0, ostep, ob.dump())
        wanted = [k for k in required_classes(A) + structural_classes(name, A) if not k.startswith("refused")]
        chosen = []  # in order of priority: the cap below cuts from the end
        for tag in ("q1", "cascade3"):  # kept whatever they show: the pass counts of the CPU suite are taken on them
            chosen += [k for k, c in enumerate(cands) if c[0] == tag and ostep["err"][k] == 0][:2]
        for cls in wanted:
            hits = [int(k) for k in np.nonzero(flags[cls])[0]]
            chosen += [k for k in hits if k not in chosen][:max(0, 2 - sum(k in chosen for k in hits))]
        assert len(chosen) <= MAX_PLANTED, (name, len(chosen))
        planted = [cands[k] for k in chosen]
    # ---- random states
    states = [(c[1], c[2], c[3], c[4], c[0]) for c in planted]
    tries = 0
    while len(states) < len(planted) + N_RANDOM_STATES[A]:
        tries += 1
        if tries > MAX_TRIES * N_RANDOM_STATES[A]:
            raise RuntimeError(f"{name}: the oracle accepted {len(states) - len(planted)} of {tries} random states")
        pos, gems, alive = random_state(rng, geo.walkable, A, G)
        if _accept(oracle_mod, w, pos, gems, alive) is not None:
            states.append((pos, gems, alive, None, "random"))
    # ---- one env per (state, joint action)
    P, Gm, Al, Ac, St = [], [], [], [], []
    for s, (pos, gems, alive, act, _tag) in enumerate(states):
        masks = _accept(oracle_mod, w, pos, gems, alive)
        acts = ([act] if act is not None else []) + joint_actions(rng, masks, s)
        for row in acts:
            P.append(pos), Gm.append(gems), Al.append(alive), Ac.append(row), St.append(s)
    total = len(P)
    assert total < MAX_ENVS, (name, total)
    case = Case(name, text, A, G, np.array(P, np.uint8).reshape(total, A, 2), np.array(Gm, bool).reshape(total, G), np.array(Al, bool).reshape(total, A),
                np.array(Ac, np.uint8).reshape(total, A), np.array(St, np.int64), len(planted))
    case.planted_tags = [c[0] for c in planted]
    return case


def build_case(name, variant=0, n=None):
    """The case of a map, truncated to `n` envs (default: the largest 16 m + 5 it holds).  Deterministic; the arrays are copies."""
    full = _built(name, variant)
    case = full.truncated(ragged(full.n) if n is None else n)
    case.planted_tags = list(full.planted_tags)
    return case


def cascade_states(name):
    """(positions, gems, alive, joint action) of the planted Q1 / cascade states of a map: the CPU suite counts move_agents passes on them."""
    full = _built(name, 0)
    out = []
    for s, tag in enumerate(full.planted_tags):
        if tag in ("q1", "cascade", "cascade3"):
            k = int(np.nonzero(full.state_of == s)[0][0])  # (a planted state's own joint action is its first env)
            out.append((full.pos[k], full.gems[k], full.alive[k], full.actions[k]))
    return out


# ---- the protocol every engine is put through: set_state, the explicit step, two sampled steps without auto-reset (they start from
# stale beams and corpses no set_state can produce), one sampled step with auto-reset (finished envs restart)
SEED, ENV_OFFSET = 77, 3
FOLLOW_UPS = [(1, False), (2, False), (3, True)]   # (t, auto_reset) of the sampled steps


class Reference:
    """The oracle's side of the protocol, computed once per case: `after_set_state` and `steps[k]` are records with
    dump / done / ghost (+ the events set_state returned, + ostep / reward for steps, + whatever `extras(ob)` returned)."""


def reference_run(oracle_mod, case, sources=None, rng=None, env_offset=ENV_OFFSET, extras=None, follow_ups=None):
    ref = Reference()
    returned = {}
    ob, ghost, d0 = run_oracle(oracle_mod, case, sources, rng, returned)
    ref.ob, ref.case = ob, case
    ref.after_set_state = {"dump": d0, "ev_count": returned["ev_count"], "events": returned["events"], "ghost": ghost.copy(), "done": done_of(d0, ghost), "extras": extras(ob) if extras else None,
                           "obs": np.stack([ob.world(e).obs() for e in range(case.n)])}
    ref.steps = []
    plan = [(0, False, case.actions)] + [(t, auto, None) for t, auto in (FOLLOW_UPS if follow_ups is None else follow_ups)]
    for t, auto, acts in plan:
        ostep = ob.step(acts, auto_reset=auto, seed=SEED, t=t, env_offset=env_offset)
        ghost = ghost & ((ostep["ev_count"] & 0x80) == 0)[:, None]  # (an auto-reset clears the bookkeeping)
        dump = ob.dump()
        ref.steps.append({"t": t, "auto_reset": auto, "actions": acts, "ostep": ostep, "dump": dump, "ghost": ghost.copy(), "done": done_of(dump, ghost),
                          "reward": reward_counts(ostep, dump), "extras": extras(ob) if extras else None})
    return ref


# Four agents with every direction in their availability lists at the start cells, a beam of colour 0 to die on.  A set_state request
# that puts agent 3, alive, on that beam is refused with InvalidWorldState and NOT rolled back: the agents stand where they were asked to
# and the lists are those of the start cells.  [East, West, North, Stay] then sends agents 0 and 1 onto one cell and agent 2 onto the
# cell agent 0 is sent back to -- the one situation in which solve_vertex_conflicts (world.rs:365-378) needs its second round.
STALE_MAP = (". . . . . X\n. S0 . S1 . X\n. . . . . X\n. S2 . S3 . X\n. . . . . .\nL0E . . . . .")
STALE_REQUEST = ([(2, 1), (2, 3), (3, 1), (5, 2)], [], [True, True, True, True])
STALE_ACTIONS = [2, 3, 0, 4]
