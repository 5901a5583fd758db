"""The rollout driver of tests/test_gpu_coopcycles.py and of the CPU replay of its plans in tests/test_coopcycles_cpu.py -- TEST
INFRASTRUCTURE.

Random play never closes a trail of order 3 or more, so a stated share of the environments (every second one) replays, from each
reset, a PLAN that the restatement says closes one: the shortest plan of `search_ref.search(text, t_max)` ("standard": no
restriction), which on a world that is interdependent over all its agents has to close a trail over all of them;
`cycles_ref.check_plan(..., closed_orders=...)` asserts the orders it closes through the package's host-side graph class.  The other
environments play at random, as in tests/test_gpu_cooptrails.play.

`play(..., gpu=False)` runs the oracle side alone: the coverage counts in the docstrings of the GPU tests are its results, and the CPU
test asserts them.
"""
import json
import os

import numpy as np
import pytest

from tests import coop_ref, coopcycles_ref, cooptrails_ref, cycles_ref, search_ref
from tests.oracle_env import OracleLLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = {c["name"]: c["map"] for c in json.load(open(os.path.join(ROOT, "tests", "golden", "kat_trails.json")))["catalogue"] if "map" in c}
PAPER3 = MAPS["paper-interdependent-3"]
PAPER3_OPEN = PAPER3.replace(" @   .    @   .   .  @", " @   .    .   .   .  @", 1)  # a wall the shortest plan does not pass: another map of the same shape
CYCLE3 = MAPS["three-agent-temporal-cycle"]
FOUR = MAPS["four-agent-interdependent-4-sequence-6"]
# map -> (horizon of the search, the closed orders of its shortest plan)
PLANNED = {PAPER3: (10, [3]), PAPER3_OPEN: (10, [3]), CYCLE3: (15, [2, 3]), FOUR: (14, [2, 3, 4])}
CLOSED_NAMES = ("episode_closed", "last_closed", "episode_cprofile", "last_cprofile")
COVER_KEYS = ("finished_top", "running_top", "order2_only", "refused_scripted", "chained", "edges")

_PLANS = {}


def plan_of(text):
    """The shortest plan of `text` (rows of action values), checked: it closes exactly the orders PLANNED names, the map's agents among
    them."""
    if text not in _PLANS:
        t_max, orders = PLANNED[text]
        res = search_ref.search(text, t_max)
        n_agents = len(res.plan[0])
        R = cycles_ref.check_plan(text, res.plan, n_agents + 1, length=res.length, closed_orders=orders)
        assert n_agents in orders and coopcycles_ref.closed_orders(R) == orders
        _PLANS[text] = res.plan
    return _PLANS[text]


def compare_closed(tracker, crefs, where):
    import torch
    cols = list(zip(*[r.arrays() for r in crefs]))
    want = [torch.tensor(cols[k], dtype=torch.int32).t().contiguous() for k in range(2)] + [torch.tensor(cols[k], dtype=torch.uint8) for k in (2, 3)]
    for name, want_k in zip(CLOSED_NAMES, want):
        got = getattr(tracker, name).cpu()
        if not torch.equal(got, want_k):
            diff = got != want_k
            bad = int((diff.any(dim=0) if name.endswith("closed") else diff.any(dim=1)).nonzero()[0])
            got_b, want_b = (got[:, bad], want_k[:, bad]) if name.endswith("closed") else (got[bad], want_k[bad])
            raise AssertionError(f"{where}: {name} differs in env {bad}: {got_b.tolist()} != {want_b.tolist()}")


def play(oracle_mod, texts, per_map, steps, seed, scripted=True, randomize=False, step_kw=None, reset_by="auto", gpu=True, set_state_at=None,
         unavailable=0.0):
    """One rollout of len(texts) * per_map environments (map m owns block m) against one oracle world and one EnvRef of coop_ref,
    cooptrails_ref and coopcycles_ref per environment; EVERY buffer of the tracker compared (torch.equal) after every step.  With
    `scripted`, every second environment replays plan_of(its map) from each reset -- a refused step is repeated --, and plays at random
    once the plan is through; the others play at random.  The other arguments as in tests/test_gpu_cooptrails.play.  Returns the
    coverage counted from the restatement alone:
      finished_top      episodes that finished with a closed trail over ALL the map's agents (in last_cprofile from then on)
      running_top       environment-steps whose running episode holds one
      order2_only       environment-steps whose running episode has closed order 2 and nothing else
      refused_scripted  refused steps inside a scripted episode
      chained           updates that entered two layers (the start edges and the state's) in one launch
      edges             environment-steps whose state has an arc"""
    n = per_map * len(texts)
    step_kw = dict(step_kw or {})
    worlds = [oracle_mod.OracleWorld(texts[e // per_map]) for e in range(n)]
    A, L, G = worlds[0].n_agents, worlds[0].n_sources, worlds[0].n_gems
    lles = [OracleLLE(w) for w in worlds]
    for r in lles:
        r.free_running = True
    refs = [coop_ref.EnvRef(A) for _ in range(n)]
    trefs = [cooptrails_ref.EnvRef(A) for _ in range(n)]
    crefs = [coopcycles_ref.EnvRef(A) for _ in range(n)]
    plans = [plan_of(texts[e // per_map]) if scripted and e % 2 == 0 else None for e in range(n)]
    at = [0] * n  # the next row of the plan
    rng = np.random.default_rng(seed)
    cover = dict.fromkeys(COVER_KEYS, 0)
    env = None
    if gpu:
        import torch

        from lle_amd import BatchedLLE
        from lle_amd.coopcycles import ClosedTrailCooperationTracker
        from tests.test_gpu_cooptrails import compare
        env = BatchedLLE(texts if len(texts) > 1 else texts[0], n, randomize_lasers=randomize, seed=seed, cooperation="closed-trails")
        first_words = env.world.map.source_first_words()
        assert isinstance(env.cooperation, ClosedTrailCooperationTracker) and env.cooperation.n_envs == n

    def colours_now():
        return env.world.src_colour.cpu().numpy()[:, first_words]

    def all_three(e, ops, state=(), starts=(), was_reset=False, refused=False):
        refs[e].update(ops, state, start_edges=starts, was_reset=was_reset)
        trefs[e].update(ops, state, start_edges=starts, was_reset=was_reset, refused=refused)
        crefs[e].update(ops, state, start_edges=starts, was_reset=was_reset, refused=refused)

    def check(where):
        compare(env.cooperation, refs, trefs, where)
        compare_closed(env.cooperation, crefs, where)

    cols = None
    if gpu:
        env.reset()
        cols = colours_now() if randomize else None
    for e, r in enumerate(lles):
        r.reset(cols[e] if cols is not None else None)
        # BatchedLLE marks the state of its construction (CLEAR | MARK_POS), then reset() finishes that episode and marks again
        all_three(e, coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(oracle_mod.OracleWorld(texts[e // per_map])))
        all_three(e, coop_ref.FINISH | coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(r.w))
    if gpu:
        check("after reset")
    for t in range(steps):
        over = np.array([r.done for r in lles])
        resetting = [int(e) for e in np.nonzero(over)[0]] if reset_by != "none" else []
        in_kernel_colours = randomize and reset_by == "auto"  # drawn by the step kernel: known only after the step
        if gpu and reset_by == "mask" and resetting:
            env.reset(env_mask=torch.from_numpy(over.astype(np.uint8)).cuda())
            cols = colours_now() if randomize else None
        starts = {}
        for e in resetting:
            cover["finished_top"] += A in crefs[e].orders()
            lles[e].reset(cols[e] if (cols is not None and reset_by == "mask") else None)
            at[e] = 0
            if reset_by == "mask":
                all_three(e, coop_ref.FINISH | coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(worlds[e]))
            elif not in_kernel_colours:
                starts[e] = coop_ref.detect(worlds[e])
        actions = np.zeros((n, A), np.uint8)
        bad = rng.random(n) < unavailable
        for e, w in enumerate(worlds):
            masks = w.available_mask()
            for a, mask in enumerate(masks):  # (drawn for every environment: the random ones do not depend on the share of scripted ones)
                opts = [k for k in range(5) if (mask >> k) & 1]
                actions[e, a] = opts[int(rng.integers(len(opts)))]
            if plans[e] is not None and at[e] < len(plans[e]):
                actions[e] = plans[e][at[e]]
                assert all((masks[a] >> int(actions[e, a])) & 1 for a in range(A)), "the plan's row is not available"
            closed = [k for k in range(5) if not (masks[0] >> k) & 1]
            bad[e] = bad[e] and bool(closed)
            if bad[e]:
                actions[e, 0] = closed[int(rng.integers(len(closed)))]
        if gpu:
            out = env.step(torch.from_numpy(actions).cuda(), auto_reset=(reset_by == "auto"), **step_kw)
            assert ((out["err"] != 0).cpu().numpy() == bad).all(), f"t={t}: the refused steps are not the ones handed an unavailable action"
            if in_kernel_colours:
                cols = colours_now()
        if in_kernel_colours:
            for e in resetting:  # LLE.reset: world.reset() under the colours the env had, then the new ones on the live world
                for l in range(L):
                    if cols is not None:
                        worlds[e].set_source(l, colour=int(cols[e][l]))
                starts[e] = coop_ref.detect(worlds[e])
        for e, r in enumerate(lles):
            in_plan = plans[e] is not None and at[e] < len(plans[e])
            if bad[e]:
                with pytest.raises(oracle_mod.OracleError):
                    r.step(actions[e])
                cover["refused_scripted"] += in_plan
            else:
                r.step(actions[e])
                at[e] += in_plan
            all_three(e, coop_ref.MARK_POS, coop_ref.detect(r.w), starts.get(e, ()), was_reset=reset_by == "auto" and e in starts, refused=bool(bad[e]))
            orders = crefs[e].orders()
            cover["running_top"] += A in orders
            cover["order2_only"] += orders == [2]
            cover["chained"] += crefs[e].layers >= 2
            cover["edges"] += len(refs[e].step) >= 1
        if gpu:
            check(f"t={t}")
        if set_state_at is not None and t == set_state_at:
            pos = [w.positions() for w in worlds]
            gems = [w.gems_collected() for w in worlds]
            alive = [w.alive() for w in worlds]
            if gpu:
                err = env.set_state(torch.tensor(pos, dtype=torch.uint8), torch.tensor(gems, dtype=torch.bool).reshape(n, G), torch.tensor(alive, dtype=torch.bool))
                ok = (err == 0).cpu().numpy()
            else:
                ok = np.ones(n, bool)
            for e, r in enumerate(lles):
                try:
                    r.set_state(pos[e], gems[e], alive[e])
                    assert ok[e]
                except oracle_mod.OracleError:
                    assert not ok[e]
                all_three(e, coop_ref.MARK_POS, coop_ref.detect(r.w))  # (after set_state no SKIP_REFUSED: the state handed in is one more state)
            if gpu:
                check(f"after set_state at t={t}")
    if gpu:  # the queries, against the restatement and against the parent's derivation from the flattened edges
        from lle_amd.cooptrails import TemporalCooperationTracker
        tr = env.cooperation
        assert tr.closed_orders().cpu().tolist() == [coopcycles_ref.orders_byte(r.R) for r in crefs]
        assert tr.closed_orders(last=True).cpu().tolist() == [coopcycles_ref.orders_byte(r.last_R) for r in crefs]
        for k in range(0, 8):
            assert tr.is_interdependent(k).cpu().tolist() == [k in r.orders() for r in crefs]
            assert tr.is_interdependent(k, last=True).cpu().tolist() == [r.last_valid and k in r.orders(last=True) for r in crefs]
        for last in (False, True):
            flattened = TemporalCooperationTracker.is_interdependent(tr, 2, last=last)
            assert tr.is_mutual(last=last).cpu().tolist() == tr.is_interdependent(2, last=last).cpu().tolist() == flattened.cpu().tolist()
        assert bool(tr.closed_exact().all()) and bool(tr.closed_exact(last=True).all())
        for e in (0, 1, n - 1):
            assert tr.triples(e) == set(crefs[e].R) and tr.triples(e, last=True) == set(crefs[e].last_R)
    return cover


def line3():
    """Three agents that start on one beam: the reset state has the arcs 0 -> 1 and 0 -> 2 (tests/test_gpu_coop.line_map(3))."""
    return "L0E S0 S1 S2 @\nX X X . ."


# The rollouts of tests/test_gpu_coopcycles.py: name -> (arguments of play, the coverage play(gpu=False) gives with them).  The GPU
# tests assert at least these counts, from the restatement alone; tests/test_coopcycles_cpu.py asserts that the oracle-only run gives
# exactly them.
ROLLOUTS = {
    "paths": (dict(texts=[PAPER3], per_map=16, steps=30, seed=81, unavailable=0.1),
              dict(finished_top=24, running_top=26, order2_only=0, refused_scripted=28, chained=0, edges=149)),
    "resets_auto": (dict(texts=[CYCLE3], per_map=64, steps=60, seed=82, unavailable=0.1, reset_by="auto"),
                    dict(finished_top=174, running_top=386, order2_only=209, refused_scripted=190, chained=0, edges=1944)),
    "resets_mask": (dict(texts=[CYCLE3], per_map=64, steps=60, seed=82, unavailable=0.1, reset_by="mask"),
                    dict(finished_top=174, running_top=386, order2_only=209, refused_scripted=190, chained=0, edges=1944)),
    "resets_none": (dict(texts=[CYCLE3], per_map=64, steps=60, seed=82, unavailable=0.1, reset_by="none"),
                    dict(finished_top=0, running_top=1670, order2_only=34, refused_scripted=32, chained=0, edges=309)),
    "four": (dict(texts=[FOUR], per_map=64, steps=60, seed=83, unavailable=0.05),
             dict(finished_top=114, running_top=381, order2_only=1388, refused_scripted=108, chained=0, edges=1278)),
    "two_maps": (dict(texts=[PAPER3, PAPER3_OPEN], per_map=32, steps=40, seed=84),
                 dict(finished_top=160, running_top=160, order2_only=0, refused_scripted=0, chained=0, edges=769)),
    "set_state": (dict(texts=[PAPER3], per_map=16, steps=20, seed=85, set_state_at=8),
                  dict(finished_top=16, running_top=16, order2_only=0, refused_scripted=0, chained=0, edges=92)),
    "chain": (dict(texts=[line3()], per_map=32, steps=30, seed=87, scripted=False, unavailable=0.1),
              dict(finished_top=0, running_top=0, order2_only=0, refused_scripted=0, chained=80, edges=243)),
}
