"""BatchedLLE(cooperation=True) -- the coop kernel, lle_amd/coop/coop.hip -- against the restatement of the rule on oracle worlds
(tests/coop_ref.py): the reference's own worlds (tests/golden/kat_coop.json) and differential rollouts in which EVERY buffer of the
tracker (step / episode / last edges, both profiles) is compared exactly (torch.equal) after every step.

The rollouts' actions come from the oracle side (uniform over each agent's available actions, numpy generator), so a rollout is the
same on every box; `play(..., gpu=False)` runs the oracle side alone.  Random play rarely cooperates: every rollout asserts that the
restatement saw at least MIN_HITS environment-steps with a non-empty edge set, and the shapes and seeds below were chosen with
play(gpu=False) so that it does (the counts are written next to them)."""
import numpy as np
import pytest

from oracle.levels import LEVELS
from tests import coop_ref
from tests.oracle_env import OracleLLE

pytestmark = pytest.mark.gpu

CASES = coop_ref.load_cases()
WORLDS = {c["name"]: c for c in CASES["worlds"]}
EIGHT = WORLDS["eight-agent-interdependent-8"]["map"]
PERIMETER = WORLDS["eight-agent-interdependent-8-perimeter"]["map"]
RING8 = {(h, (h + 1) % 8) for h in range(8)}
MIN_HITS = 20
STEP_PATHS = {"default": {}, "fused": dict(fused=True), "two_launches": dict(fused=False), "persistent": dict(persistent=True)}


def line_map(n_agents, variant=0):
    """Every agent starts on the one beam, agent 0 -- its colour -- nearest the source: it blocks, the others are helped from the
    reset on.  `variant` closes a corner cell that no exit needs: another map of the same shape for batches of several maps."""
    top = ["L0E"] + [f"S{a}" for a in range(n_agents)] + ["@"]
    bottom = ["X"] * n_agents + [".", "@" if variant else "."]
    return " ".join(top) + "\n" + " ".join(bottom)


# three beams over cell (2, 2) -- the deepest source owns no tile there --; agent 0 blocks for agent 1 from the reset on, and whoever
# stands on (2, 2) blocks (or not) for an agent further down the vertical beams
THREE_BEAM_COOP = ". . L2S . .\n. . . S2 .\nL0E S0 . S1 @\n. . . . .\nX X L0N X ."
# a source whose colour is no agent (3 >= n_agents) across the beam of agent 0: it never blocks
COLOUR_BEYOND = "L0E S0 S1 . @\n. . . L3S .\n. . . . .\nX X . . ."
# the same shape with the crossing source disabled and a second source of agent 1's colour
DISABLED = "L0E S0 S1 . @\n. . . L1S .\n. . . . .\nX X . . ."


# ---------------------------------------------------------------------------------------------- comparisons
def tracker_arrays(tracker):
    return [t.cpu() for t in (tracker.step_edges, tracker.episode_edges, tracker.last_edges, tracker.episode_profile, tracker.last_profile)]


def ref_arrays(refs, idx=None):
    import torch
    cols = list(zip(*[r.arrays() for r in refs]))
    out = [torch.tensor(cols[k], dtype=torch.int32) for k in range(3)] + [torch.tensor(cols[k], dtype=torch.uint8) for k in (3, 4)]
    return out if idx is None else [t[idx] for t in out]


NAMES = ("step_edges", "episode_edges", "last_edges", "episode_profile", "last_profile")


def compare(tracker, refs, where, idx=None):
    import torch
    for name, got, want in zip(NAMES, tracker_arrays(tracker), ref_arrays(refs, idx)):
        if not torch.equal(got, want):
            bad = int((got != want).flatten(1).any(dim=1).nonzero()[0])
            raise AssertionError(f"{where}: {name} differs in env {bad}: {got[bad].tolist()} != {want[bad].tolist()}")


# ---------------------------------------------------------------------------------------------- differential rollouts
def play(oracle_mod, texts, per_map, steps, seed, randomize=False, step_kw=None, reset_by="auto", shaping=False, gpu=True, min_hits=MIN_HITS,
         prepare=None, set_state_at=None, own_beam_hits=False):
    """One rollout of len(texts) * per_map environments (map m owns block m) against one oracle world and one coop_ref.EnvRef per
    environment.  reset_by: "auto" = step(auto_reset=True); "mask" = reset(env_mask=done) ahead of a plain step; "none" = plain steps,
    a finished environment goes on with whatever its agents may still do.  prepare(env, refs): applied to both sides after the first reset
    (per-environment sources).  set_state_at: step after which every environment is handed its own current positions through
    set_state (the episode continues).  Returns the number of environment-steps with a non-empty edge set (own_beam_hits: with an agent
    on an enabled beam of its own colour, for maps of one agent)."""
    n = per_map * len(texts)
    step_kw = dict(step_kw or {})
    worlds = [oracle_mod.OracleWorld(texts[e // per_map]) for e in range(n)]
    A, L, G = worlds[0].n_agents, worlds[0].n_sources, worlds[0].n_gems
    lles = [OracleLLE(w) for w in worlds]
    for r in lles:
        r.free_running = True
    refs = [coop_ref.EnvRef(A) for _ in range(n)]
    rng = np.random.default_rng(seed)
    env = None
    if gpu:
        import torch

        from lle_amd import BatchedLLE, LaserSubgoal, PotentialShapedLLE, SingleObjective
        kw = dict(reward_strategy=PotentialShapedLLE(SingleObjective()), extras_generator=LaserSubgoal()) if shaping else {}
        env = BatchedLLE(texts if len(texts) > 1 else texts[0], n, randomize_lasers=randomize, seed=seed, cooperation=True, **kw)
        first_words = env.world.map.source_first_words()
        assert env.cooperation is not None and env.cooperation.n_envs == n

    def colours_now():
        return env.world.src_colour.cpu().numpy()[:, first_words]

    def hit(e):
        if own_beam_hits:
            w = worlds[e]
            return any(en and col == w.tile_agent(i, j) for i, j, _l, col, _on, en in w.lasers())
        return bool(refs[e].step)

    cols = None
    if gpu:
        env.reset()
        cols = colours_now() if randomize else None
    for e, r in enumerate(lles):
        r.reset(cols[e] if cols is not None else None)
        # BatchedLLE marks the state of its construction (CLEAR | MARK_POS), then reset() finishes that episode and marks again
        refs[e].update(coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(oracle_mod.OracleWorld(texts[e // per_map])))
        refs[e].update(coop_ref.FINISH | coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(r.w))
    if prepare is not None:
        prepare(env, lles, refs)
    if gpu:
        compare(env.cooperation, refs, "after reset")
    hits = sum(hit(e) for e in range(n))
    for t in range(steps):
        over = np.array([r.done for r in lles])
        resetting = [int(e) for e in np.nonzero(over)[0]] if reset_by != "none" else []
        in_kernel_colours = randomize and reset_by == "auto"  # drawn by the step kernel: known only after the step
        if gpu and reset_by == "mask" and resetting:
            env.reset(env_mask=torch.from_numpy(over.astype(np.uint8)).cuda())
            cols = colours_now() if randomize else None
        # the oracle side resets first: the actions of a reset environment are drawn from what is available in its reset state (which
        # does not depend on the colours: World.available_actions ignores the beams)
        starts = {}
        for e in resetting:
            lles[e].reset(cols[e] if (cols is not None and reset_by == "mask") else None)
            if reset_by == "mask":
                refs[e].update(coop_ref.FINISH | coop_ref.CLEAR | coop_ref.MARK_POS, coop_ref.detect(worlds[e]))
            elif not in_kernel_colours:
                starts[e] = coop_ref.detect(worlds[e])
        actions = np.zeros((n, A), np.uint8)
        for e, w in enumerate(worlds):
            for a, mask in enumerate(w.available_mask()):
                opts = [k for k in range(5) if (mask >> k) & 1]
                actions[e, a] = opts[int(rng.integers(len(opts)))]
        if gpu:
            out = env.step(torch.from_numpy(actions).cuda(), auto_reset=(reset_by == "auto"), **step_kw)
            assert int(out["err"].max()) == 0, f"t={t}: an action was refused"
            if in_kernel_colours:
                cols = colours_now()
        if in_kernel_colours:
            for e in resetting:  # LLE.reset: world.reset() under the colours the env had, then the new ones on the live world
                for l in range(L):
                    if cols is not None:
                        worlds[e].set_source(l, colour=int(cols[e][l]))
                starts[e] = coop_ref.detect(worlds[e])
        for e, r in enumerate(lles):
            r.step(actions[e])
            refs[e].update(coop_ref.MARK_POS, coop_ref.detect(r.w), start_edges=starts.get(e, ()), was_reset=reset_by == "auto" and e in starts)
            hits += hit(e)
        if gpu:
            compare(env.cooperation, refs, f"t={t}")
        if set_state_at is not None and t == set_state_at:
            pos = [w.positions() for w in worlds]
            gems = [w.gems_collected() for w in worlds]
            alive = [w.alive() for w in worlds]
            if gpu:
                err = env.set_state(torch.tensor(pos, dtype=torch.uint8), torch.tensor(gems, dtype=torch.bool).reshape(n, G),
                                    torch.tensor(alive, dtype=torch.bool))
                ok = (err == 0).cpu().numpy()
            else:
                ok = np.ones(n, bool)
            for e, r in enumerate(lles):
                try:
                    r.set_state(pos[e], gems[e], alive[e])
                    assert ok[e]
                except oracle_mod.OracleError:
                    assert not ok[e]
                refs[e].update(coop_ref.MARK_POS, coop_ref.detect(r.w))
            if gpu:
                compare(env.cooperation, refs, f"after set_state at t={t}")
    assert hits >= min_hits, f"the rollout saw {hits} environment-steps with an edge: it proves too little"
    return hits


# (map, environments, steps, seed): with play(gpu=False) these see 71 / 67 / 39 / 73 environment-steps with an edge.  Level 5 cooperates
# least (9 to 19 in 1 024 x 40 over five seeds): it runs twice as long.
LEVEL_ROLLOUTS = [(3, 1024, 40, 31), (4, 1024, 40, 32), (5, 1024, 80, 33), (6, 1024, 40, 34)]


@pytest.mark.parametrize("level,n,steps,seed", LEVEL_ROLLOUTS, ids=[f"level{r[0]}" for r in LEVEL_ROLLOUTS])
def test_levels(oracle_mod, level, n, steps, seed):
    play(oracle_mod, [LEVELS[level]], n, steps, seed)


@pytest.mark.parametrize("auto", ["auto", "mask", "none"])
@pytest.mark.parametrize("name", ["eight", "perimeter"])
def test_eight_agent_layouts(oracle_mod, name, auto):
    """Every reset state carries the eight ring edges: the start edges of an auto-reset (a start cell on a beam: computed on a
    one-environment batch at create), the marked reset state of a masked reset, `last_*` across episode ends."""
    play(oracle_mod, [EIGHT if name == "eight" else PERIMETER], 64, 40, 41, reset_by=auto)


@pytest.mark.parametrize("shaping", [False, True], ids=["plain", "shaping"])
@pytest.mark.parametrize("path", sorted(STEP_PATHS))
def test_every_step_path(oracle_mod, path, shaping):
    play(oracle_mod, [EIGHT], 64, 30, 42, step_kw=STEP_PATHS[path], shaping=shaping)


@pytest.mark.parametrize("name,text", [("three_beam_cell", THREE_BEAM_COOP), ("colour_beyond_agents", COLOUR_BEYOND), ("disabled_source", DISABLED)])
def test_special_sources(oracle_mod, name, text):
    def prepare(env, lles, refs):
        if name != "disabled_source":
            return
        for r in lles:
            r.w.set_source(1, enabled=False)
        if env is not None:
            env.world.map.set_source(1, enabled=False)
            env.world.update_sources()
    play(oracle_mod, [text], 256, 40, 43, prepare=prepare)


def test_per_environment_sources(oracle_mod):
    """set_sources with per-environment colours and flags: the kernel reads LLE_BUF_SRC_COLOUR / LLE_BUF_SRC_ENABLED."""
    import torch
    text = "L0E . . . @\nS0 S1 S2 . .\nL1E . . . @\nX X X . ."
    n = 256
    rng = np.random.default_rng(5)
    colours = rng.integers(0, 3, (n, 2)).astype(np.uint8)
    enabled = rng.integers(1, 4, n).astype(np.int32)

    def prepare(env, lles, refs):
        for e, r in enumerate(lles):
            for l in range(2):
                r.w.set_source(l, colour=int(colours[e, l]), enabled=bool((enabled[e] >> l) & 1))
        if env is not None:
            env.world.set_sources(colours=torch.from_numpy(colours), enabled=torch.from_numpy(enabled))
            assert int(env.world.err.max()) == 0
    play(oracle_mod, [text], n, 40, 44, prepare=prepare, reset_by="none")


def test_randomize_lasers(oracle_mod):
    play(oracle_mod, [LEVELS[6]], 1024, 40, 45, randomize=True)


def test_randomize_lasers_with_masked_resets(oracle_mod):
    play(oracle_mod, [LEVELS[6]], 1024, 40, 46, randomize=True, reset_by="mask")


def test_set_state_mid_episode(oracle_mod):
    play(oracle_mod, [EIGHT], 64, 30, 47, set_state_at=10)


@pytest.mark.parametrize("n_agents,per_map", [(2, 3), (3, 5), (7, 3), (16, 3)])
def test_several_maps_with_an_odd_number_of_environments_each(oracle_mod, n_agents, per_map):
    """A workgroup spans several maps: the cell table stays in global memory (coop_kernel<G, false>) and env / envs_per_map picks it."""
    play(oracle_mod, [line_map(n_agents, v) for v in (0, 1, 0, 1)], per_map, 30, 48)


@pytest.mark.parametrize("n_agents", [2, 3, 7, 16])
def test_one_beam_for_everybody(oracle_mod, n_agents):
    """1 to 15 beneficiaries of one blocker from the reset on; 16 agents fill the lane group."""
    play(oracle_mod, [line_map(n_agents)], 64, 30, 49)
    play(oracle_mod, [line_map(n_agents, v) for v in (0, 1)], 64, 20, 50)  # (two maps, whole workgroups per map: the table in LDS)


def test_one_agent(oracle_mod):
    """One agent has nobody to help: every buffer stays empty -- the rollout asserts instead that the agent stood on its own enabled
    beam in at least MIN_HITS environment-steps -- in both table placements."""
    text = "L0E S0 . . X\n. . . . ."
    assert play(oracle_mod, [text], 64, 30, 51, own_beam_hits=True) >= MIN_HITS
    play(oracle_mod, [text, text.replace(". . . . .", ". . . . @")], 3, 30, 52, own_beam_hits=True)


@pytest.mark.parametrize("level", [1, 2])
def test_levels_without_sources(level):
    """No source, no laser tile, nobody to help: the tables are empty and every edge array stays zero on every step path, while the
    profiles still become valid and episodes still finish (levels 1 and 2 cannot be a rollout case: no state of theirs has an edge)."""
    import torch

    from lle_amd import BatchedLLE
    n = 64
    env = BatchedLLE(LEVELS[level], n, cooperation=True)
    env.reset()
    tr = env.cooperation
    g = torch.Generator().manual_seed(level)
    for t in range(40):
        avail = env.available_actions().cpu()
        acts = torch.multinomial(avail.reshape(-1, 5).float(), 1, generator=g).reshape(n, env.n_agents).to(torch.uint8)
        env.step(acts, auto_reset=True, **list(STEP_PATHS.values())[t % 4])
    env.reset(env_mask=torch.ones(n, dtype=torch.uint8))
    for edges in (tr.step_edges, tr.episode_edges, tr.last_edges):
        assert int(edges.abs().sum()) == 0
    assert tr.episode_profile.cpu().tolist() == [[0, 0, 0, 0, 0, 0, 0, 1]] * n and tr.last_profile.cpu().tolist() == [[0, 0, 0, 0, 0, 0, 0, 1]] * n
    assert tr.start_edges(0) == [] and not bool(tr.is_cooperative().any()) and bool(tr.is_independent(last=True).all())


# ---------------------------------------------------------------------------------------------- the reference's own worlds
@pytest.mark.parametrize("name", ["eight-agent-interdependent-8", "eight-agent-interdependent-8-perimeter"])
def test_eight_agent_kat_through_the_kernel(name):
    import torch

    from lle_amd import BatchedLLE
    env = BatchedLLE(WORLDS[name]["map"], 64, cooperation=True)
    env.reset()
    tr = env.cooperation
    want = torch.tensor(coop_ref.rows(RING8, 8), dtype=torch.int32).expand(64, 8)
    assert torch.equal(tr.step_edges.cpu(), want) and torch.equal(tr.episode_edges.cpu(), want)
    assert tr.episode_profile.cpu()[:, :5].tolist() == [[8, 8, 1, 1, 0]] * 64
    assert set(tr.edges(63, "step")) == RING8 and set(tr.start_edges(0)) == RING8
    assert bool(tr.is_cooperative().all()) and not bool(tr.is_asymmetric().any())
    assert not bool(tr.is_convergent(2).any()) and not bool(tr.is_divergent(2).any())
    for k in (-1, 0, 1):
        with pytest.raises(ValueError):
            tr.is_convergent(k)
        with pytest.raises(ValueError):
            tr.is_divergent(k)


@pytest.mark.parametrize("case", CASES["worlds"], ids=[c["name"] for c in CASES["worlds"]])
def test_single_world_kat(case):
    """detect_dependencies / profile_plan over lle_amd.World, one environment on the GPU."""
    from lle_amd import Action, World
    from lle_amd.characterization import TemporalCooperationGraph, detect_dependencies, profile_plan
    world = World(case["map"])
    if "edges_t0" in case["expect"]:
        assert detect_dependencies(world) == {tuple(e) for e in case["expect"]["edges_t0"]}
    plan = [[Action(a) for a in joint] for joint in case["plan"]]
    prof = profile_plan(world, plan)
    coop_ref.check_graph(prof.graph, case["expect"])
    again = TemporalCooperationGraph.from_plan([], world, reset=False)  # continues from the final state
    assert {(e.helper, e.beneficiary) for e in again.edges} == detect_dependencies(world)


def test_single_world_follows_its_sources():
    """LaserSource.disable / set_colour on a lle_amd.World reach the tracker's tables (lle_coop_update_map)."""
    from lle_amd import World
    from lle_amd.characterization import detect_dependencies
    world = World(line_map(3))
    assert detect_dependencies(world) == {(0, 1), (0, 2)}
    world.laser_sources[0].disable()
    assert detect_dependencies(world) == set()
    world.laser_sources[0].enable()
    assert detect_dependencies(world) == {(0, 1), (0, 2)}


def test_refused_step_counts_one_more_state():
    """A step that World.step refuses (err != 0) leaves the state: the same edges are marked again, byte 5 alone changes."""
    import torch

    from lle_amd import BatchedLLE
    env = BatchedLLE(line_map(3), 8, cooperation=True)
    env.reset()
    before = tracker_arrays(env.cooperation)
    acts = torch.full((8, 3), 4, dtype=torch.uint8)
    acts[::2, 0] = 0  # NORTH out of the world: refused in every other environment
    out = env.step(acts)
    assert out["err"].cpu().tolist() == [1, 0] * 4
    after = tracker_arrays(env.cooperation)
    for k in (0, 1, 2, 4):
        assert torch.equal(before[k], after[k]), NAMES[k]
    want = before[3].clone()
    want[:, 5] += 1
    assert torch.equal(after[3], want)


def test_tracker_queries_are_the_profile_of_the_flattened_graph():
    """is_cooperative / is_asymmetric / is_convergent(k) / is_divergent(k), running and last episode, against PlanProfile of the graph
    class over the same flattened edges (time plays no part in these four), after a rollout with episode ends."""
    import torch

    from lle_amd import BatchedLLE
    from lle_amd.characterization import DependencyEdge, TemporalCooperationGraph
    n = 64
    env = BatchedLLE(line_map(7), n, cooperation=True)
    env.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(25):
        avail = env.available_actions().cpu()
        acts = torch.multinomial(avail.reshape(-1, 5).float(), 1, generator=g).reshape(n, 7).to(torch.uint8)
        env.step(acts, auto_reset=True)  # (an environment that is reset first may refuse actions drawn for its old state: it then stays)
    tr = env.cooperation
    seen = set()
    for last in (False, True):
        got = {"coop": tr.is_cooperative(last).cpu(), "indep": tr.is_independent(last).cpu(), "asym": tr.is_asymmetric(last).cpu()}
        for k in (2, 3, 6, 7):
            got[f"conv{k}"], got[f"div{k}"] = tr.is_convergent(k, last).cpu(), tr.is_divergent(k, last).cpu()
        for e in range(n):
            prof = TemporalCooperationGraph([DependencyEdge(h, b, 0) for h, b in tr.edges(e, "last" if last else "episode")]).profile()
            want = {"coop": prof.is_cooperative, "indep": prof.is_independent, "asym": prof.is_asymmetric}
            for k in (2, 3, 6, 7):
                want[f"conv{k}"], want[f"div{k}"] = prof.is_convergent(k), prof.is_divergent(k)
            for key, value in want.items():
                assert bool(got[key][e]) == bool(value), (last, e, key)
                seen.add((key, bool(value)))
    assert {("coop", True), ("asym", True), ("div2", True), ("div3", True), ("div7", False)} <= seen, sorted(seen)
    assert int(tr.last_profile[:, 7].sum()) > 0, "no episode ended"


def test_without_the_argument_nothing_changes():
    """A BatchedLLE built without cooperation= never loads the library (a fresh interpreter: this process has loaded it)."""
    import os
    import subprocess
    import sys
    code = ("import sys, torch\n"
            "from lle_amd import BatchedLLE\n"
            "import lle_amd\n"
            "env = lle_amd.level(6).build(64)\n"
            "env.reset()\n"
            "acts = torch.full((64, env.n_agents), 4, dtype=torch.uint8, device='cuda')\n"
            "for kw in ({}, dict(fused=True), dict(fused=False), dict(persistent=True)):\n"
            "    env.step(acts, auto_reset=True, **kw)\n"
            "assert env.cooperation is None\n"
            "assert 'lle_amd.cooperation' not in sys.modules\n"
            "assert 'liblle_coop' not in open('/proc/self/maps').read()\n"
            "tracked = lle_amd.level(6).build(64, cooperation=True)\n"
            "assert isinstance(tracked.cooperation, lle_amd.CooperationTracker)\n"
            "print('untouched')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=300)
    assert res.returncode == 0 and "untouched" in res.stdout, res.stdout + res.stderr


def test_every_compiled_kernel_is_launched():
    """Last in the module: the rollouts above drive every coop_kernel<G, LDS_TABLE> against the restatement (lanes per environment
    1 / 2 / 4 / 8 / 16 x cell table in LDS or in global memory); each must be named by lle_coop_debug_launched."""
    from lle_amd import cooperation
    missing = sorted(set(cooperation.compiled_kernels()) - set(cooperation.launched_kernels()))
    assert not missing, f"compiled but never launched: {missing}"
    assert len(cooperation.compiled_kernels()) == 10
