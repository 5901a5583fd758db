"""The facts tests/test_gpu_search_edges.py rests on, from the restatements over the oracle alone, without a GPU: the six-agent
searches and tables, the pools that overflow and fit, the exact state counts, the rebuilt tables and the seeds of the lived-in batches
(tests/search_edges_inputs.py names the inputs)."""
import numpy as np

from tests import forest_ref, helpgraph_ref, policy_ref, search_ref
from tests import search_edges_inputs as inp

U, D = policy_ref.UNKNOWN, policy_ref.DEAD_END


def test_six_agent_searches(oracle_mod):
    std = search_ref.search(inp.SIX, 4)
    assert (std.length, std.frontier, std.expanded) == (2, [1, 47, 436], [64, 3561])
    search_ref.check_plan(inp.SIX, std.plan, length=2)
    assert any(row[4] != 4 for row in std.plan) and any(row[5] != 4 for row in std.plan), "agents 4 and 5 have to walk"
    alone = search_ref.search(inp.SIX, 4, "no-cooperation")
    assert (alone.length, alone.frontier, alone.expanded) == (None, [1, 31, 276, 332, 200], [64, 2256, 12814, 8890])
    lanes = search_ref.search(inp.LANES6, 4)
    assert (lanes.length, lanes.frontier, lanes.expanded) == (1, [1, 63], [64])
    w = oracle_mod.OracleWorld(inp.SIX)
    assert w.n_agents == 6 == oracle_mod.OracleWorld(inp.LANES6).n_agents


def test_six_agent_forest_inputs(oracle_mod):
    """Two maps of one shape with different answers; level 1 of both is 47 states x 15 625 codes: 45 pieces of 16 384."""
    a, b = oracle_mod.OracleWorld(inp.SIX), oracle_mod.OracleWorld(inp.SIX_VARIANT)
    assert (a.height, a.width, a.n_agents, a.n_sources, a.n_gems) == (b.height, b.width, b.n_agents, b.n_sources, b.n_gems)
    assert sorted(a.exit_pos) != sorted(b.exit_pos) and len(a.exit_pos) == len(b.exit_pos) == 6
    refs = {m: forest_ref.oracle([inp.SIX, inp.SIX_VARIANT], 2, m) for m in forest_ref.MODES}
    assert [(r.length, r.frontier, r.expanded) for r in refs["standard"]] == [(2, [1, 47, 436], [64, 3561]), (None, [1, 47, 304], [64, 2691])]
    assert [(r.length, r.frontier, r.expanded) for r in refs["no-cooperation"]] == [(None, [1, 31, 276], [64, 2256]), (None, [1, 31, 276], [64, 2256])]
    assert -(-47 * 5 ** 6 // 16384) == 45


def test_six_agent_tables(oracle_mod):
    t = policy_ref.build(inp.SIX, 12, False)
    assert (t.n_states, t.complete, t.depth_reached, t.root_steps) == (2704, True, 11, 2)
    assert t.frontier == [1, 47, 436, 540, 320, 320, 288, 400, 256, 64, 32, 0]
    answers = [t.answer(s) for s in t.states]
    steps = np.array([a[0] for a in answers])
    assert {int(k): int((steps == k).sum()) for k in np.unique(steps)} == {D: 676, 0: 8, 1: 121, 2: 606, 3: 926, 4: 367}
    digits = np.array([policy_ref.joint_of(a[1], 6) for a in answers])
    assert (digits[:, 4] != policy_ref.STAY).any() and (digits[:, 5] != policy_ref.STAY).any(), "the codes use the two highest digits"
    assert max(a[1] for a in answers) < 5 ** 6 <= 0xFFFF and policy_ref.code_of([policy_ref.STAY] * 6) == 15624
    cut = policy_ref.build(inp.SIX, 4, False)
    assert (cut.n_states, cut.complete, cut.depth_reached, cut.root_steps) == (1344, False, 4, 2)
    exact, no_plan, beyond = cut.kinds()
    assert exact > 0 and no_plan + beyond > 0 and exact + no_plan + beyond == 1344


def test_pools_that_overflow_and_fit(oracle_mod):
    text, t_max = inp.text(inp.CAPACITY_MAP), inp.CAPACITY_T_MAX
    std, alone = search_ref.search(text, t_max), search_ref.search(text, t_max, "no-cooperation")
    assert (std.n_states, std.length, alone.n_states, alone.length) == (363, 5, 55, None)
    assert alone.n_states <= inp.SEARCH_POOL < std.n_states
    over = helpgraph_ref.search(text, t_max, *inp.HELPGRAPH_OVER)
    fits = helpgraph_ref.search(text, t_max, *inp.HELPGRAPH_FITS)
    assert (over.n_states, over.length, fits.n_states, fits.length) == (505, 5, 245, None)
    assert fits.n_states <= inp.HELPGRAPH_POOL < over.n_states


def test_exact_counts(oracle_mod):
    """About a dozen states each; the help-graph search stores 14 records where the plain one stores 11 states."""
    text = inp.text(inp.EXACT_MAP)
    assert search_ref.search(text, inp.EXACT_T_MAX).n_states == 11 and search_ref.search(text, inp.EXACT_T_MAX).length == 2
    assert search_ref.search(text, inp.EXACT_T_MAX, "no-cooperation").n_states == 10
    assert helpgraph_ref.search(text, inp.EXACT_T_MAX).n_states == 14
    recorded = next(s for s in inp.HG_CASES["searches"] if s["map"] == inp.EXACT_MAP and s["mode"] == "standard")
    assert (recorded["t_max"], recorded["states"]) == (inp.EXACT_T_MAX, 14)
    t = policy_ref.build(text, inp.EXACT_HORIZON, False)
    assert (t.n_states, t.complete, t.root_steps) == (16, True, 2)


def test_rebuilt_tables(oracle_mod):
    """The five configurations of the rebuilt handle differ in size, completeness and identity."""
    tables = [policy_ref.build(inp.GEMS, h, c) for h, c in inp.REBUILDS]
    assert [(t.n_states, t.complete, t.root_steps) for t in tables] == [(12, True, 2), (12, True, 2), (44, True, 8), (11, False, None), (12, True, 2)]
    cut = tables[3]
    assert cut.kinds()[0] == 0 and all(cut.answer(s)[0] == U for s in cut.states)
    # the states of the largest table, looked up in every configuration: some are not in the cut table at all
    batch = tables[2]
    assert sum((s.key not in cut.table) for s in batch.states) > 0
    assert len({s.key[:-1] for s in batch.states}) == 12


def test_lived_in_batches(oracle_mod):
    """The seed leaves solved, reset and dead environments visible, and ragged last workgroups (1 000 = 3 x 256 + 232)."""
    assert sum(inp.ROLLOUT_CHUNKS) == inp.LIVED_STEPS and inp.LIVED_ENVS % 256 != 0
    for name, horizon in inp.LIVED.items():
        lived = inp.lived_in(inp.text(name), horizon)
        want = np.stack(lived.want)
        assert want.shape == (inp.LIVED_STEPS, inp.LIVED_ENVS)
        assert (want == 0).any() and (want == D).any() and (want > 0).any() and not (want == U).any(), name
        assert np.stack(lived.was_reset).any(), name
        ends = np.cumsum(inp.ROLLOUT_CHUNKS) - 1  # the steps a chunked rollout() shows
        assert (want[ends] == 0).any() and (want[ends] == D).any(), name
        # an environment reset at the start of a step has taken one joint action since: those that took all-STAY are at the reset state
        stayed = [w[r & (a == policy_ref.STAY).all(1)] for w, r, a in zip(lived.want, lived.was_reset, lived.actions)]
        stayed = np.concatenate(stayed)
        assert stayed.size > 0 and (stayed == lived.root_steps).all(), name


def test_padded_and_gem_inputs(oracle_mod):
    text = inp.text(inp.PADDED_MAP)
    t = policy_ref.build(text, inp.PADDED_HORIZON, False)
    assert (t.n_agents, t.n_states, t.complete, t.root_steps) == (3, 506, True, 9)
    lived = inp.lived_in(text, inp.PADDED_HORIZON, False, inp.PADDED_STEPS)
    last = lived.want[-1]
    assert (last >= 0).any() and (last == D).any()
    # gems: flipping the gem word changes an answer of the collect_gems table and never one of the plain table
    with_gems = policy_ref.build(inp.GEMS, 12, True)
    lived = inp.lived_in(inp.GEMS, 12, True, inp.PADDED_STEPS)
    table, changed, unknown = with_gems.table, 0, 0
    for e, key in enumerate(lived.keys):
        word = inp.gem_word(lived.gems[-1][e])
        assert inp.answer_with_gems(table, key, word, 2) == lived.want[-1][e]
        flipped = inp.answer_with_gems(table, key, word ^ (1 + e % 3), 2)
        changed += flipped != lived.want[-1][e]
        unknown += flipped == U
        assert inp.answer_with_gems(table, key, word | 1 << 7, 2) == U
    assert changed > 0 and unknown > 0
