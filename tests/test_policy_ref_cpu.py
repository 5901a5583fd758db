"""The restatement of the steps-to-go table over the oracle (tests/policy_ref.py) pinned to figures computed independently on the CPU:
states, levels, completeness, the root's steps, how many states are exact / without a plan / beyond the horizon, and the largest exact
value.  tests/test_gpu_policy.py compares liblle_policy.so with the same tables, state by state."""
import pytest

from tests import policy_ref

ROWS = {r[0]: r for r in policy_ref.rows()}
# name: (states, levels, complete, root, (exact, no plan, beyond the horizon), largest exact value)
FIGURES = {
    "line": (4, 4, True, 3, (4, 0, 0), 3),
    "single-laser-asymmetric": (16, 4, True, 2, (12, 4, 0), 4),
    "one-way-detour": (678, 9, True, 6, (678, 0, 0), 14),
    "one-way-detour-h7": (674, 7, False, 6, (43, 82, 549), 6),
    "termination-exhausted": (350, 9, True, None, (0, 350, 0), None),
    "exit-freezes": (10, 4, True, None, (0, 10, 0), None),
    "five-lanes": (243, 3, True, 2, (243, 0, 0), 2),
    "long-beam": (69, 8, False, 7, (35, 14, 20), 7),
    "gems-collect": (44, 11, True, 8, (41, 3, 0), 9),
    "gems": (12, 6, True, 2, (12, 0, 0), 5),
    "open-two-agent": (72, 5, True, 2, (72, 0, 0), 4),
}


def test_every_row_has_figures():
    assert set(ROWS) == set(FIGURES)


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_figures(name):
    _, text, horizon, collect_gems = ROWS[name]
    states, levels, complete, root, kinds, largest = FIGURES[name]
    t = policy_ref.build(text, horizon, collect_gems)
    exact = [t.answer(s)[0] for s in t.states if t.answer(s)[0] >= 0]
    print(name, t.n_states, t.depth_reached, t.complete, t.root_steps, t.kinds(), max(exact, default=None), t.frontier, t.expanded)
    assert (t.n_states, t.depth_reached, t.complete, t.root_steps, t.kinds(), max(exact, default=None)) == (states, levels, complete, root, kinds, largest)
    assert sum(t.frontier) == t.n_states and len(t.frontier) == t.depth_reached + 1 and (t.frontier[-1] == 0) is complete
    answers = [t.answer(s)[0] for s in t.states]
    if complete:  # no state of a complete table reads UNKNOWN; the ones without a plan are dead ends
        assert policy_ref.UNKNOWN not in answers and answers.count(policy_ref.DEAD_END) == kinds[1]
    else:         # ... and no state of a table cut at the horizon reads DEAD_END
        assert policy_ref.DEAD_END not in answers and answers.count(policy_ref.UNKNOWN) == kinds[1] + kinds[2]
    assert len(t.table) == t.n_states and all(v[2] <= t.depth_reached for v in t.table.values())


@pytest.mark.parametrize("name", sorted(FIGURES))
def test_values_are_consistent(name):
    """A goal state reads 0 with the all-STAY code; every other exact answer is one more than the answer of the successor its action
    leads to; the all-STAY action of an expanded state leads back to it (which the GPU tests rely on when they pad replayed prefixes)."""
    _, text, horizon, collect_gems = ROWS[name]
    t = policy_ref.build(text, horizon, collect_gems)
    stay = policy_ref.code_of([policy_ref.STAY] * t.n_agents)
    for i, s in enumerate(t.states):
        steps, code = t.answer(s)
        if s.depth < t.depth_reached:
            assert (stay, i) in s.edges
        if s.goal:
            assert (s.steps, s.code) == (0, stay)
        elif steps >= 0:
            successor = t.states[dict(s.edges)[code]]
            assert successor.steps == steps - 1 and t.answer(successor)[0] == steps - 1
            assert all(t.states[j].steps is None or (t.states[j].steps + 1, c) >= (steps, code) for c, j in s.edges)
        else:
            assert code == stay
