"""The restatement of the shortest-plan search over the oracle (tests/search_ref.py) against the reference's expectations
(tests/golden/kat_solver.json), without a GPU.  The GPU tests compare the kernels with this restatement, so it has to agree with the
reference first.

One search per layout and mode at the largest stated t_max; the smaller horizons follow from the shortest lengths it finds, because a
shortest plan of length L padded with all-STAY rows is a plan of every length >= L: solvable(t) = (L <= t),
independent(t) = solvable(t) and (L_no_cooperation <= t), cooperative(t) = solvable(t) and not independent(t)
(python/lle/characterization/world_characterization.py:47-58).

Left out, because replaying prefixes on the oracle takes too long for a test (20 s, longer than a minute, 14 s): the built-in levels 2,
3 and 4.  tests/test_gpu_solver.py checks them on the device.  No other layout is left out."""
import pytest

from tests import search_ref

CASES = search_ref.load_cases()
LEFT_OUT = {"level-2": "20 s on the oracle", "level-3": "does not finish within a minute on the oracle", "level-4": "14 s on the oracle"}
CATALOGUE = [c for c in CASES["catalogue"] if c["name"] not in LEFT_OUT]


def test_only_the_three_levels_are_left_out():
    assert len(CASES["catalogue"]) == 26 and len(CATALOGUE) == 23
    assert sorted(LEFT_OUT) == ["level-2", "level-3", "level-4"]


@pytest.mark.parametrize("case", CATALOGUE, ids=[c["name"] for c in CATALOGUE])
def test_catalogue_on_the_restatement(oracle_mod, case):
    text = search_ref.map_text(case)
    t_top = max(int(t) for t in case["expect"])
    standard = search_ref.search(text, t_top, "standard")
    independent = search_ref.search(text, t_top, "no-cooperation")
    for t, expect in case["expect"].items():
        solvable = standard.length is not None and standard.length <= int(t)
        is_independent = solvable and independent.length is not None and independent.length <= int(t)
        got = dict(solvable=solvable, cooperative=solvable and not is_independent, independent=is_independent)
        for key, want in expect.items():
            assert got[key] is want, (case["name"], t, key)
    for mode, res in (("standard", standard), ("no-cooperation", independent)):
        assert len(res.frontier) == len(res.expanded) + 1 and res.frontier[0] == 1
        if res.plan is not None:
            search_ref.check_plan(text, res.plan, mode, length=res.length)
    if standard.length is not None and independent.length is not None:
        assert independent.length >= standard.length


def test_solver_cases_on_the_restatement(oracle_mod):
    for case in CASES["solver"]["lengths"]:
        if case["call"] == "find_shortest" and case["t_min"] is None:
            assert search_ref.search(case["map"], case["t_max"]).length == case["length"]
        else:  # a requested length: the shortest plan is not longer
            t_max = 2 if case["t_max"] == "auto" else case["t_max"]
            assert search_ref.search(case["map"], t_max).length <= case["length"]
    for case in CASES["solver"]["solvable"]:
        assert (search_ref.search(case["map"], case["t_max"]).length is not None) is case["solvable"], case["name"]
    for case in CASES["solver"]["collect_gems"]:
        assert (search_ref.search(case["map"], case["t_max"]).length is not None) is case["solvable"]
        assert (search_ref.search(case["map"], case["t_max"], collect_gems=True).length is not None) is case["solvable_with_gems"]


def test_termination_maps(oracle_mod):
    """The three ways a search ends without a plan, and the rule that a level is always finished."""
    exhausted = search_ref.search("S0 S1 S2\n. . .\nL1E . .\nX X X", 30)
    assert exhausted.length is None and exhausted.n_states == 350 and len(exhausted.frontier) == 10 and exhausted.frontier[-1] == 0
    frozen = search_ref.search("S0 . S1 . X X", 12)  # an exit freezes the agent that reaches it
    assert frozen.length is None and frozen.frontier[-1] == 0
    horizon = search_ref.search("S0 . . X", 2)
    assert horizon.length is None and len(horizon.expanded) == 2 and horizon.frontier[-1] > 0
    solved = search_ref.search("S0 . . X", 5)
    assert solved.length == 3 and solved.plan == [[2], [2], [2]] and solved.frontier == [1, 1, 1, 1] and solved.expanded == [2, 3, 3]
    gems = "S0 . G .\n.  . . .\nX  . . G"
    assert search_ref.search(gems, 12).length == 2 and search_ref.search(gems, 12, collect_gems=True).length == 8
    with pytest.raises(AssertionError):
        search_ref.check_plan("S0 . . X", [[2], [2]])
