"""Hand transcription of the reference's cooperation tests as data; running it rewrites kat_coop.json.

Graph cases restate python/tests/characterization/test_plan.py and python/tests/test_temporal_dependency_graph.py: the temporal edges
a test builds ([helper, beneficiary, t]) and what it asserts.  World cases restate the tests that replay a world: the map text, the
plan and the asserted edges / properties.  Nothing here imports or executes the reference; only inputs and expected outputs are kept.
README_coop.md (next to this file) lists the reference tests that are left out, and why.

Keys of `expect` (each optional): is_independent, is_cooperative, is_asymmetric, is_mutual (booleans); sequential, interdependent,
convergent, divergent ({argument: boolean}); longest_trail, n_edges, max_helpers, max_beneficiaries (integers); flattened,
asymmetric_edges ([[helper, beneficiary]]); is_empty; edges ([[helper, beneficiary, t]], the graph's whole edge set);
value_error ({"sequential" | "convergent" | "divergent": [arguments that raise ValueError]}).
"""
import json
import os

PLAN = "python/tests/characterization/test_plan.py"
GRAPH = "python/tests/test_temporal_dependency_graph.py"
LAYOUTS = "python/tests/world_layouts.py"

RING4 = [[0, 1, 1], [1, 2, 2], [2, 3, 3], [3, 0, 4]]
LINE4 = [[0, 1, 1], [1, 2, 2], [2, 3, 3]]
BRANCH = [[0, 1, 1], [0, 2, 1], [0, 3, 1]]
CONVERGE = [[1, 0, 1], [2, 0, 1], [3, 0, 1]]
CYCLE3 = [[0, 1, 1], [1, 2, 2], [2, 0, 3]]
STATIC2 = [[0, 1, 1], [1, 0, 1]]

GRAPHS = [
    dict(name="profile_empty_graph", ref=f"{PLAN}:10-18", edges=[],
         expect=dict(is_independent=True, is_cooperative=False, interdependent={"2": False}, sequential={"2": False}, is_asymmetric=False)),
    dict(name="profile_single_edge", ref=f"{PLAN}:21-29", edges=[[0, 1, 16]],
         expect=dict(is_independent=False, is_cooperative=True, interdependent={"2": False}, sequential={"2": False}, is_asymmetric=True)),
    dict(name="profile_joining_edges", ref=f"{PLAN}:32-44", edges=[[5, 6, 5], [6, 9, 18], [9, 52, 125], [4, 52, 17]],
         expect=dict(sequential={"2": True, "3": True, "4": False})),
    dict(name="profile_separating_edges", ref=f"{PLAN}:47-74", edges=[[0, 1, 1], [1, 3, 2], [3, 6, 3], [1, 5, 25], [5, 2, 26], [2, 9, 50]],
         expect=dict(is_cooperative=True, is_asymmetric=True, sequential={"2": True, "3": True, "4": True, "5": False},
                     interdependent={"2": False}, is_mutual=False)),
    dict(name="profile_two_mutual", ref=f"{PLAN}:77-91", edges=STATIC2,
         expect=dict(is_cooperative=True, is_independent=False, interdependent={"2": True, "3": False}, sequential={"2": True, "3": False},
                     is_mutual=True)),
    dict(name="profile_length5_sequence", ref=f"{PLAN}:94-112", edges=[[19, 17, 125], [0, 1, 0], [17, 8, 126], [15, 19, 19], [1, 15, 14]],
         expect=dict(is_mutual=False, is_cooperative=True, is_independent=False,
                     sequential={"2": True, "3": True, "4": True, "5": True, "6": False},
                     interdependent={"2": False, "3": False, "4": False, "5": False})),
    dict(name="simultaneous_mutual_help_is_bounded_sequence", ref=f"{PLAN}:115-126", edges=STATIC2,
         expect=dict(sequential={"2": True}, is_cooperative=True, is_independent=False, interdependent={"2": True})),
    dict(name="rejects_mutual_as_asymmetric", ref=f"{PLAN}:129-138", edges=[[0, 1, 1], [1, 0, 2]], expect=dict(is_asymmetric=False, is_mutual=True)),
    dict(name="exact_interdependence_distinct_from_threshold", ref=f"{PLAN}:165-176", edges=RING4,
         expect=dict(interdependent={"3": False, "4": True, "5": False})),
    dict(name="convergence_counts_repeated_helper_once", ref=f"{PLAN}:214-223", edges=[[0, 2, 1], [0, 2, 3], [0, 2, 4]], expect=dict(convergent={"2": False})),
    dict(name="convergence_distinct_helpers_at_different_times", ref=f"{PLAN}:226-234", edges=[[0, 2, 1], [1, 2, 7]], expect=dict(convergent={"2": True})),
    dict(name="convergence_does_not_combine_beneficiaries", ref=f"{PLAN}:237-245", edges=[[0, 1, 1], [1, 2, 2]], expect=dict(convergent={"2": False})),
    dict(name="convergence_threshold_is_monotone", ref=f"{PLAN}:248-260", edges=[[0, 3, 1], [1, 3, 4], [2, 3, 9]],
         expect=dict(convergent={"2": True, "3": True, "4": False})),
    dict(name="convergence_ignores_duplicate_and_unrelated", ref=f"{PLAN}:263-277", edges=[[0, 3, 1], [0, 3, 1], [0, 3, 5], [1, 3, 7], [4, 5, 2], [5, 4, 3]],
         expect=dict(max_helpers=2, convergent={"2": True, "3": False})),
    dict(name="rejects_thresholds_below_two", ref=f"{PLAN}:280-289,406-409", edges=[],
         expect=dict(value_error=dict(sequential=[-1, 0, 1], convergent=[-1, 0, 1], divergent=[-1, 0, 1]))),
    dict(name="divergence_counts_repeated_beneficiary_once", ref=f"{PLAN}:292-305", edges=[[0, 2, 1], [0, 2, 3], [0, 2, 4]],
         expect=dict(max_beneficiaries=1, divergent={"2": False})),
    dict(name="divergence_without_convergence", ref=f"{PLAN}:308-320", edges=[[0, 1, 1], [0, 2, 7]], expect=dict(divergent={"2": True}, convergent={"2": False})),
    dict(name="divergence_accepts_simultaneous_help", ref=f"{PLAN}:323-334", edges=[[0, 1, 3], [0, 2, 3]], expect=dict(divergent={"2": True})),
    dict(name="convergence_without_divergence", ref=f"{PLAN}:337-349", edges=[[0, 2, 1], [1, 2, 7]], expect=dict(convergent={"2": True}, divergent={"2": False})),
    dict(name="divergence_threshold_is_monotone", ref=f"{PLAN}:352-366", edges=[[0, 1, 1], [0, 2, 4], [0, 3, 9]],
         expect=dict(divergent={"2": True, "3": True, "4": False})),
    dict(name="divergence_ignores_duplicate_and_unrelated", ref=f"{PLAN}:369-383", edges=[[0, 1, 1], [0, 1, 1], [0, 1, 5], [0, 2, 7], [4, 5, 2], [5, 4, 3]],
         expect=dict(max_beneficiaries=2, divergent={"2": True, "3": False})),
    dict(name="empty_graph_is_not_divergent", ref=f"{PLAN}:386-389", edges=[], expect=dict(max_beneficiaries=0, divergent={"2": False})),
    dict(name="self_loops_do_not_contribute", ref=f"{PLAN}:392-403", edges=[[0, 0, 1], [0, 1, 2]],
         expect=dict(max_beneficiaries=1, max_helpers=1, divergent={"2": False}, convergent={"2": False}, flattened=[[0, 1]])),
    # ---- python/tests/test_temporal_dependency_graph.py
    dict(name="non_empty_graph_not_independent", ref=f"{GRAPH}:118-120", edges=[[0, 1, 2]], expect=dict(is_independent=False)),
    dict(name="flattened_edges_collapses_time", ref=f"{GRAPH}:126-130", edges=[[0, 1, 1], [0, 1, 3], [0, 1, 5]], expect=dict(flattened=[[0, 1]])),
    dict(name="flattened_edges_all_edges", ref=f"{GRAPH}:132-138", edges=BRANCH, expect=dict(flattened=[[0, 1], [0, 2], [0, 3]])),
    dict(name="trail_strictly_increasing_times", ref=f"{GRAPH}:144-152", edges=LINE4, expect=dict(longest_trail=3)),
    dict(name="trail_same_time_two_edges", ref=f"{GRAPH}:154-161", edges=[[0, 1, 1], [1, 2, 1]], expect=dict(longest_trail=2)),
    dict(name="trail_same_time", ref=f"{GRAPH}:163-171,200-211", edges=[[0, 1, 1], [1, 2, 1], [2, 3, 1]], expect=dict(longest_trail=3)),
    dict(name="trail_decreasing_times", ref=f"{GRAPH}:173-182", edges=[[0, 1, 3], [1, 2, 2], [2, 3, 1]], expect=dict(longest_trail=1)),
    dict(name="trail_non_monotonic_times", ref=f"{GRAPH}:184-198", edges=[[0, 1, 0], [1, 2, 2], [2, 3, 1]], expect=dict(longest_trail=2)),
    dict(name="trail_mixed_times", ref=f"{GRAPH}:213-224", edges=[[0, 1, 1], [1, 2, 2], [0, 3, 1], [3, 4, 3]], expect=dict(longest_trail=2)),
    dict(name="trail_hamiltonian_cycle", ref=f"{GRAPH}:226-231", edges=RING4, expect=dict(longest_trail=4)),
    dict(name="trail_may_revisit_agents", ref=f"{GRAPH}:233-241", edges=[[0, 1, 1], [1, 0, 2], [0, 2, 3]], expect=dict(longest_trail=3)),
    dict(name="trail_may_not_revisit_same_edge", ref=f"{GRAPH}:243-251", edges=[[0, 1, 1], [1, 0, 1], [1, 2, 3]], expect=dict(longest_trail=3)),
    dict(name="three_agents_is_trail_of_length_2", ref=f"{GRAPH}:253-260", edges=[[0, 1, 1], [1, 2, 2]], expect=dict(longest_trail=2)),
    dict(name="cycle_three_agents_returns_3", ref=f"{GRAPH}:262-272", edges=CYCLE3, expect=dict(longest_trail=3, interdependent={"3": True})),
    dict(name="cycle_same_time_three_agents_returns_3", ref=f"{GRAPH}:274-285", edges=[[0, 1, 1], [1, 2, 1], [2, 0, 3]],
         expect=dict(longest_trail=3, interdependent={"3": True, "4": False})),
    dict(name="branching_trail", ref=f"{GRAPH}:297-304", edges=[[0, 1, 1], [0, 2, 2]], expect=dict(longest_trail=1)),
    dict(name="mutual_help_is_sequence", ref=f"{GRAPH}:306-313", edges=[[0, 1, 1], [1, 0, 2]], expect=dict(longest_trail=2)),
    dict(name="simultaneous_mutual_help_trail", ref=f"{GRAPH}:315-322", edges=STATIC2, expect=dict(longest_trail=2)),
    dict(name="independent_graph_trail", ref=f"{GRAPH}:324-327", edges=[], expect=dict(longest_trail=0)),
    dict(name="cycle_branching", ref=f"{GRAPH}:333-335", edges=BRANCH, expect=dict(interdependent={"2": False})),
    dict(name="temporal_cycle_detected", ref=f"{GRAPH}:337-342", edges=CYCLE3, expect=dict(interdependent={"2": False, "3": True, "4": False})),
    dict(name="static_cycle_is_detected", ref=f"{GRAPH}:344-347", edges=STATIC2, expect=dict(interdependent={"2": True})),
    dict(name="cycle_disconnected", ref=f"{GRAPH}:349-351", edges=[[0, 1, 1], [2, 3, 2]], expect=dict(interdependent={"2": False})),
    dict(name="cycle_in_scc", ref=f"{GRAPH}:353-357", edges=[[0, 1, 1], [1, 0, 2], [1, 2, 3], [2, 1, 4], [0, 2, 5], [2, 0, 6]],
         expect=dict(interdependent={"3": True})),
    dict(name="self_loop_is_ignored", ref=f"{GRAPH}:363-368", edges=[[0, 0, 1]], expect=dict(flattened=[], is_empty=True)),
    dict(name="duplicate_edges_collapsed", ref=f"{GRAPH}:370-379", edges=[[0, 1, 1], [0, 1, 1], [0, 1, 1]], expect=dict(n_edges=1)),
    dict(name="negative_time_steps", ref=f"{GRAPH}:388-392", edges=[[0, 1, -5]], expect=dict(edges=[[0, 1, -5]])),
    dict(name="sequential_help_sequence", ref=f"{GRAPH}:398-408", edges=LINE4, expect=dict(longest_trail=3, interdependent={"2": False})),
    dict(name="bottleneck_pattern", ref=f"{GRAPH}:410-419", edges=[[0, 1, 1], [0, 2, 1], [0, 3, 1], [0, 4, 1]], expect=dict(longest_trail=1)),
    dict(name="diamond_pattern", ref=f"{GRAPH}:421-433", edges=[[0, 1, 1], [0, 2, 1], [1, 3, 2], [2, 3, 2]],
         expect=dict(longest_trail=2, interdependent={"2": False, "3": False}, is_asymmetric=True)),
    dict(name="has_asymmetric_edge_single", ref=f"{GRAPH}:436-439", edges=[[0, 1, 1]], expect=dict(is_asymmetric=True)),
    dict(name="has_asymmetric_edge_chain", ref=f"{GRAPH}:441-446", edges=[[0, 1, 1], [2, 0, 1]], expect=dict(is_asymmetric=True)),
    dict(name="asymmetric_edges", ref=f"{GRAPH}:449-451", edges=[[0, 1, 2], [1, 2, 3]], expect=dict(asymmetric_edges=[[0, 1]])),
    dict(name="closed_trail_bowtie", ref=f"{GRAPH}:454-476", edges=[[0, 1, 1], [1, 0, 2], [0, 2, 3], [2, 0, 4]], expect=dict(interdependent={"3": True})),
    dict(name="closed_trail_double_petal", ref=f"{GRAPH}:464-478", edges=[[0, 1, 1], [1, 2, 2], [2, 0, 3], [0, 1, 4], [1, 3, 5], [3, 0, 6]],
         expect=dict(interdependent={"4": True})),
    dict(name="exact_order_4_without_order_3", ref=f"{GRAPH}:481-495", edges=RING4, expect=dict(interdependent={"4": True, "3": False})),
    dict(name="max_distinct_beneficiaries_groups_per_helper", ref=f"{GRAPH}:498-504", edges=BRANCH, expect=dict(max_beneficiaries=3, max_helpers=1)),
    dict(name="max_distinct_helpers_dual", ref=f"{GRAPH}:507-513", edges=CONVERGE, expect=dict(max_helpers=3, max_beneficiaries=1)),
    dict(name="max_distinct_beneficiaries_collapses_time", ref=f"{GRAPH}:516-530", edges=[[0, 1, 1], [0, 1, 1], [0, 1, 6], [0, 2, 6], [3, 4, 2]],
         expect=dict(max_beneficiaries=2)),
    dict(name="degree_metrics_ignore_self_loops", ref=f"{GRAPH}:533-537", edges=[[0, 0, 1], [0, 1, 2]], expect=dict(max_beneficiaries=1, max_helpers=1)),
    dict(name="degree_metrics_of_the_empty_graph", ref=f"{GRAPH}:540-547", edges=[], expect=dict(max_beneficiaries=0, max_helpers=0)),
]

EIGHT = """
  .   .  .   .   .  .   .   . L1S  .
 L0E S0  X   .   .  .   .   . S1   .
  .   .  .  L5S  .  .   .   .  X   .
  .   .  .  S5   .  X  S4  L4W .   .
  .   .  .   X   .  .   .   .  .   .
  .   X  .   .   .  .   X   .  .   .
  X  S7  X  S6  L6W .  S3   X S2  L2W
  .  L7N .   .   .  .  L3N  .  .   .
"""

EIGHT_PERIMETER = """
 .   .   . . .   L1S .   . .   .   .
L0E  S0  X . .   S1  .   . .   .   .
 .   .   . . .   X   .   . .   .   .
 .   .   . . .   .   .   . .   L3S .
 .   .   . . L2E S2  X   . .   S3  .
 .   X   . . .   @   .   . .   X   .
 .   S7  . . X   S6  L6W . .   .   .
 .   L7N . . .   X   .   . .   .   .
 .   .   . . .   S5  .   . X   S4  L4W
 .   .   . . .   L5N .   . .   .   .
"""

ASYMMETRIC_CORRIDOR = """
 @  S0 S1 @ @ @
L0E .  .  . . .
 @  @  @  @ @ .
 @  @  @  @ X .
 @  @  @  @ @ X
"""

RING8 = [[h, (h + 1) % 8] for h in range(8)]
N, S, E, W, STAY = 0, 1, 2, 3, 4

WORLDS = [
    dict(name="eight-agent-interdependent-8", ref=f"{PLAN}:179-189; {LAYOUTS}:787-802", map=EIGHT, plan=[],
         expect=dict(edges=[[h, b, 0] for h, b in RING8], edges_t0=RING8,
                     interdependent={"2": False, "3": False, "4": False, "5": False, "6": False, "7": False, "8": True, "9": False})),
    dict(name="eight-agent-interdependent-8-perimeter", ref=f"{LAYOUTS}:804-825", map=EIGHT_PERIMETER, plan=[],
         note="the expected edges are the layout's description (the exact cycle 0 -> 1 -> ... -> 7 -> 0 at t = 0) and its expectation "
              "interdependent={7: False, 8: True, 9: False}",
         expect=dict(edges=[[h, b, 0] for h, b in RING8], edges_t0=RING8, interdependent={"7": False, "8": True, "9": False})),
    dict(name="multiple_steps_in_a_row_remains_asymmetric", ref=f"{PLAN}:192-214", map=ASYMMETRIC_CORRIDOR,
         note="the reference obtains its plan from lle.solve(world, 16); this 12-step plan is written by hand: agent 0 steps onto its beam and "
              "waits while agent 1 walks along it and leaves, then follows",
         plan=[[S, S], [STAY, E], [STAY, E], [STAY, E], [STAY, S], [E, S], [E, S], [E, STAY], [E, STAY], [S, STAY], [S, STAY], [W, STAY]],
         expect=dict(is_asymmetric=True, is_cooperative=True, is_independent=False, sequential={"2": False}, interdependent={"2": False, "3": False})),
]


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_coop.json")
    with open(out, "w") as f:
        json.dump(dict(graphs=GRAPHS, worlds=WORLDS), f, indent=1)
        f.write("\n")
    print(f"{len(GRAPHS)} graph cases and {len(WORLDS)} world cases -> {out}")
