"""The forest of steps-to-go tables without a GPU: header / exports / binding of liblle_policyforest.so, where the library is registered,
the lazy name, every host-side refusal, PolicyForest's argument errors, the fixed input sets against the figures the issue states
(reproduced from tests/policy_ref.py), and the lane, level, pass and answer arithmetic of policyforest_logic.hpp with a host relaxation
of a three-map forest under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program
(tests/hostsim/policyforest_pieces.cpp).  The tables themselves are built on the MI355X (tests/test_gpu_policyforest.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, forest, policy, policyforest
from tests import policyforest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7


def handles(maps):
    return (C.c_void_p * len(maps))(*[m.h for m in maps])


def options(envs_per_map=0, max_states_per_map=0, struct_bytes=None, device=-1):
    return policyforest.PolicyForestOptions(C.sizeof(policyforest.PolicyForestOptions) if struct_bytes is None else struct_bytes, device, envs_per_map,
                                            max_states_per_map, None)


# ---------------------------------------------------------------------------------------------------------------- the library
def test_library_exports_sizes_and_constants():
    """liblle_policyforest.so exports every function include/lle_policyforest.h declares, and the binding knows exactly those; the
    header is plain C; struct sizes and field offsets of the binding are the header's."""
    L = policyforest.lib()
    header = open(os.path.join(ROOT, "include", "lle_policyforest.h")).read()
    declared = set(re.findall(r"\b(lle_policyforest_[a-z_0-9]+)\s*\(", header))
    assert declared == set(policyforest.EXPORTS) and len(policyforest.EXPORTS) == 9
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "policyforest", "policyforest.hip")).read()
    for include in ("../../include/lle_policyforest.h", "../forest/forest_core.hpp", "../policy/policy_logic.hpp", "policyforest_logic.hpp"):
        assert f'#include "{include}"' in source
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    for foreign in ("lle_policy_create", "lle_policy_build", "lle_policy_lookup", "lle_forest_create", "lle_search_create"):
        assert foreign + "(" not in source  # of liblle_policy.so only the host-only fingerprint is called
    assert "__syncthreads" not in source and "__shared__" not in source  # a workgroup straddles maps: no staged table, no barrier
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "lle_policyforest.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d", '
            'sizeof(lle_policyforest_options), sizeof(lle_policyforest_result), sizeof(lle_policyforest_summary), sizeof(lle_policy_args), '
            'offsetof(lle_policyforest_options, stream), offsetof(lle_policyforest_result, n_states), offsetof(lle_policyforest_result, passes), '
            'offsetof(lle_policyforest_summary, explore_ms), offsetof(lle_policyforest_summary, relax_lanes), (int)LLE_POLICY_CAPACITY, (int)LLE_POLICY_UNKNOWN, '
            '(int)LLE_POLICY_DEAD_END); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    O, Rs, S = policyforest.PolicyForestOptions, policyforest.PolicyForestMapResult, policyforest.PolicyForestSummary
    assert got == [C.sizeof(O), C.sizeof(Rs), C.sizeof(S), C.sizeof(policy.PolicyArgs), O.stream.offset, Rs.n_states.offset, Rs.passes.offset, S.explore_ms.offset,
                   S.relax_lanes.offset, policyforest.LLE_POLICY_CAPACITY, policyforest.PolicyForest.UNKNOWN, policyforest.PolicyForest.DEAD_END]
    assert sorted(policyforest.compiled_kernels()) == sorted(policyforest.KERNELS) and len(policyforest.KERNELS) == 7
    assert policyforest.launched_kernels() == []
    assert "lle_policyforest.h" in open(os.path.join(ROOT, "include", "lle_policy.h")).read()  # the multi-map refusal points to the forest


def test_build_knows_the_library():
    from lle_amd import build
    text = open(build.__file__).read()
    assert '("policyforest", "liblle_policyforest.so", "liblle_policy.so")' in text  # built after the library it links against
    assert text.index('("policy", "liblle_policy.so")') < text.index('("policyforest", "liblle_policyforest.so"')
    needed = subprocess.run(["readelf", "-d", policyforest.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "liblle_policy.so" in needed and "liblle_hip.so" in needed and "$ORIGIN" in needed and "liblle_forest.so" not in needed
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "policyforest.EXPORTS" in entry and "liblle_policyforest.so does not export" in entry
    assert os.path.exists(policyforest.LIB_PATH)
    ignored = subprocess.run(["git", "check-ignore", "-q", policyforest.LIB_PATH], cwd=ROOT)
    assert ignored.returncode in (0, 128)  # ignored (128: not a git checkout)


def test_lazy_names():
    assert lle_amd.PolicyForest is policyforest.PolicyForest and "PolicyForest" in lle_amd.__all__
    assert lle_amd.OptimalPolicy is policy.OptimalPolicy  # the single-map policy keeps its name
    assert policyforest.PolicyForest.UNKNOWN == policy.OptimalPolicy.UNKNOWN and policyforest.PolicyForest.DEAD_END == policy.OptimalPolicy.DEAD_END


def test_host_side_refusals():
    L = policyforest.lib()
    line, other = Map(LINE), Map("S0 . X .")

    def refused(maps, n, opt, word):
        got = L.lle_policyforest_create(maps, n, None if opt is None else C.byref(opt))
        message = L.lle_policyforest_last_error()
        assert got is None and word in message, (word, message)

    two = handles([line, other])
    refused(None, 1, None, b"NULL maps")
    refused(two, 0, None, b"n_maps must be at least 1")
    refused((C.c_void_p * 2)(line.h, None), 2, None, b"NULL map (entry 1)")
    refused(two, 2, options(struct_bytes=4), b"lle_policyforest_options.struct_bytes")
    for E, cap, word in ((-1, 0, b"envs_per_map must be 1 .. 2^30"), ((1 << 30) + 1, 0, b"envs_per_map must be"), (0, -1, b"max_states_per_map must be 1 .. 2^30"),
                         (0, (1 << 30) + 1, b"max_states_per_map must be"), (1 << 30, 0, b"n_maps * envs_per_map")):
        refused(two, 2, options(E, cap), word)
    refused(handles([line]), 1, options(1 << 30, 1 << 30), b"below 2^31")  # a table segment of 2^32 slots
    refused(handles([line, Map("S0 . X")]), 2, None, b"lle_batch_create_multi: the maps of a batch must agree on height, width")
    refused(handles([Map(SEVEN)]), 1, None, b"more than 6 agents")
    # nothing wrong with the arguments: where they are refused all the same, what is missing is the device
    for maps, n, opt in ((two, 2, None), (handles([line]), 1, options(7, 128))):
        got = L.lle_policyforest_create(maps, n, None if opt is None else C.byref(opt))
        assert got is not None or b"no HIP device: the policy forest" in L.lle_policyforest_last_error(), L.lle_policyforest_last_error()
        L.lle_policyforest_free(got)
    # the arguments of a build are judged before the handle is looked at
    res = (policyforest.PolicyForestMapResult * 2)()

    def build_refused(word, horizon=3, struct_bytes=None, summary=None):
        args = policy.PolicyArgs(C.sizeof(policy.PolicyArgs) if struct_bytes is None else struct_bytes, 0, horizon, 0)
        assert L.lle_policyforest_build(None, C.byref(args), res, summary) < 0 and word in L.lle_policyforest_last_error(), (word, L.lle_policyforest_last_error())

    build_refused(b"lle_policy_args.struct_bytes", struct_bytes=8)
    build_refused(b"horizon must be 0 .. 32767", horizon=-1)
    build_refused(b"horizon must be 0 .. 32767", horizon=32768)
    build_refused(b"lle_policyforest_summary.struct_bytes", summary=C.byref(policyforest.PolicyForestSummary(8)))
    build_refused(b"NULL handle")
    args = policy.PolicyArgs(C.sizeof(policy.PolicyArgs), 0, 3, 0)
    assert L.lle_policyforest_build(None, C.byref(args), None, None) == -1 and b"NULL arguments or results" in L.lle_policyforest_last_error()
    assert L.lle_policyforest_stats(None, 0, None, None, 0) == -1
    assert L.lle_policyforest_fingerprints(None, None, 0) == -1
    assert L.lle_policyforest_lookup(None, None, -1, None, None, 0, None) == -1
    L.lle_policyforest_free(None)


def test_policy_forest_argument_errors():
    """Refusals that come before any device work."""
    with pytest.raises(ValueError, match="at least one world"):
        policyforest.PolicyForest([], 5)
    with pytest.raises(ValueError, match="horizon must be 0 .. 32767"):
        policyforest.PolicyForest([LINE], -1)
    with pytest.raises(ValueError, match="horizon must be 0 .. 32767"):
        policyforest.PolicyForest([LINE], 40000)
    with pytest.raises(ValueError, match="at least 1"):
        policyforest.PolicyForest([LINE], 5, envs_per_map=0)
    with pytest.raises(ValueError, match="at least 1"):
        policyforest.PolicyForest([LINE], 5, max_states_per_map=0)
    with pytest.raises(ValueError, match="at most 6 agents"):
        policyforest.PolicyForest([SEVEN], 4)
    with pytest.raises(ValueError, match="lle_batch_create_multi: the maps of a batch must agree on height, width"):  # the C message
        policyforest.PolicyForest([LINE, LINE, "S0 . X"], 5)
    with pytest.raises(ValueError, match="n_maps \\* envs_per_map must be at most 2\\^30"):
        policyforest.PolicyForest([LINE, LINE], 5, envs_per_map=1 << 30)
    assert policyforest.PolicyForest._horizon("auto", Map("S0 . . .\n. . . X")) == 4 and policyforest.PolicyForest._horizon(7, Map(LINE)) == 7


# ---------------------------------------------------------------------------------------------------------------- the fixed input sets
def test_sets_have_the_stated_shapes():
    shapes = {"A": (16, 4, 5, 2, 1, 1), "B": (16, 5, 5, 2, 2, 1), "C": (6, 4, 4, 3, 1, 0)}
    for name, (count, h, w, agents, sources, gems) in shapes.items():
        s = R.SETS[name]
        assert len(s.maps) == count and {forest.shape_key(Map(t)) for t in s.maps} == {forest.shape_key(Map(s.maps[0]))}, name
        m = Map(s.maps[0])
        assert (m.height, m.width, m.n_agents, m.n_sources, m.n_gems) == (h, w, agents, sources, gems), name
    assert 5 ** Map(R.SET_C.maps[0]).n_agents == 125


def test_set_a_has_the_stated_tables():
    whole, cut = R.tables("A", 40), R.tables("A", 6)
    assert all(t.complete for t in whole) and [t.n_states for t in whole] == R.A40_N_STATES
    assert min(t.depth_reached for t in whole) == 7 and max(t.depth_reached for t in whole) == 13
    kinds = [R.kinds(t) for t in whole]  # (exact, no plan, beyond the horizon, dead end)
    assert [m for m, k in enumerate(kinds) if k[0] == 0 and k[3] == whole[m].n_states] == R.A40_UNSOLVABLE == [8, 13]  # complete and unsolvable
    assert sum(1 for k in kinds if k[0] > 0 and k[3] > 0) == 9 and all(k[1] == k[2] == 0 for k in kinds)  # exact answers beside dead ends
    assert not any(t.complete for t in cut) and [t.n_states for t in cut] == R.A6_N_STATES and all(t.depth_reached == 6 for t in cut)
    kinds = [R.kinds(t) for t in cut]
    assert sum(1 for k in kinds if k[0] > 0 and k[1] > 0 and k[2] > 0) == 12 and all(k[3] == 0 for k in kinds)  # exact, no plan and beyond the horizon at once
    assert [m for m, k in enumerate(kinds) if k[1] == cut[m].n_states] == R.A6_NO_PLAN == [5, 7, 8, 13]  # UNKNOWN throughout
    assert [t.root_steps for t in cut] == R.A6_ROOTS and [R.root_answer(t) for t in cut] == [R.UNKNOWN if r is None else r for r in R.A6_ROOTS]
    assert max(t.n_states for t in whole) == 211 and [t.n_states for t in whole].index(211) == 5 and sorted(t.n_states for t in whole)[-2] == 210
    assert [m for m, t in enumerate(whole) if t.n_states <= 128] == [1, 8, 13, 14]  # what fits a pool of 128
    gems = R.tables("A", 6, True)  # one gem per map: with collect_gems another table
    assert [t.n_states for t in gems] != R.A6_N_STATES and all(len(t.states[0].gems) == 1 for t in gems)


def test_sets_b_and_c_have_the_stated_tables():
    cut, whole = R.tables("B", 6), R.tables("B", 40)
    assert {m: (t.n_states, t.depth_reached) for m, t in enumerate(cut) if t.complete} == R.B6_COMPLETE == {1: (46, 6), 13: (24, 5)}  # finished inside a running lock-step
    assert max(t.n_states for t in cut) == 252 and sum(not t.complete for t in cut) == 14
    assert all(t.complete for t in whole) and max(t.n_states for t in whole) == 280
    assert min(t.depth_reached for t in whole) == 5 and max(t.depth_reached for t in whole) == 14
    assert [m for m, t in enumerate(whole) if R.kinds(t)[3] == t.n_states] == R.B40_UNSOLVABLE == [5, 8, 14]
    whole, cut = R.tables("C", 40), R.tables("C", 6)
    assert [t.n_states for t in whole] == R.C40_N_STATES and max(t.depth_reached for t in whole) == 19 and all(t.complete for t in whole)
    assert [t.n_states for t in cut] == R.C6_N_STATES and [t.complete for t in cut] == [False, True, False, False, False, False]


def test_layout_of_a_multi_map_batch():
    """`expected` and `replay_rows`: state k of map m in environment m * E_c + k, the reset state in the spare ones."""
    ts = R.tables("A", 6)
    E_c = R.envs_per_map(ts)
    steps, actions = R.expected("A", 6)
    assert E_c == 210 and steps.shape == (16 * E_c,) and actions.shape == (16 * E_c, 2)
    for m, t in enumerate(ts):
        for k in (0, 1, t.n_states - 1, min(t.n_states, E_c - 1), E_c - 1):  # (map 9 fills its block)
            s = t.states[k if k < t.n_states else 0]
            assert (int(steps[m * E_c + k]), actions[m * E_c + k].tolist()) == (t.answer(s)[0], R.policy_ref.joint_of(t.answer(s)[1], 2))
    rows = R.replay_rows(ts, E_c)
    assert len(rows) == 6 and all(r.shape == (16 * E_c, 2) for r in rows)
    m, k = 3, ts[3].n_states - 1
    prefix = ts[3].states[k].prefix
    assert [tuple(r[m * E_c + k]) for r in rows[:len(prefix)]] == [tuple(p) for p in prefix] and all((r[m * E_c + E_c - 1] == R.STAY).all() for r in rows)
    small = R.expected("A", 6, E_c=7)
    assert small[0].shape == (112,) and small[0][7 * 3 + 2] == ts[3].answer(ts[3].states[2])[0]


def test_rollout_seed_leaves_every_class():
    """The sampled states of the expert rollouts, by the oracle: environments with an answer, with a dead agent, and dead ends with
    everybody alive -- with and without auto-reset."""
    cfg = R.ROLLOUT
    for auto_reset, want in ((False, (536, 415, 73, 0)), (True, (770, 120, 134, 0))):
        steps, alive = R.sampled_answers(cfg["name"], cfg["horizon"], cfg["seed"], cfg["steps"], cfg["envs_per_map"], auto_reset)
        assert R.rollout_classes(steps, alive, cfg["envs_per_map"]) == want


# ---------------------------------------------------------------------------------------------------------------- the logic on the host
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_pieces_passes_and_answers_under_sanitizers(tmp_path):
    """tests/hostsim/policyforest_pieces.cpp: its own main over policyforest_logic.hpp and the shared logic headers, built with g++
    -fsanitize=address,undefined and run as a child process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "policyforest_pieces")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "policyforest_pieces.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in ("1", "2"):
        res = subprocess.run([exe, seed], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["levels"]) > 300 and int(out["served"]) > 10000 and int(out["lanes"]) > int(out["served"])
        assert int(out["passes"]) > 100 and int(out["answers"]) > 1000
