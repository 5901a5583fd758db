"""The steps-to-go table without a GPU: header / exports / binding of liblle_policy.so, every host-side refusal, the map fingerprint, and
what lle_amd/policy/policy_logic.hpp adds to the search's table code under AddressSanitizer + UndefinedBehaviorSanitizer in a
stand-alone program (tests/hostsim/policy_values.cpp).  The table itself is built on the MI355X (tests/test_gpu_policy.py)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import lle_amd
from lle_amd import Map, World, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = "S0 . . X"
SEVEN = " ".join(f"S{k}" for k in range(7)) + " X" * 7
KERNELS = ["policy_commit", "policy_expand", "policy_insert", "policy_lookup", "policy_relax"]


def test_library_exports():
    """liblle_policy.so exports every function include/lle_policy.h declares, and the binding knows exactly those; the header is plain C
    and the one the library is compiled against; struct sizes, field offsets and constants of the binding are the header's."""
    L = policy.lib()
    header = open(os.path.join(ROOT, "include", "lle_policy.h")).read()
    declared = set(re.findall(r"\b(lle_policy_[a-z_0-9]+)\s*\(", header))
    assert declared == set(policy.EXPORTS)
    assert all(hasattr(L, s) for s in declared)
    source = open(os.path.join(ROOT, "lle_amd", "policy", "policy.hip")).read()
    logic = open(os.path.join(ROOT, "lle_amd", "policy", "policy_logic.hpp")).read()
    assert '#include "../../include/lle_policy.h"' in source and '#include "policy_logic.hpp"' in source
    assert '#include "../search/search_logic.hpp"' in logic
    assert "lle_batch_set_state" not in source and "capi_internal" not in source  # states move through the buffers of the public ABI only
    shared = [open(os.path.join(ROOT, "lle_amd", "search", h)).read() for h in ("search_logic.hpp", "search_device.hpp")]
    assert '#include "../search/search_device.hpp"' in source
    for text in [source, logic] + shared:  # everything that compiles into the library: 32-bit global atomics, no inline assembly
        assert "unsigned long long" not in text and "asm" not in text
    structs = {"lle_policy_options": policy.PolicyOptions, "lle_policy_args": policy.PolicyArgs, "lle_policy_result": policy.PolicyResult}
    fields = [(name, f) for name, cls in structs.items() for f, _ in cls._fields_]
    prints = "".join(f'printf("%zu ", sizeof({name}));' for name in structs)
    prints += "".join(f'printf("%zu ", offsetof({name}, {f}));' for name, f in fields)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "lle_policy.h"\nint main(void) { ' + prints +
            'printf("%d %d %d %d %d", LLE_POLICY_CAPACITY, LLE_POLICY_UNKNOWN, LLE_POLICY_DEAD_END, LLE_POLICY_MAX_AGENTS, LLE_POLICY_MAX_HORIZON); return 0; }\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sizes.c"), os.path.join(d, "sizes")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(cls) for cls in structs.values()] + [getattr(structs[name], f).offset for name, f in fields]
    want += [policy.LLE_POLICY_CAPACITY, policy.LLE_POLICY_UNKNOWN, policy.LLE_POLICY_DEAD_END, policy.LLE_POLICY_MAX_AGENTS, policy.LLE_POLICY_MAX_HORIZON]
    assert got == want
    assert (policy.OptimalPolicy.UNKNOWN, policy.OptimalPolicy.DEAD_END) == (-1, -2)
    assert sorted(policy.compiled_kernels()) == KERNELS
    assert policy.launched_kernels() == []


def test_the_files_of_the_search_are_not_this_library_s():
    """policy.hip has its own kernels: the search's and the forest's sources do not know the library."""
    for path in ("lle_amd/search/search.hip", "lle_amd/search/search_logic.hpp", "lle_amd/search/search_device.hpp", "lle_amd/forest/forest.hip",
                 "lle_amd/forest/forest_logic.hpp", "include/lle_search.h", "include/lle_forest.h"):
        assert "policy" not in open(os.path.join(ROOT, path)).read()


def test_lazy_names():
    assert lle_amd.OptimalPolicy is policy.OptimalPolicy and lle_amd.PolicyCapacityError is policy.PolicyCapacityError
    assert issubclass(lle_amd.PolicyCapacityError, RuntimeError)
    assert {"OptimalPolicy", "PolicyCapacityError"} <= set(lle_amd.__all__)


def test_host_side_refusals():
    L, line = policy.lib(), Map(LINE)
    assert L.lle_policy_create(None, None) is None and b"NULL" in L.lle_policy_last_error()
    bad = policy.PolicyOptions(4, -1, 0, 0, None)
    assert L.lle_policy_create(line.h, C.byref(bad)) is None and b"struct_bytes" in L.lle_policy_last_error()
    for chunk, max_states, word in ((-1, 0, b"chunk"), ((1 << 30) + 1, 0, b"chunk"), (0, -1, b"max_states"), (0, 1 << 31, b"max_states"),
                                    (0, (1 << 30) + 1, b"max_states")):
        opt = policy.PolicyOptions(C.sizeof(policy.PolicyOptions), -1, chunk, max_states, None)
        assert L.lle_policy_create(line.h, C.byref(opt)) is None and word in L.lle_policy_last_error()
    assert L.lle_policy_create(Map(SEVEN).h, None) is None and b"more than 6 agents" in L.lle_policy_last_error()
    assert L.lle_policy_build(None, None, None) == -1 and b"NULL" in L.lle_policy_last_error()
    assert L.lle_policy_stats(None, None, None, 0) == -1
    assert L.lle_policy_lookup(None, None, None, None, 0, None) == -1 and b"NULL" in L.lle_policy_last_error()
    assert L.lle_policy_map_fingerprint(None) == 0 and b"NULL" in L.lle_policy_last_error()
    L.lle_policy_free(None)


def test_constructor_refusals():
    for horizon in (-1, 32768):
        with pytest.raises(ValueError, match="horizon"):
            policy.OptimalPolicy(LINE, horizon)
    with pytest.raises(ValueError):
        policy.OptimalPolicy(LINE, 5, chunk=0)
    with pytest.raises(ValueError):
        policy.OptimalPolicy(LINE, 5, max_states=0)
    with pytest.raises(ValueError, match="at most 6 agents"):
        policy.OptimalPolicy(SEVEN, 4)
    with pytest.raises(ValueError, match="at most 6 agents"):
        policy.OptimalPolicy(World(SEVEN), 4)


def test_fingerprint():
    w = World("S0 . X X")
    first = policy.map_fingerprint(w._map)
    assert first == policy.map_fingerprint(w._map.clone()) == policy.map_fingerprint(Map("S0 . X X")) and 0 < first < 1 << 64
    w.exit_pos = [(0, 3)]
    assert policy.map_fingerprint(w._map) != first
    assert policy.map_fingerprint(Map("S0 . X X", row_align=256)) == first  # the pitch of an observation row decides no step
    prints = {policy.map_fingerprint(Map(text)) for text in ("S0 . X X", "S0 . X .", "S0 . X @", "S0 G X X", "S0 V X X", "S0 . X X\n. . . .",
                                                              "S0 . X X\nL0E . . .", "S0 . X X\nL0E . . @", "S0 . X X\n. L0E . .")}
    assert len(prints) == 9
    coloured = Map("S0 . X X\nS1 . . .\nL0E . . .")
    before = policy.map_fingerprint(coloured)
    coloured.set_source(0, agent_id=1)
    recoloured = policy.map_fingerprint(coloured)
    coloured.set_source(0, enabled=False)
    assert len({before, recoloured, policy.map_fingerprint(coloured)}) == 3


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_value_and_find_code_under_sanitizers(tmp_path):
    """tests/hostsim/policy_values.cpp: its own main over policy_logic.hpp, built with g++ -fsanitize=address,undefined and run as a child
    process; nothing sanitized is loaded into this interpreter."""
    exe = str(tmp_path / "policy_values")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "hostsim", "policy_values.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        out = dict(kv.split("=") for kv in res.stdout.split()[1:])
        assert res.stdout.startswith("OK ") and int(out["hits"]) > 5000 and int(out["misses"]) > 5000 and int(out["wraps"]) > 1000 and int(out["full"]) == 40
