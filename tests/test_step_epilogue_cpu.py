"""tests/hostsim/stat_fields.cpp: the packed counters of a single step (step_logic.hpp stat_pack_* / stat_unpack, written once for host and
device) summed over a wavefront's environments on the host -- every field at its maximum for every G, all of them together, random values
below -- built with g++ -fsanitize=address,undefined and run as a child process; nothing sanitized is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def test_packed_counters_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stat_fields")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "hostsim", "stat_fields.cpp"), "-o", exe] + SAN, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        res = subprocess.run([exe, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
        assert res.returncode == 0, f"rc={res.returncode}\n{res.stdout[-3000:]}\n{res.stderr[-6000:]}"
        # 5 lane-group sizes x 2 bounds x (7 single fields + all together + 200 random wavefronts), and the 64-environment wavefront
        assert res.stdout.split() == ["OK", f"cases={5 * 2 * (7 + 1 + 200) + 1}"], res.stdout
