"""What the shortest-plan search does per second: level 4 (t_max 10), the layout `paper-fully-coupled` (t_max 10) and level 6 (t_max
21, the pool as large as --max-states allows; an overflow is reported with the depth at which it happened), each in mode standard.
Per map: distinct states, available joint actions expanded, seconds of lle_search_run (wall clock around the call, which synchronises;
the handle is made before the clock starts) and expansions per second.  Nobody promised a figure.  Prints one JSON line.  GPU box.

    python tools/bench_solver.py [--max-states 16777216] [--chunk 65536] [--repeats 3] [--only level4] [--profile DIR]

--profile DIR adds "kernel_shares" to the line: the share of the kernel time in the step launch against search_expand, search_insert
and search_commit, from ONE `rocprofv3 --kernel-trace --stats -d DIR` run of level 6 (a run of its own, no counters, one repeat),
whose kernel statistics the tool reads back and sums per kernel.

Every measurement runs in a child process under a time limit (--timeout seconds, `timeout -k` around the profiler): a hang ends there."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULLY_COUPLED = """
 @  L0S  @ @ @ @
S0   .   . . @ @
S1   .   . . . @
S2   .   . . . @
 @  L2E  . . . @
 @   @   X X X L1W
"""


def measure(args):
    from lle_amd import Map, solver
    from lle_amd.solver import SolveMode

    cases = {"level4": (Map(level=4), 10, 1 << 22), "fully_coupled": (Map(FULLY_COUPLED), 10, 1 << 22), "level6": (Map(level=6), 21, args.max_states)}
    out = {"chunk": args.chunk, "repeats": args.repeats, "cases": {}}
    for name, (map_, t_max, max_states) in cases.items():
        if args.only and name != args.only:
            continue
        s = solver.Solver(map_, t_max, chunk=args.chunk, max_states=max_states)
        s._handle()
        runs, row = [], {"t_max": t_max, "max_states": max_states}
        for _ in range(args.repeats):
            s._cache.clear()
            t0 = time.perf_counter()
            try:
                s._shortest(SolveMode.standard(), False)
            except solver.SolverCapacityError as e:
                row["overflow"] = str(e)
                m = re.search(r"at depth (\d+)", str(e))
                row["overflow_depth"] = int(m.group(1)) if m else None
                runs.append(time.perf_counter() - t0)
                break
            runs.append(time.perf_counter() - t0)
        st = s.last_stats
        if st is not None and "overflow" not in row:
            expanded = sum(st["expanded"])
            row.update(length=st["length"], n_states=st["n_states"], expanded=expanded, frontier=st["frontier"],
                       expansions_per_second=round(expanded / min(runs)) if runs and min(runs) > 0 else None)
        row["seconds"] = [round(r, 4) for r in runs]
        out["cases"][name] = row
        s.free()
    print(json.dumps(out))


GROUPS = ("search_expand", "search_insert", "search_commit", "step_kernel")


def kernel_shares(directory, args):
    """One kernel-trace run of level 6 under the profiler, in a child under a time limit; {kernel group: share of the kernel time}."""
    argv = ["timeout", "-k", "10", str(args.timeout), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", directory, "-o", "solver", "--",
            sys.executable, os.path.abspath(__file__), "--child", "--only", "level6", "--repeats", "1", "--max-states", str(args.max_states),
            "--chunk", str(args.chunk)]
    res = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        return {"error": f"rocprofv3 run ended with {res.returncode}", "tail": res.stdout[-500:]}
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        seen = [os.path.relpath(f, directory) for f in glob.glob(os.path.join(directory, "**", "*"), recursive=True) if os.path.isfile(f)]
        return {"error": "no kernel_stats.csv under " + directory, "files": seen[:20]}
    total = {g: 0.0 for g in GROUPS + ("other",)}
    calls = {g: 0 for g in GROUPS + ("other",)}
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0)
            group = next((g for g in GROUPS if g in name), "other")
            total[group] += ns
            calls[group] += int(float(row.get("Calls") or 0))
    whole = sum(total.values()) or 1.0
    return {"file": os.path.relpath(files[0], directory), "total_ms": round(whole / 1e6, 3),
            "share": {g: round(v / whole, 4) for g, v in total.items()}, "ms": {g: round(v / 1e6, 3) for g, v in total.items()}, "calls": calls}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-states", type=int, default=1 << 24)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["level4", "fully_coupled", "level6"])
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--profile", metavar="DIR")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        measure(a)
    else:  # a fresh child process under a time limit
        argv = [sys.executable, os.path.abspath(__file__), "--child", "--max-states", str(a.max_states), "--chunk", str(a.chunk), "--repeats", str(a.repeats)]
        argv += ["--only", a.only] if a.only else []
        res = subprocess.run(argv, timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        if res.returncode != 0:  # nothing more is started on the GPU after a failed run
            sys.stdout.write(res.stdout)
            sys.exit(res.returncode)
        line = json.loads(res.stdout.strip().splitlines()[-1])
        if a.profile:
            line["kernel_shares"] = kernel_shares(a.profile, a)
        print(json.dumps(line))
