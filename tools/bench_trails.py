"""The trail search (lle_amd.trails, liblle_trails.so) per recorded search: records stored, levels, wall time -- and the help-graph
search of the same map at the same t_max (lle_amd.helpgraph, liblle_helpgraph.so, `standard`) beside it, as a record ratio and a time
ratio.

The layouts and searches are those of tests/golden/kat_trails.json.  Every handle exists before its clock starts; a row is the median
over --repeats of one `lle_trails_run` / `lle_helpgraph_run` through the Python binding (the cache is cleared between runs).  One JSON
line per search, then a summary line.

    python tools/bench_trails.py [--repeats 5] [--chunk 65536]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(solver, mode, collect_gems, repeats):
    import torch
    times = []
    for _ in range(repeats):
        solver._cache.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.find_shortest(mode, collect_gems=collect_gems)
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times), solver.last_stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=65536)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_trails.py needs an MI355X"
    from lle_amd import HelpGraphSolver, TrailSolver
    with open(os.path.join(ROOT, "tests", "golden", "kat_trails.json")) as f:
        cases = json.load(f)
    maps = dict({c["name"]: c["map"] for c in cases["catalogue"] if "map" in c}, **cases["maps"])
    rows, standard_cache = [], {}
    for s in cases["searches"]:
        if "changes" in s:  # a search on a changed world (tests/test_gpu_trails_edges.py): the tests' concern, not timed here, as bench_helpgraph.py
            continue
        key = (s["map"], s["t_max"], s["collect_gems"])
        if key not in standard_cache:
            standard = HelpGraphSolver(maps[s["map"]], s["t_max"], chunk=args.chunk)
            standard._handle()
            standard_cache[key] = timed(standard, "standard", s["collect_gems"], args.repeats)
            standard.free()
        standard_ms, standard_stats = standard_cache[key]
        ours = TrailSolver(maps[s["map"]], s["t_max"], chunk=args.chunk)
        ours._handle()
        mode = f"no-sequence-{s['n']}"
        ms, stats = timed(ours, mode, s["collect_gems"], args.repeats)
        ours.free()
        assert stats["n_states"] == s["states"] and stats["length"] == s["length"], (s, stats)
        row = dict(layout=s["map"], t_max=s["t_max"], mode=mode, collect_gems=s["collect_gems"], length=stats["length"], records=stats["n_states"],
                   levels=len(stats["expanded"]), ms=round(ms, 3), standard_length=standard_stats["length"], standard_records=standard_stats["n_states"],
                   standard_levels=len(standard_stats["expanded"]), standard_ms=round(standard_ms, 3),
                   record_ratio=round(stats["n_states"] / standard_stats["n_states"], 3), time_ratio=round(ms / standard_ms, 3))
        rows.append(row)
        print(json.dumps(row))
    print(json.dumps(dict(summary=True, device=torch.cuda.get_device_name(0), searches=len(rows), chunk=args.chunk, repeats=args.repeats,
                          total_ms=round(sum(r["ms"] for r in rows), 3), max_record_ratio=max(r["record_ratio"] for r in rows),
                          median_record_ratio=statistics.median(r["record_ratio"] for r in rows),
                          median_time_ratio=statistics.median(r["time_ratio"] for r in rows))))


if __name__ == "__main__":
    main()
