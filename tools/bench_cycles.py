"""The closed-trail search (lle_amd.cycles, liblle_cycles.so) per recorded search: records stored, levels, wall time -- and
`TrailSolver`'s `standard` search of the same map at the same t_max in the same run beside it (liblle_helpgraph.so through the inner
solver), which is what the times are read against, as a record ratio and a time ratio.

The layouts and searches are those of tests/golden/kat_cycles.json.  Every handle exists before its clock starts and has run once
(warm-up); a row is the median over --repeats of one `lle_cycles_run` / one `standard` search through the Python binding (the cache is
cleared between runs).  One JSON line per search, then a summary line.

    python tools/bench_cycles.py [--repeats 5] [--chunk 65536]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(solver, mode, collect_gems):
    """One search: an int is an order for CycleSolver's native search, a text a mode of TrailSolver (whose inner solver's cache is cleared too)."""
    if isinstance(mode, int):
        solver.shortest_without_closed_trail(mode, collect_gems=collect_gems)
        return
    if solver._inner is not None:
        solver._inner._cache.clear()
    solver.find_shortest(mode, collect_gems=collect_gems)


def timed(solver, mode, collect_gems, repeats):
    import torch
    run(solver, mode, collect_gems)  # warm-up: handles, code objects
    times = []
    for _ in range(repeats):
        solver._cache.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(solver, mode, collect_gems)
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times), solver.last_stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=65536)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_cycles.py needs an MI355X"
    from lle_amd import CycleSolver, TrailSolver
    with open(os.path.join(ROOT, "tests", "golden", "kat_cycles.json")) as f:
        cases = json.load(f)
    maps = dict({c["name"]: c["map"] for c in cases["catalogue"]}, **cases["maps"])
    rows, standard_cache = [], {}
    for s in cases["searches"]:
        if "changes" in s:  # a search on a changed world: the tests' concern, not timed here, as bench_trails.py
            continue
        key = (s["map"], s["t_max"], s["collect_gems"])
        if key not in standard_cache:
            standard = TrailSolver(maps[s["map"]], s["t_max"], chunk=args.chunk)
            standard_cache[key] = timed(standard, "standard", s["collect_gems"], args.repeats)
            standard.free()
        standard_ms, standard_stats = standard_cache[key]
        ours = CycleSolver(maps[s["map"]], s["t_max"], chunk=args.chunk)
        ours._handle()
        mode = f"no-interdependence-{s['n']}"
        ms, stats = timed(ours, s["n"], s["collect_gems"], args.repeats)
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
