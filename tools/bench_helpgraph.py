"""The help-graph search (lle_amd.helpgraph, liblle_helpgraph.so) per layout and mode: records stored, levels, wall time -- and the plain
search of the same map (lle_amd.solver, liblle_search.so, `standard`) beside it, with the ratio of records stored.

The layouts and searches are those of tests/golden/kat_helpgraph.json.  Every handle exists before its clock starts; a row is the
median over --repeats of one `lle_helpgraph_run` / `lle_search_run` through the Python binding (the cache is cleared between runs).
One JSON line per search, then a summary line.

    python tools/bench_helpgraph.py [--repeats 5] [--chunk 65536]
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
    assert torch.cuda.is_available(), "bench_helpgraph.py needs an MI355X"
    from lle_amd import HelpGraphSolver, Solver
    with open(os.path.join(ROOT, "tests", "golden", "kat_helpgraph.json")) as f:
        cases = json.load(f)
    maps = dict({c["name"]: c["map"] for c in cases["catalogue"]}, **cases["maps"])
    rows, plain_cache = [], {}
    for s in cases["searches"]:
        if "changes" in s:  # a search on a changed world (tests/golden/make_kat_helpgraph.py): the tests' concern, not timed here
            continue
        key = (s["map"], s["t_max"], s["collect_gems"])
        if key not in plain_cache:
            plain = Solver(maps[s["map"]], s["t_max"], chunk=args.chunk)
            plain._handle()
            plain_cache[key] = timed(plain, "standard", s["collect_gems"], args.repeats)
            plain.free()
        plain_ms, plain_stats = plain_cache[key]
        ours = HelpGraphSolver(maps[s["map"]], s["t_max"], chunk=args.chunk)
        ours._handle()
        mode = f"{s['mode']}-{s['param']}" if s["mode"] in ("no-convergence", "no-divergence") else s["mode"]
        ms, stats = timed(ours, mode, s["collect_gems"], args.repeats)
        ours.free()
        assert stats["n_states"] == s["states"] and stats["length"] == s["length"], (s, stats)
        row = dict(layout=s["map"], t_max=s["t_max"], mode=mode, collect_gems=s["collect_gems"], length=stats["length"], records=stats["n_states"],
                   levels=len(stats["expanded"]), ms=round(ms, 3), plain_length=plain_stats["length"], plain_states=plain_stats["n_states"],
                   plain_levels=len(plain_stats["expanded"]), plain_ms=round(plain_ms, 3), records_per_plain_state=round(stats["n_states"] / plain_stats["n_states"], 3))
        rows.append(row)
        print(json.dumps(row))
    print(json.dumps(dict(summary=True, device=torch.cuda.get_device_name(0), searches=len(rows), chunk=args.chunk, repeats=args.repeats,
                          total_ms=round(sum(r["ms"] for r in rows), 3), max_ratio=max(r["records_per_plain_state"] for r in rows),
                          median_ratio=statistics.median(r["records_per_plain_state"] for r in rows))))


if __name__ == "__main__":
    main()
