"""Filtering many small maps by the shape of cooperation they require: one help forest (lle_amd.helpforest, liblle_helpforest.so)
against a loop of one TrailCharacterizer per map (lle_amd.trails, liblle_trails.so, liblle_helpgraph.so, liblle_search.so).

256 maps `mapgen.generate(5, 5, 2, 2, 0, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s)`, s = 0 .. 255, t_max = 12, the constraint
`Asymmetric() & ~Sequential(3)` -- what a filtered generator asks of a batch of candidates.

  forest E=64 / 256 / 1024   `Constraint.satisfied_by_many(maps, characterizer=TrailCharacterizer)`: wall time of the whole call (handle
                             creation, the runs the constraint needs, free), and of the runs alone on handles that exist
  loop                       for every map `Constraint.is_satisfied_by(map, characterizer=TrailCharacterizer)`: wall time with the
                             creation of its handles, and of its searches alone (a characterizer that has answered once, its caches
                             emptied before the clock starts)

Per configuration: median wall time over --repeats, forest runs, pieces and occupancy.  One JSON line per configuration, then a
summary line.  The answers of every configuration are compared with each other before anything is printed.

    python tools/bench_helpforest.py [--maps 256] [--repeats 5] [--loop-repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_MAX = 12


def make_maps(n):
    from lle_amd import mapgen
    return [mapgen.generate(5, 5, 2, 2, 0, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s) for s in range(n)]


def constraint():
    from lle_amd import Asymmetric, Constraint, Sequential
    return Constraint(T_MAX, Asymmetric() & ~Sequential(3))


def sync():
    import torch
    torch.cuda.synchronize()


def bench_forest(maps, E, repeats):
    from lle_amd import TrailCharacterizer, helpforest
    c = constraint()
    whole, search = [], []
    answers = None
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        answers = c.satisfied_by_many(maps, characterizer=TrailCharacterizer, envs_per_map=E).tolist()
        whole.append(time.perf_counter() - t0)
    runs = []
    for _ in range(repeats):
        with helpforest.characterize_many(maps, T_MAX, envs_per_map=E) as many:
            for f in many.forests:  # every handle exists before the clock starts
                f._handle()
                f._no_cooperation(False, None)
                f._inner._cache.clear()
            sync()
            t0 = time.perf_counter()
            got = [c._accepts(many.entry(i)) for i in range(len(maps))]
            search.append(time.perf_counter() - t0)
            assert got == answers
            runs = many.runs
    pieces = sum(r.pieces for _mode, r in runs)
    valid, lanes = sum(r.valid_items for _mode, r in runs), sum(r.launched_lanes for _mode, r in runs)
    return dict(config=f"help forest E={E}", envs_per_map=E, whole_ms=1e3 * statistics.median(whole), search_ms=1e3 * statistics.median(search),
                runs=[mode for mode, _r in runs], searched=[int((r.n_states > 0).sum()) for _mode, r in runs], pieces=pieces, valid_items=valid,
                launched_lanes=lanes, occupancy=valid / lanes if lanes else 0.0), answers


def emptied(c):
    """A characterizer whose handles exist and whose answers are forgotten."""
    c._results.clear()
    s = c._solver
    while s is not None:
        s._cache.clear()
        s = getattr(s, "_inner", None)
    return c


def bench_loop(maps, repeats):
    from lle_amd import TrailCharacterizer, World
    c = constraint()
    whole, search = [], []
    answers = None
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        rows = []
        for text in maps:
            one = TrailCharacterizer(World(text), T_MAX)
            rows.append(c._accepts(one))
            one._solver.free()
        whole.append(time.perf_counter() - t0)
        answers = rows
        total = 0.0
        for text in maps:
            one = TrailCharacterizer(World(text), T_MAX)
            c._accepts(one)
            emptied(one)
            sync()
            t0 = time.perf_counter()
            c._accepts(one)
            total += time.perf_counter() - t0
            one._solver.free()
        search.append(total)
    return dict(config="loop of TrailCharacterizer", whole_ms=1e3 * statistics.median(whole), search_ms=1e3 * statistics.median(search)), answers


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--envs-per-map", type=int, nargs="+", default=[64, 256, 1024])
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_helpforest.py needs an MI355X"
    maps = make_maps(args.maps)
    results, answers = [], []
    for E in args.envs_per_map:
        row, a = bench_forest(maps, E, args.repeats)
        results.append(row)
        answers.append(a)
    row, a = bench_loop(maps, args.loop_repeats)
    results.append(row)
    answers.append(a)
    assert all(a == answers[0] for a in answers), "the configurations disagree"
    for row in results:
        print(json.dumps(row))
    loop = results[-1]
    best = min(results[:-1], key=lambda r: r["search_ms"])
    print(json.dumps(dict(summary=True, device=torch.cuda.get_device_name(0), n_maps=len(maps), t_max=T_MAX, accepted=sum(answers[0]),
                          loop_search_ms=loop["search_ms"], loop_whole_ms=loop["whole_ms"], best_forest=best["config"], best_forest_search_ms=best["search_ms"],
                          best_forest_whole_ms=best["whole_ms"], search_speedup=loop["search_ms"] / best["search_ms"], whole_speedup=loop["whole_ms"] / best["whole_ms"],
                          search_speedup_by_config={r["config"]: loop["search_ms"] / r["search_ms"] for r in results[:-1]})))


if __name__ == "__main__":
    main()
