"""Characterising many small maps: one forest (lle_amd.forest, liblle_forest.so) against a loop of one WorldCharacterizer per map
(lle_amd.solver, liblle_search.so).

256 maps `mapgen.generate(5, 5, 2, 2, 1, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s)`, s = 0 .. 255, t_max = 12, both modes
("standard", "no-cooperation") per map -- what a filtered generator asks of a batch of candidates.

  forest E=64 / 256 / 1024   `characterize_many` in one forest: wall time of the whole call (handle creation, two runs, free), and of
                             the two runs alone on a handle that exists
  loop                       for every map a WorldCharacterizer asked is_solvable / is_cooperative / is_independent: wall time with
                             the creation of its handle, and of its searches alone (the handle is made before the clock starts)

Per configuration: median wall time over --repeats, launches issued, occupancy.  One JSON line per configuration, then a summary
line.  The answers of every configuration are compared with each other before anything is printed.

    python tools/bench_forest.py [--maps 256] [--repeats 5] [--loop-repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T_MAX = 12
MODES = ("standard", "no-cooperation")


def make_maps(n):
    from lle_amd import mapgen
    return [mapgen.generate(5, 5, 2, 2, 1, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s) for s in range(n)]


def sync():
    import torch
    torch.cuda.synchronize()


def bench_forest(maps, E, repeats):
    from lle_amd import forest
    whole, search = [], []
    answers = None
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        many = forest.characterize_many(maps, T_MAX, envs_per_map=E)
        whole.append(time.perf_counter() - t0)
        answers = (many.solvable.tolist(), many.cooperative.tolist(), many.shortest_length.tolist(), many.shortest_independent_length.tolist())
    f = forest.ForestSolver(maps, T_MAX, envs_per_map=E)
    f._handle()
    runs = {}
    for _ in range(repeats):
        f._cache.clear()
        sync()
        t0 = time.perf_counter()
        for mode in MODES:
            runs[mode] = f.run(mode)
        search.append(time.perf_counter() - t0)
    pieces = sum(r.pieces for r in runs.values())
    valid, lanes = sum(r.valid_items for r in runs.values()), sum(r.launched_lanes for r in runs.values())
    solved = sum(int((r.length > 0).any()) for r in runs.values())
    f.free()
    return dict(config=f"forest E={E}", envs_per_map=E, whole_ms=1e3 * statistics.median(whole), search_ms=1e3 * statistics.median(search),
                launches=4 * pieces + 2 + solved, pieces=pieces, valid_items=valid, launched_lanes=lanes, occupancy=valid / lanes if lanes else 0.0), answers


def bench_loop(maps, repeats):
    from lle_amd import World, WorldCharacterizer
    whole, search = [], []
    launches = valid = lanes = 0
    answers = None
    for _ in range(repeats):
        # ---- with handle creation: the parent commit's way as a user writes it
        sync()
        t0 = time.perf_counter()
        rows = []
        for text in maps:
            c = WorldCharacterizer(World(text), T_MAX)
            rows.append((c.is_solvable(), c.is_cooperative(), c.is_independent(), c.shortest_path, c.shortest_independent_path))
            c._solver.free()
        whole.append(time.perf_counter() - t0)
        answers = ([r[0] for r in rows], [r[1] for r in rows], [-1 if r[3] is None else len(r[3]) for r in rows], [-1 if r[4] is None else len(r[4]) for r in rows])
        # ---- the searches alone: every handle exists before its clock starts
        total, launches, valid, lanes = 0.0, 0, 0, 0
        for text in maps:
            c = WorldCharacterizer(World(text), T_MAX)
            s = c._solver
            s._handle()
            sync()
            t0 = time.perf_counter()
            c.is_solvable(), c.is_cooperative(), c.is_independent()
            total += time.perf_counter() - t0
            for (_plan, stats) in s._cache.values():
                for d in range(len(stats["expanded"])):
                    items = stats["frontier"][d] * 5 ** s.world.n_agents
                    valid += items
                    for item0 in range(0, items, s.chunk):  # (a piece launches its items, rounded up to whole workgroups of 256)
                        launches += 4
                        lanes += -(-min(s.chunk, items - item0) // 256) * 256
            s.free()
        search.append(total)
    return dict(config="loop of WorldCharacterizer", whole_ms=1e3 * statistics.median(whole), search_ms=1e3 * statistics.median(search), launches=launches,
                valid_items=valid, launched_lanes=lanes, occupancy=valid / lanes if lanes else 0.0), answers


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--envs-per-map", type=int, nargs="+", default=[64, 256, 1024])
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_forest.py needs an MI355X"
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
    print(json.dumps(dict(summary=True, device=torch.cuda.get_device_name(0), n_maps=len(maps), t_max=T_MAX, solvable=sum(answers[0][0]), cooperative=sum(answers[0][1]),
                          loop_search_ms=loop["search_ms"], loop_whole_ms=loop["whole_ms"], best_forest=best["config"], best_forest_search_ms=best["search_ms"],
                          best_forest_whole_ms=best["whole_ms"], search_speedup=loop["search_ms"] / best["search_ms"], whole_speedup=loop["whole_ms"] / best["whole_ms"],
                          search_speedup_by_config={r["config"]: loop["search_ms"] / r["search_ms"] for r in results[:-1]})))


if __name__ == "__main__":
    main()
