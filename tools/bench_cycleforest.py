"""Filtering many small maps by the closed chain of help they require: one cycle forest (lle_amd.cycleforest, liblle_cycleforest.so)
against a loop of one CycleCharacterizer per map (lle_amd.cycles, liblle_cycles.so and the libraries below it).

256 maps `mapgen.generate(5, 5, 3, 3, 0, n_exits=3, wall_fraction=0.10, n_voids=0, seed=s)`, s = 0 .. 255, t_max = 10, two workloads:

  filter   the constraint `Interdependent(3)` -- what a filtered generator asks of a batch of candidates.  Most candidates are settled
           by the standard and no-cooperation runs and by the profile of their shortest plan; `searched` says how many reach the
           closed-trail search.
  search   the closed-trail search of order 3 itself on EVERY map: `CycleForestSolver.run_closed_trail(3)` against a loop of
           `CycleSolver.shortest_without_closed_trail(3)`.

  forest E=64 / 256 / 1024   wall time of the whole call (handle creation, the runs, free), and of the runs alone on handles that exist
  loop                       one CycleCharacterizer (CycleSolver) per map: wall time with the creation of its handles, and of its
                             searches alone (an object that has answered once and was told to `forget()` before the clock starts)

The configurations alternate inside every repeat, after one warm-up pass of each; per configuration the median wall time over
--repeats with the least and the largest, every clock stopped behind a device synchronise.  One JSON line per configuration, then a
summary line.  The answers of every configuration are compared with each other before anything is printed.

    python tools/bench_cycleforest.py [--maps 256] [--repeats 5]
    python tools/bench_cycleforest.py --scratch     # no GPU: the scratch bytes per lane of cf_insert<3> / <21> by the compiler's report
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_MAX, ORDER = 10, 3


def make_maps(n):
    from lle_amd import mapgen
    return [mapgen.generate(5, 5, 3, 3, 0, n_exits=3, wall_fraction=0.10, n_voids=0, seed=s) for s in range(n)]


def constraint():
    from lle_amd import Constraint, Interdependent
    return Constraint(T_MAX, Interdependent(ORDER))


def sync():
    import torch
    torch.cuda.synchronize()


def clock(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def scratch_bytes():
    """{kernel: scratch bytes per lane} of the cf_insert instantiations, from hipcc's resource report (compiles the device code once)."""
    src = os.path.join(ROOT, "lle_amd", "cycleforest", "cycleforest.hip")
    res = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src,
                          "-o", os.devnull], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True)
    out, name = {}, None
    for line in res.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "cf_insert" in name:
            out["cf_insert<3>" if "ILi3E" in name else "cf_insert<21>"] = int(m.group(1))
    return out


# ------------------------------------------------------------------------------------------------ the filter
class ForestFilter:
    def __init__(self, maps, E):
        self.maps, self.E, self.c = maps, E, constraint()
        self.config = f"filter: cycle forest E={E}"
        self.runs = []

    def whole(self):
        from lle_amd import CycleCharacterizer
        return self.c.satisfied_by_many(self.maps, characterizer=CycleCharacterizer, envs_per_map=self.E).tolist()

    def search(self):
        """(seconds of the runs alone, answers): every handle exists before the clock starts."""
        from lle_amd import cycleforest
        with cycleforest.characterize_many(self.maps, T_MAX, envs_per_map=self.E) as many:
            [self.c._accepts(many.entry(i)) for i in range(len(self.maps))]
            many.forget()
            seconds, got = clock(lambda: [self.c._accepts(many.entry(i)) for i in range(len(self.maps))])
            self.runs = list(many.runs)
        return seconds, got

    def row(self, whole, search):
        pieces = sum(r.pieces for _mode, r in self.runs)
        valid, lanes = sum(r.valid_items for _mode, r in self.runs), sum(r.launched_lanes for _mode, r in self.runs)
        return dict(config=self.config, envs_per_map=self.E, runs=[mode for mode, _r in self.runs], searched=[int((r.n_states > 0).sum()) for _mode, r in self.runs],
                    pieces=pieces, valid_items=valid, launched_lanes=lanes, occupancy=valid / lanes if lanes else 0.0, **times(whole, search))


class LoopFilter:
    config = "filter: loop of CycleCharacterizer"

    def __init__(self, maps):
        self.maps, self.c = maps, constraint()

    def whole(self):
        from lle_amd import CycleCharacterizer, World
        rows = []
        for text in self.maps:
            one = CycleCharacterizer(World(text), T_MAX)
            rows.append(self.c._accepts(one))
            one._solver.free()
        return rows

    def search(self):
        from lle_amd import CycleCharacterizer, World
        total, rows = 0.0, []
        for text in self.maps:
            one = CycleCharacterizer(World(text), T_MAX)
            self.c._accepts(one)
            one.forget()
            seconds, got = clock(lambda: self.c._accepts(one))
            total += seconds
            rows.append(got)
            one._solver.free()
        return total, rows

    def row(self, whole, search):
        return dict(config=self.config, **times(whole, search))


# ------------------------------------------------------------------------------------------------ the search itself, on every map
def lengths(plans):
    return [None if p is None else len(p) for p in plans]


class ForestSearch:
    def __init__(self, maps, E):
        self.maps, self.E = maps, E
        self.config = f"search: cycle forest E={E}"
        self.last = None

    def whole(self):
        from lle_amd import cycleforest
        f = cycleforest.CycleForestSolver(self.maps, T_MAX, envs_per_map=self.E)
        try:
            return lengths(f.run_closed_trail(ORDER).plans)
        finally:
            f.free()

    def search(self):
        from lle_amd import cycleforest
        f = cycleforest.CycleForestSolver(self.maps, T_MAX, envs_per_map=self.E)
        try:
            f.run_closed_trail(ORDER)  # (makes the handle)
            f.forget()
            seconds, self.last = clock(lambda: f.run_closed_trail(ORDER))
            return seconds, lengths(self.last.plans)
        finally:
            f.free()

    def row(self, whole, search):
        r = self.last
        return dict(config=self.config, envs_per_map=self.E, searched=len(self.maps), records=int(r.n_states.sum()), pieces=r.pieces, valid_items=r.valid_items,
                    launched_lanes=r.launched_lanes, occupancy=r.occupancy, **times(whole, search))


class LoopSearch:
    config = "search: loop of CycleSolver"

    def __init__(self, maps):
        self.maps = maps

    def whole(self):
        from lle_amd import CycleSolver, World
        rows = []
        for text in self.maps:
            one = CycleSolver(World(text), T_MAX)
            rows.append(one.shortest_without_closed_trail(ORDER))
            one.free()
        return lengths(rows)

    def search(self):
        from lle_amd import CycleSolver, World
        total, rows = 0.0, []
        for text in self.maps:
            one = CycleSolver(World(text), T_MAX)
            one.shortest_without_closed_trail(ORDER)  # (makes the handle)
            one.forget()
            seconds, got = clock(lambda: one.shortest_without_closed_trail(ORDER))
            total += seconds
            rows.append(got)
            one.free()
        return total, lengths(rows)

    def row(self, whole, search):
        return dict(config=self.config, **times(whole, search))


def times(whole, search):
    ms = lambda xs: [round(1e3 * x, 3) for x in (statistics.median(xs), min(xs), max(xs))]  # noqa: E731
    (w, w_lo, w_hi), (s, s_lo, s_hi) = ms(whole), ms(search)
    return dict(whole_ms=w, whole_ms_range=[w_lo, w_hi], search_ms=s, search_ms_range=[s_lo, s_hi])


def measure(configs, repeats):
    """One warm-up pass of every configuration, then `repeats` passes in which the configurations alternate."""
    answers = []
    for c in configs:
        answers.append(c.whole())
        assert c.search()[1] == answers[-1], c.config
    assert all(a == answers[0] for a in answers), "the configurations disagree"
    whole, search = {c.config: [] for c in configs}, {c.config: [] for c in configs}
    for _ in range(repeats):
        for c in configs:
            seconds, got = clock(c.whole)
            assert got == answers[0]
            whole[c.config].append(seconds)
            seconds, got = c.search()
            assert got == answers[0]
            search[c.config].append(seconds)
    return [c.row(whole[c.config], search[c.config]) for c in configs], answers[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--envs-per-map", type=int, nargs="+", default=[1024, 256, 64])
    ap.add_argument("--scratch", action="store_true", help="print the scratch bytes per lane of the insert kernels (compiles; needs no GPU) and stop")
    args = ap.parse_args()
    if args.scratch:
        print(json.dumps(dict(scratch_bytes_per_lane=scratch_bytes())))
        return
    import torch
    assert torch.cuda.is_available(), "bench_cycleforest.py needs an MI355X"
    maps = make_maps(args.maps)
    for name, forests, loop in (("filter", [ForestFilter(maps, E) for E in args.envs_per_map], LoopFilter(maps)),
                                ("search", [ForestSearch(maps, E) for E in args.envs_per_map], LoopSearch(maps))):
        rows, answers = measure(forests + [loop], args.repeats)
        for row in rows:
            print(json.dumps(row), flush=True)
        last, best = rows[-1], min(rows[:-1], key=lambda r: r["search_ms"])
        kept = sum(bool(a) for a in answers) if name == "filter" else sum(a is not None for a in answers)
        print(json.dumps(dict(summary=name, device=torch.cuda.get_device_name(0), n_maps=len(maps), t_max=T_MAX, order=ORDER,
                              **({"accepted": kept} if name == "filter" else {"with_a_plan": kept}), loop_search_ms=last["search_ms"], loop_whole_ms=last["whole_ms"],
                              best_forest=best["config"], best_forest_search_ms=best["search_ms"], best_forest_whole_ms=best["whole_ms"],
                              search_speedup=last["search_ms"] / best["search_ms"], whole_speedup=last["whole_ms"] / best["whole_ms"],
                              search_speedup_by_config={r["config"]: last["search_ms"] / r["search_ms"] for r in rows[:-1]})), flush=True)


if __name__ == "__main__":
    main()
