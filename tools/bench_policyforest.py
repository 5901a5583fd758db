"""What the forest of steps-to-go tables costs (lle_amd.PolicyForest, liblle_policyforest.so) against a loop of one OptimalPolicy per map
(liblle_policy.so).  Nobody promised a figure for any of these; profiles/r21_policyforest.md holds what was measured.

BUILD   256 maps `mapgen.generate(5, 5, 2, 2, 1, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s)`, s = 0 .. 255, horizon 12 -- the
        shape of tools/bench_forest.py.  One PolicyForest at envs_per_map 64 / 256 / 1024: wall time of the constructor (handle
        creation and build), of the build alone on a handle that exists (`rebuild`), occupancy of both phases, passes per map.  The
        loop: one OptimalPolicy per map, with the creation of its handle; the builds alone come from the library's own explore_ms +
        relax_ms.  Every configuration's per-map figures are compared with each other before anything is printed.
LOOKUP  256 maps x 256 environments after 30 sampled steps, HIP events around loops, the variants timed in alternation:
        plain_step, forest_act_and_step, forest_lookup; the same on 65 536 environments of ONE map with OptimalPolicy
        (single_plain_step, single_act_and_step, single_lookup); and 256 single-map lookups of 256 environments each (loop_of_lookups).

One JSON line per configuration.  GPU box.

    python tools/bench_policyforest.py [--maps 256] [--repeats 3] [--steps 300] [--warmup 30] [--rounds 5] [--skip-loop]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_policyforest.py --child --only lookup --variants forest_lookup,single_lookup --rounds 1

The measurement runs in a child process under a time limit (--timeout seconds): a hang ends there."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HORIZON = 12


def make_maps(n):
    from lle_amd import mapgen
    return [mapgen.generate(5, 5, 2, 2, 1, n_exits=2, wall_fraction=0.12, n_voids=0, seed=s) for s in range(n)]


def sync():
    import torch
    torch.cuda.synchronize()


def figures(n_states, depth, complete, roots):
    return [int(v) for v in n_states], [int(v) for v in depth], [bool(v) for v in complete], [int(v) for v in roots]


def bench_build_forest(maps, E, repeats):
    from lle_amd import PolicyForest
    whole, build = [], []
    pf = None
    for _ in range(repeats):
        if pf is not None:
            pf.free()
        sync()
        t0 = time.perf_counter()
        pf = PolicyForest(maps, HORIZON, envs_per_map=E)
        whole.append(time.perf_counter() - t0)
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        pf.rebuild()
        build.append(time.perf_counter() - t0)
    passes = sorted(pf.passes.tolist())
    row = dict(config=f"forest E={E}", envs_per_map=E, whole_ms=1e3 * statistics.median(whole), build_ms=1e3 * statistics.median(build),
               explore_ms=pf.explore_ms, relax_ms=pf.relax_ms, occupancy_explore=pf.occupancy["explore"], occupancy_relax=pf.occupancy["relax"],
               explore_lanes=pf.occupancy["explore_lanes"], relax_lanes=pf.occupancy["relax_lanes"], states=int(pf.n_states.sum()),
               passes_min=passes[0], passes_median=passes[len(passes) // 2], passes_max=passes[-1], over_capacity=int(pf.over_capacity.sum()))
    answers = figures(pf.n_states, pf.depth_reached, pf.complete, pf.root_steps)
    pf.free()
    return row, answers


def bench_build_loop(maps, repeats):
    from lle_amd import OptimalPolicy
    whole, build = [], []
    answers = None
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        rows, inner = [], 0.0
        for text in maps:
            p = OptimalPolicy(text, HORIZON)
            rows.append((p.n_states, p.depth_reached, p.complete, p.root_steps, p.passes))
            inner += p.stats["explore_ms"] + p.stats["relax_ms"]
            p.free()
        whole.append(time.perf_counter() - t0)
        build.append(inner)
        # (OptimalPolicy.root_steps is None for both sentinels: compared as "has a plan")
        answers = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [-1 if r[3] is None else r[3] for r in rows])
    passes = sorted(r[4] for r in rows)
    return dict(config="loop of OptimalPolicy", whole_ms=1e3 * statistics.median(whole), build_ms=statistics.median(build), passes_min=passes[0],
                passes_median=passes[len(passes) // 2], passes_max=passes[-1]), answers


def bench_lookup(maps, args):
    import torch

    from lle_amd import BatchedWorld, OptimalPolicy, PolicyForest
    M, E = len(maps), args.envs_per_map
    n = M * E
    pf = PolicyForest(maps, HORIZON)
    many, single = BatchedWorld(maps, n), BatchedWorld(maps[0], n)
    singles = [BatchedWorld(text, E) for text in maps]
    one = OptimalPolicy(maps[0], HORIZON)
    for t in range(30):
        many.step(sample=True, seed=7, t=t)
        single.step(sample=True, seed=7, t=t)
    starts = {id(many): many.snapshot(), id(single): single.snapshot()}
    buf = torch.empty(n, dtype=torch.int32, device=many.device)
    small = torch.empty(E, dtype=torch.int32, device=many.device)
    first = pf.steps_to_go(many)
    out = dict(config="lookup", n_maps=M, envs_per_map=E, envs=n, steps=args.steps, warmup=args.warmup, rounds=args.rounds,
               after_30_sampled_steps=dict(exact=int((first >= 0).sum()), unknown=int((first == pf.UNKNOWN).sum()), dead_end=int((first == pf.DEAD_END).sum())))

    def plain_step(t):
        many.step(sample=True, auto_reset=True, seed=7, t=t)

    def forest_lookup(t):
        pf.steps_to_go(many, check_map=False, out=buf)

    def forest_act_and_step(t):
        pf.act(many, check_map=False, out=buf)
        many.step(many.actions, auto_reset=True)

    def single_plain_step(t):
        single.step(sample=True, auto_reset=True, seed=7, t=t)

    def single_lookup(t):
        one.steps_to_go(single, check_map=False, out=buf)

    def single_act_and_step(t):
        one.act(single, check_map=False, out=buf)
        single.step(single.actions, auto_reset=True)

    def loop_of_lookups(t):
        for m, bw in enumerate(singles):
            pf.steps_to_go(bw, check_map=False, out=small, map_index=m)

    variants = dict(plain_step=plain_step, forest_lookup=forest_lookup, forest_act_and_step=forest_act_and_step, single_plain_step=single_plain_step,
                    single_lookup=single_lookup, single_act_and_step=single_act_and_step, loop_of_lookups=loop_of_lookups)
    if args.variants:
        variants = {k: variants[k] for k in args.variants.split(",")}

    def run(name, steps):
        fn = variants[name]
        if name == "loop_of_lookups":
            steps = max(1, steps // 16)
        for bw in (many, single):
            bw.restore(starts[id(bw)])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(steps):
            fn(30 + t)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps  # us per iteration

    for name in variants:
        run(name, args.warmup)
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name in variants:  # alternating: drifts of the box hit all alike
            times[name].append(run(name, args.steps))
    u = out["us_per_call"] = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["all_rounds_us"] = {k: [round(x, 3) for x in v] for k, v in times.items()}
    if "forest_act_and_step" in u and "plain_step" in u:
        out["forest_act_cost_us"] = round(u["forest_act_and_step"] - u["plain_step"], 3)
    if "single_act_and_step" in u and "single_plain_step" in u:
        out["single_act_cost_us"] = round(u["single_act_and_step"] - u["single_plain_step"], 3)
    return out


def measure(args):
    import torch
    assert torch.cuda.is_available(), "bench_policyforest.py needs an MI355X"
    maps = make_maps(args.maps)
    if args.only in (None, "build"):
        results, answers = [], []
        for E in args.envs_per_map_build:
            row, a = bench_build_forest(maps, E, args.repeats)
            results.append(row)
            answers.append(a)
        for a in answers[1:]:
            assert a == answers[0], "the forests disagree"
        if not args.skip_loop:
            row, a = bench_build_loop(maps, args.loop_repeats)
            results.append(row)
            mine = answers[0]
            assert a[:3] == mine[:3] and a[3] == [v if v >= 0 else -1 for v in mine[3]], "the loop of OptimalPolicy and the forest disagree"
        for row in results:
            print(json.dumps(row), flush=True)
    if args.only in (None, "lookup"):
        print(json.dumps(bench_lookup(maps, args)), flush=True)
    from lle_amd import policyforest
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), kernels=policyforest.launched_kernels())), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--maps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-repeats", type=int, default=2)
    ap.add_argument("--envs-per-map-build", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--envs-per-map", type=int, default=256, help="environments per map of the looked-up batch")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["build", "lookup"], default=None)
    ap.add_argument("--skip-loop", action="store_true", help="no loop of one OptimalPolicy per map")
    ap.add_argument("--variants", default=None, help="comma-separated subset of the lookup variants (under a profiler: `forest_lookup` alone gives pf_lookup's time)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts, or a profiler wraps)")
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
