"""What the steps-to-go table costs: the build (explore / relax, passes, states) of the largest built-in level that explores completely
within the default capacity, and, on 65 536 environments of that level after 30 sampled steps, one lookup launch and `act` + step --
next to the same batch's plain step launch and to a launch of the library's own that has nothing to do (the lookup over a batch of ONE
environment).  HIP events around loops, one process, the variants timed in alternation.  Nobody promised a figure for any of these.
Prints one JSON line.  GPU box.

    python tools/bench_policy.py [--levels 5,4,3,2,1] [--envs 65536] [--steps 500] [--warmup 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_policy.py --child --rounds 1 --variants lookup     (the lookup kernel's own time)

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


def measure(args):
    import torch

    from lle_amd import BatchedWorld, Map, OptimalPolicy, PolicyCapacityError

    out = {"envs": args.envs, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "levels_tried": {}}
    pol = level = None
    for candidate in [int(v) for v in args.levels.split(",")]:
        t0 = time.perf_counter()
        try:
            p = OptimalPolicy(Map(level=candidate))
        except PolicyCapacityError as e:
            out["levels_tried"][str(candidate)] = {"capacity": str(e), "wall_s": round(time.perf_counter() - t0, 3)}
            continue
        out["levels_tried"][str(candidate)] = {"n_states": p.n_states, "complete": p.complete, "depth_reached": p.depth_reached, "horizon": p.horizon,
                                               "passes": p.passes, "root_steps": p.root_steps, "explore_ms": round(p.stats["explore_ms"], 3),
                                               "relax_ms": round(p.stats["relax_ms"], 3), "wall_s": round(time.perf_counter() - t0, 3)}
        if p.complete:
            pol, level = p, candidate
            break
        p.free()
    if pol is None:
        out["error"] = "no level explores completely"
        print(json.dumps(out), flush=True)
        return
    out["level"] = level
    n = args.envs
    bw = BatchedWorld(Map(level=level), n)
    one = BatchedWorld(Map(level=level), 1)
    for t in range(30):
        bw.step(sample=True, seed=7, t=t)
    start = bw.snapshot()
    steps_buf = torch.empty(n, dtype=torch.int32, device=bw.device)
    one_buf = torch.empty(1, dtype=torch.int32, device=bw.device)
    first = pol.steps_to_go(bw)
    out["after_30_sampled_steps"] = {"exact": int((first >= 0).sum()), "unknown": int((first == pol.UNKNOWN).sum()), "dead_end": int((first == pol.DEAD_END).sum()),
                                     "mean_steps_to_go": round(float(first[first >= 0].float().mean()), 3) if (first >= 0).any() else None}

    def plain_step(t):
        bw.step(sample=True, auto_reset=True, seed=7, t=t)

    def lookup(t):
        pol.steps_to_go(bw, check_map=False, out=steps_buf)

    def lookup_checked(t):
        pol.steps_to_go(bw, out=steps_buf)

    def act_and_step(t):
        pol.act(bw, check_map=False, out=steps_buf)
        bw.step(bw.actions, auto_reset=True)

    def empty_launch(t):
        pol.steps_to_go(one, check_map=False, out=one_buf)

    variants = {"plain_step": plain_step, "lookup": lookup, "lookup_with_map_check": lookup_checked, "act_and_step": act_and_step, "empty_launch": empty_launch}
    if args.variants:
        variants = {k: variants[k] for k in args.variants.split(",")}

    def run(name, steps):
        fn = variants[name]
        if name in ("plain_step", "lookup", "lookup_with_map_check"):
            bw.restore(start)  # (the lookups read the sampled states; the stepping loops start from them)
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
    out["us_per_call"] = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["all_rounds_us"] = {k: [round(x, 3) for x in v] for k, v in times.items()}
    u = out["us_per_call"]
    if "act_and_step" in u and "plain_step" in u:
        out["act_cost_us"] = round(u["act_and_step"] - u["plain_step"], 3)
    if "lookup" in u and "plain_step" in u:
        out["lookup_over_step"] = round(u["lookup"] / u["plain_step"], 3)
    from lle_amd import policy
    out["kernels"] = policy.launched_kernels()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--levels", default="5,4,3,2,1", help="built-in levels to try, in this order, until one explores completely")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default=None, help="comma-separated subset of plain_step,lookup,lookup_with_map_check,act_and_step,empty_launch (under a "
                    "profiler: `lookup` alone gives policy_lookup's time over the whole batch)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts, or a profiler wraps)")
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
