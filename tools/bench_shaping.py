"""What reward shaping costs per step: level 6 x 65 536 environments, HIP events, one process, three BatchedLLE side by side and timed in
alternation --
  (a) the default step, unshaped;
  (b) the same with PotentialShapedLLE + LaserSubgoal extras (one more small launch: the shaping kernel);
  (c) the unshaped step with fused=False (one more small launch: lle_batch_env_outputs).
The yardstick for (b) - (a) is (c) - (a) of the same run: what the project already pays for one more small launch.  Expected:
(b) - (a) <= 1.25 x ((c) - (a)).  Prints one JSON line.  GPU box.

    python tools/bench_shaping.py [--envs 65536] [--steps 1000] [--warmup 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_shaping.py --child --only shaped --rounds 1   (the kernel's own time)

The measurement runs in a child process under a time limit (--timeout seconds): a hang ends there."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import torch

    from lle_amd import BatchedLLE, LaserSubgoal, Map, PotentialShapedLLE, SingleObjective

    n = args.envs
    mk = {"plain": lambda: BatchedLLE(Map(level=6), n, seed=1),
          "shaped": lambda: BatchedLLE(Map(level=6), n, seed=1, reward_strategy=PotentialShapedLLE(SingleObjective()), extras_generator=LaserSubgoal()),
          "two_launches": lambda: BatchedLLE(Map(level=6), n, seed=1)}
    names = [args.only] if args.only else ["plain", "shaped", "two_launches"]
    envs = {k: mk[k]() for k in names}
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = [torch.randint(0, 5, (n, 4), generator=g, device="cuda", dtype=torch.uint8) for _ in range(8)]
    kw = {"plain": {}, "shaped": {}, "two_launches": dict(fused=False)}

    def run(name, steps):
        env, k = envs[name], kw[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(steps):
            env.step(actions[t & 7], auto_reset=True, **k)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps  # us per step

    for name in names:
        envs[name].reset()
        run(name, args.warmup)
    times = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:  # alternating: drifts of the box hit all three alike
            times[name].append(run(name, args.steps))
    out = {"envs": n, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "us_per_step": {k: round(statistics.median(v), 3) for k, v in times.items()}, "all_rounds_us": {k: [round(x, 3) for x in v] for k, v in times.items()}}
    if not args.only:
        a, b, c = (out["us_per_step"][k] for k in ("plain", "shaped", "two_launches"))
        out["shaping_cost_us"], out["yardstick_us"] = round(b - a, 3), round(c - a, 3)
        out["within_bound"] = bool(b - a <= 1.25 * (c - a))
    env = envs.get("shaped")
    if env is not None:
        A, E = env.n_agents, env.extras_shape[0]
        # per environment and step: positions and the auto-reset flag read, both reached arrays read and written, base reward read, shaped
        # reward and extras written
        out["shaping_bytes_per_env"] = int(env.world.pos.stride(0)) + 1 + 2 * 2 * 4 * A + 4 + 4 + 4 * A * E
        from lle_amd import shaping
        out["kernels"] = shaping.launched_kernels()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["plain", "shaped", "two_launches"], default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts, or a profiler wraps)")
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
