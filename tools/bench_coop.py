"""What the cooperation tracker costs per step: level 6 x 65 536 environments, HIP events, one process, three BatchedLLE side by side
and timed in alternation --
  (a) the default step, no tracker;
  (b) the same with cooperation=True (one more small launch: the coop kernel);
  (c) the untracked step with fused=False (one more small launch: lle_batch_env_outputs), for comparison: what the project already
      pays for one more small launch.
Nobody promised a figure for (b) - (a): the tool reports it next to (c) - (a) of the same run and the bytes the launch moves.
Prints one JSON line.  GPU box.

    python tools/bench_coop.py [--envs 65536] [--steps 1000] [--warmup 50] [--rounds 5]
    python tools/bench_coop.py --only plain          (the same step loop alone: also runs on a checkout without the tracker)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_coop.py --child --only tracked --rounds 1   (the kernel's own time)

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

    from lle_amd import BatchedLLE, Map

    n = args.envs
    mk = {"plain": lambda: BatchedLLE(Map(level=6), n, seed=1),
          "tracked": lambda: BatchedLLE(Map(level=6), n, seed=1, cooperation=True),
          "two_launches": lambda: BatchedLLE(Map(level=6), n, seed=1)}
    names = [args.only] if args.only else ["plain", "tracked", "two_launches"]
    envs = {k: mk[k]() for k in names}
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = [torch.randint(0, 5, (n, 4), generator=g, device="cuda", dtype=torch.uint8) for _ in range(8)]
    kw = {"plain": {}, "tracked": {}, "two_launches": dict(fused=False)}

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
        a, b, c = (out["us_per_step"][k] for k in ("plain", "tracked", "two_launches"))
        out["coop_cost_us"], out["second_small_launch_us"] = round(b - a, 3), round(c - a, 3)
    env = envs.get("tracked")
    if env is not None:
        A = env.n_agents
        # per environment and step: positions, state bits and the auto-reset flag read; the episode's edges and profile read and written;
        # this state's edges written.  An environment that was reset also writes the last episode's edges and profile.
        out["coop_bytes_per_env"] = int(env.world.pos.stride(0)) + 8 + 1 + 2 * 4 * A + 2 * 8 + 4 * A
        out["coop_bytes_per_reset_env_extra"] = 4 * A + 8
        from lle_amd import cooperation
        out["kernels"] = cooperation.launched_kernels()
        tr = env.cooperation
        torch.cuda.synchronize()
        out["cooperative_running"] = int(tr.is_cooperative().sum())
        out["cooperative_last"] = int(tr.is_cooperative(last=True).sum())
        out["finished_once"] = int((tr.last_profile[:, 7] > 0).sum())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["plain", "tracked", "two_launches"], default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts, or a profiler wraps)")
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
