"""What the temporal cooperation tracker costs per step: 65 536 environments, HIP events, one process, four BatchedLLE side by side and
timed in alternation --
  (a) plain         the default step, no tracker;
  (b) tracked       cooperation=True (one more small launch: the coop kernel);
  (c) temporal      cooperation="temporal" (two more small launches: the coop kernel, then the cooptrails kernel);
  (d) tracked_two   cooperation=True with fused=False (the coop kernel and one more small launch of the project's own,
                    lle_batch_env_outputs): the yardstick of profiles/r08_coop.md, measured again here.
The figure of interest is (c) - (b) against (d) - (b).  Nobody promised a figure.

--map level6 (default): uniform random actions (eight pre-drawn tensors), auto-reset: almost no state has an edge, every group takes
the fast path.  --map ring: the eight-agent ring of tests/golden/kat_coop.json, everybody stays: every state holds the eight ring
edges and every group enters the walk with saturated fields -- the divergence cost.  Prints one JSON line.  GPU box.

    python tools/bench_cooptrails.py [--map level6|ring] [--envs 65536] [--steps 1000] [--warmup 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_cooptrails.py --child --only temporal --rounds 1   (the kernel's own time)

The measurement runs in a child process under a time limit (--timeout seconds): a hang ends there."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["plain", "tracked", "temporal", "tracked_two"]


def measure(args):
    import torch

    from lle_amd import BatchedLLE, Map

    n = args.envs
    if args.map == "ring":
        cases = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_coop.json")))["worlds"]
        text = {c["name"]: c["map"] for c in cases}["eight-agent-interdependent-8"]
        make_map = lambda: Map(text)  # noqa: E731
    else:
        make_map = lambda: Map(level=6)  # noqa: E731
    coop = {"plain": False, "tracked": True, "temporal": "temporal", "tracked_two": True}
    names = [args.only] if args.only else NAMES
    envs = {k: BatchedLLE(make_map(), n, seed=1, cooperation=coop[k]) for k in names}
    A = next(iter(envs.values())).n_agents
    g = torch.Generator(device="cuda").manual_seed(0)
    if args.map == "ring":
        actions = [torch.full((n, A), 4, device="cuda", dtype=torch.uint8) for _ in range(8)]  # STAY
    else:
        actions = [torch.randint(0, 5, (n, A), generator=g, device="cuda", dtype=torch.uint8) for _ in range(8)]
    kw = {k: (dict(fused=False) if k == "tracked_two" else {}) for k in NAMES}

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
        for name in names:  # alternating: drifts of the box hit all alike
            times[name].append(run(name, args.steps))
    out = {"map": args.map, "envs": n, "agents": A, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "us_per_step": {k: round(statistics.median(v), 3) for k, v in times.items()}, "all_rounds_us": {k: [round(x, 3) for x in v] for k, v in times.items()}}
    if not args.only:
        u = out["us_per_step"]
        out["coop_cost_us"] = round(u["tracked"] - u["plain"], 3)
        out["trails_cost_us"] = round(u["temporal"] - u["tracked"], 3)
        out["one_more_small_launch_us"] = round(u["tracked_two"] - u["tracked"], 3)
    env = envs.get("temporal")
    if env is not None:
        # per environment and step: A rows of this state's edges (4 B each), the auto-reset and the refusal byte read; the trail value and
        # its profile read and written.  An environment that was reset also writes the last episode's value and profile.
        out["trails_bytes_per_env"] = 4 * A + 2 + 2 * 8 + 2 * 4
        out["trails_bytes_per_reset_env_extra"] = 8 + 4
        from lle_amd import cooptrails
        out["kernels"] = cooptrails.launched_kernels()
        tr = env.cooperation
        torch.cuda.synchronize()
        out["states_with_an_edge_now"] = int((tr.step_edges != 0).any(dim=1).sum())
        out["sequential_2_running"] = int(tr.is_sequential(2).sum())
        out["finished_once"] = int((tr.last_tprofile[:, 3] > 0).sum())
        out["sequential_2_last"] = int(tr.is_sequential(2, last=True).sum())
        out["saturated_running"] = int((tr.longest_trail() == 15).sum())
        out["dense_running"] = int((~tr.trails_exact()).sum())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", choices=["level6", "ring"], default="level6")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=NAMES, default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts, or a profiler wraps)")
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
