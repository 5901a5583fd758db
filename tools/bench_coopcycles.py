"""What the closed-trail cooperation tracker costs per step: 65 536 environments, HIP events, one process, everything in the SAME run --
  the step, four BatchedLLE side by side and timed in alternation
    (a) tracked       cooperation=True (the coop kernel behind the step);
    (b) temporal      cooperation="temporal" (the coop kernel, then the cooptrails kernel);
    (c) closed        cooperation="closed-trails" (the coop kernel, the cooptrails kernel, then the coopcycles kernel);
    (d) tracked_two   cooperation=True with fused=False (the coop kernel and one more small launch of the project's own,
                      lle_batch_env_outputs): the yardstick of profiles/r08_coop.md, measured again here;
  the launches ALONE on the closed-trails environment, as the last step left its rows (almost no state has an arc)
    trails_alone      lle_cooptrails_update(MARK_POS)
    closed_alone      lle_coopcycles_update(MARK_POS)
  and the made-up worst case: a ring over all agents written into every environment's rows, so that every state of every
  environment enters the walk
    closed_ring_fresh lle_coopcycles_update(CLEAR | MARK_POS): the walk from the empty value
    closed_ring_held  lle_coopcycles_update(MARK_POS): the walk from the value the ring has filled
    trails_ring_held  lle_cooptrails_update(MARK_POS) on the same rows.
The figures of interest are (c) - (b) against (d) - (a) and closed_alone against trails_alone: the bytes of the no-arc path are no more,
hence the expectation of the same time.  Every figure is the median of --rounds rounds; all rounds are printed, they are the run's own spread.  Nobody
promised a figure.

--map level6 (default; 4 agents: coopcycles_kernel<3>), --map line6 (six agents on one beam: coopcycles_kernel<21>, every reset state
has five arcs).  Prints one JSON line.  GPU box.

    python tools/bench_coopcycles.py [--map level6|line6] [--envs 65536] [--steps 1000] [--warmup 50] [--rounds 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_coopcycles.py --child --only closed --skip-worst --rounds 1   (the kernel's own time)

The measurement runs in a child process under a time limit (--timeout seconds): a hang ends there."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ["tracked", "temporal", "closed", "tracked_two"]
LINE6 = "L0E S0 S1 S2 S3 S4 S5 @\nX X X X X X . ."


def measure(args):
    import torch

    from lle_amd import BatchedLLE, Map, coopcycles, cooptrails

    n = args.envs
    make_map = (lambda: Map(LINE6)) if args.map == "line6" else (lambda: Map(level=6))  # noqa: E731
    coop = {"tracked": True, "temporal": "temporal", "closed": "closed-trails", "tracked_two": True}
    names = [args.only] if args.only else NAMES
    envs = {k: BatchedLLE(make_map(), n, seed=1, cooperation=coop[k]) for k in names}
    A = next(iter(envs.values())).n_agents
    g = torch.Generator(device="cuda").manual_seed(0)
    actions = [torch.randint(0, 5, (n, A), generator=g, device="cuda", dtype=torch.uint8) for _ in range(8)]
    kw = {k: (dict(fused=False) if k == "tracked_two" else {}) for k in NAMES}

    def timed(fn, repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in range(repeats):
            fn(t)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / repeats  # us per call

    def run(name, steps):
        env, k = envs[name], kw[name]
        return timed(lambda t: env.step(actions[t & 7], auto_reset=True, **k), steps)

    for name in names:
        envs[name].reset()
        run(name, args.warmup)
    times = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:  # alternating: drifts of the box hit all alike
            times[name].append(run(name, args.steps))
    out = {"map": args.map, "envs": n, "agents": A, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    env = envs.get("closed")
    if env is not None:
        tr = env.cooperation
        W = tr.n_words
        torch.cuda.synchronize()
        out["states_with_an_arc_now"] = int((tr.step_edges != 0).any(dim=1).sum())
        out["interdependent_2_running"] = int(tr.is_interdependent(2).sum())
        out["interdependent_3_running"] = int(tr.is_interdependent(3).sum())
        out["finished_once"] = int((tr.last_cprofile[:, 3] > 0).sum())
        out["dense_running"] = int((~tr.closed_exact()).sum())
        mark = coopcycles.LLE_COOPCYCLES_MARK_POS
        alone = {"trails_alone": lambda t: tr.launch_trails(tr.make_trails_args(mark)),
                 "closed_alone": lambda t: tr.launch_closed(tr.make_closed_args(mark))}
        ring = torch.tensor([1 << ((a + 1) % A) for a in range(A)], dtype=torch.int32, device="cuda").repeat(n, 1)
        worst = {"closed_ring_fresh": lambda t: tr.launch_closed(tr.make_closed_args(coopcycles.LLE_COOPCYCLES_CLEAR | mark)),
                 "closed_ring_held": lambda t: tr.launch_closed(tr.make_closed_args(mark)),
                 "trails_ring_held": lambda t: tr.launch_trails(tr.make_trails_args(mark))}
        for k in list(alone) + ([] if args.skip_worst else list(worst)):
            times[k] = []
        for _ in range(args.rounds):
            for k, fn in alone.items():
                timed(fn, 20)
                times[k].append(timed(fn, args.steps))
        if not args.skip_worst:
            tr.step_edges.copy_(ring)
        for _ in range(0 if args.skip_worst else args.rounds):
            for k, fn in worst.items():
                timed(fn, 20)
                times[k].append(timed(fn, args.steps))
        torch.cuda.synchronize()
        out["ring_closed_orders"] = sorted({int(b) for b in tr.closed_orders().unique().cpu().tolist()})
        out["ring_dense"] = int((~tr.closed_exact()).sum())
        # per environment and step on the no-arc path: A rows of this state's edges (4 B each), the auto-reset and the refusal byte and the
        # profile word read; nothing written once the row is valid.  A state with an arc reads and writes the W value words and writes
        # the profile; an environment that was reset writes the last episode's W words and profile and the running episode's W words.
        out["closed_bytes_per_env_no_arc"] = 4 * A + 2 + 4
        out["closed_bytes_per_env_with_an_arc_extra"] = 2 * 4 * W + 4
        out["closed_bytes_per_reset_env_extra"] = 3 * 4 * W + 4 + 4
        out["trails_bytes_per_env"] = 4 * A + 2 + 2 * 8 + 2 * 4
        out["kernels"] = coopcycles.launched_kernels() + cooptrails.launched_kernels()
    out["us"] = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out["all_rounds_us"] = {k: [round(x, 3) for x in v] for k, v in times.items()}
    if not args.only:
        u = out["us"]
        out["trails_cost_us"] = round(u["temporal"] - u["tracked"], 3)
        out["closed_cost_us"] = round(u["closed"] - u["temporal"], 3)
        out["one_more_small_launch_us"] = round(u["tracked_two"] - u["tracked"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", choices=["level6", "line6"], default="level6")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=NAMES, default=None)
    ap.add_argument("--skip-worst", action="store_true", help="leave the ring rows out (under a profiler: the kernel's time on the no-arc path alone)")
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts, or a profiler wraps)")
    args = ap.parse_args()
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
