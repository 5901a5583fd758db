"""Two builds of liblle_hip.so against each other on one box: alternating A / B child processes (LLE_HIP_LIB is read once per process),
each timing the same workloads launch-to-launch over HIP events, in the process layout of tools/incremental_ab.py.  GPU box.

    python3 tools/lib_ab.py --a <parent's liblle_hip.so> --b lle_amd/liblle_hip.so [--pairs 5] [--side]

Prints every figure, per side the median and the spread (max - min over the pairs), and the median difference B - A.  --side adds
level 1 x 4 096, level 6 x 262 144, config 5 x 65 536 and BatchedLLE.step in one launch with and without randomize_lasers."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(side):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import torch
    from lle_prof import timeit

    from lle_amd import BatchedLLE, BatchedWorld, Map, mapgen
    out = {}

    def world(label, m, n, fill=False):
        bw = BatchedWorld(m, n)
        step = bw.sampled_stepper(seed=1)
        out[label] = statistics.median(timeit(step, iters=200, warm=20) for _ in range(5))
        if fill:
            probe = bw.row_fill_prober()
            out[label + " row fill"] = statistics.median(timeit(probe, iters=200, warm=20) for _ in range(5))
            bw.observe()
        t = bw.tuning()
        out[label + " rules"] = {k: t[k] for k in ("envs_per_wave", "row_heads", "write_through", "head_group", "rotate_rows")}
        del bw, step
        torch.cuda.empty_cache()

    world("level 6 x 65536", Map(level=6), 65536, fill=True)
    if side:
        world("level 1 x 4096", Map(level=1), 4096)
        world("level 6 x 262144", Map(level=6), 262144)
        world("config 5 x 65536", Map(mapgen.config5(0)), 65536)
        for label, kw in (("LLE.step one launch", dict()), ("LLE.step one launch randomize_lasers", dict(randomize_lasers=True))):
            env = BatchedLLE(Map(level=6), 65536, **kw)
            env.reset()
            acts = torch.full((65536, env.n_agents), 4, dtype=torch.uint8, device=env.world.device)
            out[label] = statistics.median(timeit(lambda: env.step(acts, auto_reset=True, fused=True), iters=200, warm=20) for _ in range(3))
            del env
            torch.cuda.empty_cache()
    print("AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--side", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.side)
    runs = {"A": [], "B": []}
    for pair in range(args.pairs):
        for name, lib in (("A", args.a), ("B", args.b)):
            env = dict(os.environ, LLE_HIP_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + (["--side"] if args.side else []), env=env, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:  # a fault, an abort or a crash: nothing more is started on the GPU
                print(p.stderr[-2000:])
                print(f"pair {pair} side {name}: exit status {p.returncode}; stopping", flush=True)
                return p.returncode
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("AB ")][-1]
            runs[name].append(json.loads(line[3:]))
            print(f"pair {pair} {name}: " + "  ".join(f"{k} {v:.2f}" for k, v in runs[name][-1].items() if not isinstance(v, dict)), flush=True)
    print("rules A:", {k: v for k, v in runs["A"][-1].items() if isinstance(v, dict)})
    print("rules B:", {k: v for k, v in runs["B"][-1].items() if isinstance(v, dict)})
    print("| workload | A median | A spread | B median | B spread | median of B - A | 3 x larger spread |")
    print("|---|---|---|---|---|---|---|")
    for k, v in runs["A"][0].items():
        if isinstance(v, dict):
            continue
        a, b = [r[k] for r in runs["A"]], [r[k] for r in runs["B"]]
        d = statistics.median(y - x for x, y in zip(a, b))
        sa, sb = max(a) - min(a), max(b) - min(b)
        print(f"| {k} | {statistics.median(a):.2f} | {sa:.2f} | {statistics.median(b):.2f} | {sb:.2f} | {d:+.2f} | {3 * max(sa, sb):.2f} |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
