"""Expert rollouts over a curriculum of generated worlds: `generate_n` keeps a handful of solvable worlds, ONE `PolicyForest` builds the
steps-to-go table of every world in the same launches, a batch that holds all the worlds is scattered with sampled steps, and
`PolicyForest.act` writes an optimal joint action into every environment's action buffer before each step -- one lookup launch for the
whole batch -- until every environment that has an answer is solved.  GPU box.

    python examples/expert_curriculum.py [--worlds 8] [--envs-per-world 512] [--horizon 12] [--sampled-steps 6] [--seed 1]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--envs-per-world", type=int, default=512)
    ap.add_argument("--horizon", type=int, default=12)
    ap.add_argument("--sampled-steps", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    from lle_amd import BatchedWorld, Constraint, PolicyForest, Solvable, generate_n

    keep = Constraint(t_max=args.horizon, predicate=Solvable(), min_solution_length=4)
    worlds = list(generate_n(args.worlds, keep, height=5, width=5, n_agents=2, n_lasers=2, n_gems=1, n_exits=2, wall_fraction=0.12, seed=0, batch=128,
                             max_attempts=2048))
    print(f"{len(worlds)} solvable 5x5 worlds whose shortest plan has at least 4 steps")
    maps = [w.world_string for w in worlds]

    pf = PolicyForest(worlds, args.horizon)
    for m in range(pf.n_maps):
        print(f"world {m}: {int(pf.n_states[m])} states, {'complete' if pf.complete[m] else 'cut at the horizon'} after {int(pf.depth_reached[m])} levels, "
              f"{int(pf.passes[m])} relaxation passes, {int(pf.root_steps[m])} steps from the reset state")
    print(f"explore {pf.explore_ms:.1f} ms at occupancy {pf.occupancy['explore']:.2f}, relax {pf.relax_ms:.1f} ms at occupancy {pf.occupancy['relax']:.2f}")

    env = BatchedWorld(maps, len(maps) * args.envs_per_world)  # world m owns the environments [m * E, (m + 1) * E)
    for t in range(args.sampled_steps):  # random walks, no auto-reset: some environments lose an agent on the way
        env.step(sample=True, seed=args.seed, t=t, write_obs=False)
    steps = pf.steps_to_go(env)
    answered, dead, unknown = steps >= 0, steps == pf.DEAD_END, steps == pf.UNKNOWN
    print(f"after {args.sampled_steps} sampled steps: {int(answered.sum())} environments with an answer (mean {float(steps[answered].float().mean()):.2f} steps to "
          f"go, max {int(steps[answered].max())}), {int(dead.sum())} dead ends, {int(unknown.sum())} unknown (beyond the horizon)")
    arrived_bits = 16 + torch.arange(env.map.n_agents, device=env.device)
    rounds = 0
    while True:
        left = pf.act(env)  # the experts' actions land in env.actions; STAY where nothing is known or nothing can be done
        if not (left > 0).any().item():
            break
        env.step(env.actions, write_obs=False)
        rounds += 1
    arrived = (((env.bits.unsqueeze(1) >> arrived_bits) & 1) == 1).all(1)
    assert bool(arrived[answered].all()) and not bool(arrived[dead].any()), "every environment with an answer ends with everybody on an exit, no dead end does"
    assert rounds == int(steps[answered].max())
    print(f"{int(arrived.sum())} environments solved in {rounds} expert steps")


if __name__ == "__main__":
    main()
