"""Expert rollouts from random mid-episode states: build the steps-to-go table of a map once, scatter a batch with sampled steps, then
let `OptimalPolicy.act` write an optimal joint action into every environment's action buffer before each step, until every
environment that can still be solved is solved.  GPU box.

    python examples/expert_rollout.py [--level 3] [--envs 4096] [--sampled-steps 12] [--seed 1]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sampled-steps", type=int, default=12)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch

    from lle_amd import BatchedWorld, Map, OptimalPolicy

    pol = OptimalPolicy(Map(level=args.level))
    print(f"level {args.level}: {pol.n_states} states, {'complete' if pol.complete else 'cut at the horizon'} after {pol.depth_reached} levels, "
          f"{pol.passes} relaxation passes, {pol.root_steps} steps from the reset state "
          f"(explore {pol.stats['explore_ms']:.1f} ms, relax {pol.stats['relax_ms']:.1f} ms)")
    env = BatchedWorld(Map(level=args.level), args.envs)
    for t in range(args.sampled_steps):  # random walks, no auto-reset: some environments lose an agent on the way
        env.step(sample=True, seed=args.seed, t=t, write_obs=False)
    steps = pol.steps_to_go(env)
    solvable, dead, unknown = steps >= 0, steps == pol.DEAD_END, steps == pol.UNKNOWN
    print(f"after {args.sampled_steps} sampled steps: {int(solvable.sum())} solvable (mean {float(steps[solvable].float().mean()):.2f} steps to go, "
          f"max {int(steps[solvable].max())}), {int(dead.sum())} dead ends, {int(unknown.sum())} unknown")
    n_agents = env.map.n_agents
    arrived_bits = 16 + torch.arange(n_agents, device=env.device)
    rounds = 0
    while True:
        left = pol.act(env)  # the expert's actions land in env.actions; STAY where nothing is known or nothing can be done
        if not (left > 0).any().item():
            break
        env.step(env.actions, write_obs=False)
        rounds += 1
    arrived = (((env.bits.unsqueeze(1) >> arrived_bits) & 1) == 1).all(1)
    assert bool(arrived[solvable].all()) and not bool(arrived[dead].any()), "every solvable environment ends with everybody on an exit, no dead end does"
    print(f"{int(arrived.sum())} environments solved in {rounds} expert steps; the longest needed {int(steps[solvable].max())}")


if __name__ == "__main__":
    main()
