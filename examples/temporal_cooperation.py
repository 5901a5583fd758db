"""How deep was the cooperation in the episodes a policy just played?  BatchedLLE(cooperation="temporal") keeps, per environment, the
longest trail of help events in time order -- the temporal half of the reference's PlanProfile -- by one more small launch per step.
BatchedLLE(cooperation="closed-trails") also keeps which closed trails of help the episode holds: is_interdependent(n_agents)."""
import json
import os

import torch

from lle_amd import BatchedLLE, Map

env = BatchedLLE(Map(level=6), 16384, cooperation="temporal")
env.reset()
for t in range(300):
    avail = env.available_actions()
    actions = torch.rand(avail.shape, device=avail.device).masked_fill(~avail, -1.0).argmax(-1)  # a random available action per agent
    env.step(actions, auto_reset=True)
tracker = env.cooperation
finished = tracker.last_tprofile[:, 3] > 0                       # an episode has finished in the environment
n = max(int(finished.sum()), 1)
print("finished episodes:", int(finished.sum()))
print("  cooperative      :", f"{int((tracker.is_cooperative(last=True) & finished).sum()) / n:.4f}")
print("  is_sequential(2) :", f"{int(tracker.is_sequential(2, last=True).sum()) / n:.4f}")
print("  is_mutual        :", f"{int((tracker.is_mutual(last=True) & finished).sum()) / n:.4f}")
print("  longest trail    :", int(tracker.longest_trail(last=True).max()), "| exact:", bool(tracker.trails_exact(last=True).all()))

# Did THIS episode close a chain of help over three agents?  cooperation="closed-trails" keeps, per environment, the set of (anchor,
# current, support) triples of the episode's help trails by one more small launch, and answers is_interdependent(n_agents) for 2..6.
# Random play never closes such a trail, so half of the environments replay a shortest plan of `paper-interdependent-3` (in it agent 0
# helps 1, then 1 helps 2, then 2 helps 0; no plan of that world avoids such a closed trail) and the other half stays put.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
catalogue = json.load(open(os.path.join(ROOT, "tests", "golden", "kat_trails.json")))["catalogue"]
text = {c["name"]: c["map"] for c in catalogue if "map" in c}["paper-interdependent-3"]
plan = [[1, 1, 4], [1, 1, 4], [1, 4, 4], [1, 4, 0], [1, 4, 3], [2, 1, 0], [2, 4, 0]]  # joint actions, one row per step (4 = stay)
env = BatchedLLE(Map(text), 1024, cooperation="closed-trails")
env.reset()
scripted = torch.arange(1024, device=env.world.device) % 2 == 0
for row in plan:
    actions = torch.full((1024, 3), 4, dtype=torch.uint8, device=env.world.device)
    actions[scripted] = torch.tensor(row, dtype=torch.uint8, device=env.world.device)
    out = env.step(actions, auto_reset=False)
tracker = env.cooperation
print("paper-interdependent-3, 512 scripted and 512 idle episodes:")
print("  is_interdependent(3), scripted:", int(tracker.is_interdependent(3)[scripted].sum()), "| idle:", int(tracker.is_interdependent(3)[~scripted].sum()))
print("  is_interdependent(2), scripted:", int(tracker.is_interdependent(2)[scripted].sum()), "| exact:", bool(tracker.closed_exact().all()))
print("  triples of environment 0      :", sorted((a, c, sorted(s)) for a, c, s in tracker.triples(0)))
