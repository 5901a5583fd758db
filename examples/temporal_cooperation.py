"""How deep was the cooperation in the episodes a policy just played?  BatchedLLE(cooperation="temporal") keeps, per environment, the
longest trail of help events in time order -- the temporal half of the reference's PlanProfile -- by one more small launch per step."""
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
