"""BatchedLLE(cooperation="closed-trails") -- the coop kernel, the cooptrails kernel and behind them the coopcycles kernel,
lle_amd/coopcycles/coopcycles.hip -- in differential rollouts: the coop arrays against tests/coop_ref.py, the trail arrays against
tests/cooptrails_ref.py, the closed-trail arrays against the restatement from the definition of a trail (tests/coopcycles_ref.py over
tests/cycles_ref.layer_update), EVERY buffer of the tracker compared exactly (torch.equal) after every step.

The driver is tests/coopcycles_play.play: random play never closes a trail of order 3 or more, so every second environment replays,
from each reset, the shortest plan of its map, which closes a trail over all its agents.  Every rollout asserts its coverage from the
restatement ALONE; the minimum is the count that the oracle-only run (gpu=False) of the very same arguments gives
(coopcycles_play.ROLLOUTS, asserted without a GPU by tests/test_coopcycles_cpu.py) and is written in the docstring."""
import os
import subprocess
import sys

import pytest

from tests import coopcycles_play
from tests.coopcycles_play import ROLLOUTS, play

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_PATHS = {"default": {}, "fused": dict(fused=True), "two_launches": dict(fused=False), "persistent": dict(persistent=True)}


def rollout(oracle_mod, name, **more):
    """play with the arguments of ROLLOUTS[name]; the coverage is at least the oracle-only run's."""
    kwargs, least = ROLLOUTS[name]
    cover = play(oracle_mod, **kwargs, **more)
    assert all(cover[k] >= least[k] for k in least), (cover, least)
    return cover


@pytest.mark.parametrize("path", sorted(STEP_PATHS))
def test_every_step_path(oracle_mod, path):
    """paper-interdependent-3, 16 x 30, seed 81, a tenth of the steps refused: 24 finished episodes with order 3 in last_cprofile,
    26 environment-steps whose running episode holds order 3, 28 refused steps inside a scripted episode, 149 states with an arc."""
    cover = rollout(oracle_mod, "paths", step_kw=STEP_PATHS[path])
    assert cover["finished_top"] >= 24 and cover["running_top"] >= 26 and cover["refused_scripted"] >= 28, cover


@pytest.mark.parametrize("reset_by", ["auto", "mask", "none"])
def test_every_way_of_resetting(oracle_mod, reset_by):
    """three-agent-temporal-cycle, 64 x 60, seed 82, a tenth of the steps refused.  auto and mask: 174 finished episodes with order 3,
    386 environment-steps with order 3 running, 209 with order 2 only, 190 refused steps inside a scripted episode.  none: no episode
    finishes, 1 670 environment-steps with order 3 running (the value stays), 34 with order 2 only, 32 refused inside a plan."""
    cover = rollout(oracle_mod, "resets_" + reset_by)
    if reset_by == "none":
        assert cover["running_top"] >= 1670 and cover["order2_only"] >= 34 and cover["refused_scripted"] >= 32, cover
    else:
        assert cover["finished_top"] >= 174 and cover["running_top"] >= 386 and cover["order2_only"] >= 209 and cover["refused_scripted"] >= 190, cover


def test_four_agents(oracle_mod):
    """four-agent-interdependent-4-sequence-6, 64 x 60, seed 83, a twentieth of the steps refused: 114 finished episodes with order 4
    (their plan closes 2, 3 and 4), 381 environment-steps with order 4 running, 1 388 with order 2 only, 108 refused inside a plan."""
    cover = rollout(oracle_mod, "four")
    assert cover["finished_top"] >= 114 and cover["running_top"] >= 381 and cover["order2_only"] >= 1388 and cover["refused_scripted"] >= 108, cover


def test_two_maps(oracle_mod):
    """paper-interdependent-3 and the same with one wall opened, 2 x 32, 40 steps, seed 84: 160 finished episodes with order 3."""
    cover = rollout(oracle_mod, "two_maps")
    assert cover["finished_top"] >= 160 and cover["running_top"] >= 160, cover


def test_set_state_mid_episode(oracle_mod):
    """paper-interdependent-3, 16 x 20, seed 85, every environment handed its own state after step 8 (one more state of the episode):
    16 finished episodes with order 3."""
    cover = rollout(oracle_mod, "set_state")
    assert cover["finished_top"] >= 16 and cover["running_top"] >= 16, cover


def test_reset_chains_two_layers(oracle_mod):
    """Three agents that start on one beam (the reset state has two arcs), 32 x 30 at random, seed 87: 80 updates in which the step
    kernel's reset chains the start layer and the state's layer in one launch."""
    cover = rollout(oracle_mod, "chain")
    assert cover["chained"] >= 80, cover


def test_randomize_lasers(oracle_mod):
    """Level 6, 64 x 60 at random, seed 67 (no plan: the colours are drawn on the device, so the coverage cannot be counted on the
    oracle alone); some environment-steps have an edge (the seeds 67 to 70 showed 9, 3, 4 and 4 on an MI355X)."""
    from oracle.levels import LEVELS
    cover = play(oracle_mod, [LEVELS[6]], 64, 60, 67, scripted=False, randomize=True)
    assert cover["edges"] >= 1, cover


def test_the_three_trackers():
    import lle_amd
    from lle_amd.coopcycles import ClosedTrailCooperationTracker
    from lle_amd.cooptrails import TemporalCooperationTracker
    closed = lle_amd.level(6).build(8, cooperation="closed-trails")
    assert type(closed.cooperation) is ClosedTrailCooperationTracker and closed.cooperation.episode_closed.shape == (3, 8)
    assert bool(closed.cooperation.episode_cprofile[:, 3].all()) and not bool(closed.cooperation.is_interdependent(2).any())
    temporal = lle_amd.level(6).build(8, cooperation="temporal")
    assert type(temporal.cooperation) is TemporalCooperationTracker and not hasattr(temporal.cooperation, "episode_closed")
    with pytest.raises(NotImplementedError):
        temporal.cooperation.is_interdependent(3)
    for bad in ("flattened", "closed", "closed_trails"):
        with pytest.raises(ValueError, match="temporal.*closed-trails"):
            lle_amd.level(6).build(8, cooperation=bad)
    from tests.test_gpu_coop import line_map
    with pytest.raises(ValueError, match="at most 6 agents"):
        lle_amd.BatchedLLE(line_map(7), 8, cooperation="closed-trails")
    assert lle_amd.BatchedLLE(line_map(7), 8, cooperation="temporal").cooperation.n_agents == 7


@pytest.mark.parametrize("cooperation", ["True", "'temporal'"])
def test_the_other_trackers_do_not_load_the_library(cooperation):
    """cooperation=True and cooperation="temporal" in a fresh interpreter never load liblle_coopcycles.so."""
    code = ("import sys, torch, lle_amd\n"
            f"env = lle_amd.level(6).build(64, cooperation={cooperation})\n"
            "env.reset()\n"
            "env.step(torch.full((64, env.n_agents), 4, dtype=torch.uint8, device='cuda'), auto_reset=True)\n"
            "assert 'lle_amd.coopcycles' not in sys.modules\n"
            "assert 'liblle_coopcycles' not in open('/proc/self/maps').read() and 'liblle_coop.so' in open('/proc/self/maps').read()\n"
            "print('untouched')\n")
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0 and "untouched" in res.stdout, res.stdout + res.stderr


def test_every_compiled_kernel_is_launched(oracle_mod):
    """Last in the module: three and four agents (3 words) ran above; one short rollout with 5 agents and one with 6 (21 words)
    against the restatement; then each coopcycles_kernel<W> must be named by lle_coopcycles_debug_launched."""
    from lle_amd import coopcycles
    from tests.test_gpu_coop import line_map
    for n_agents in (5, 6):
        cover = play(oracle_mod, [line_map(n_agents)], 16, 10, 70 + n_agents, scripted=False)
        assert cover["edges"] >= 16, cover
    missing = sorted(set(coopcycles.compiled_kernels()) - set(coopcycles.launched_kernels()))
    assert not missing, f"compiled but never launched: {missing}"
    assert coopcycles.compiled_kernels() == ["coopcycles_kernel<3>", "coopcycles_kernel<21>"] and coopcycles_play.CLOSED_NAMES[0] == "episode_closed"
