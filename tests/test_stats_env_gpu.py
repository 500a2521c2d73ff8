"""Episode statistics on the real envs' step outputs: BatchedEnv att (combined radar) and wgru at
E = 64, N = 3, BatchedUAM at E = 32, N = 4, seeded random actions, auto-reset from the bank.  Every
step's outputs are downloaded and fed to the numpy restatement (tests/stats_ref.py); totals, running
state and log must match (integers and the running return exact, the sums within the bound).

Each env runs with its default episode_length through the fused step tail (att / wgru; UAM: step +
auto-reset) and with episode_length = 4 through the separate launches.  Both runs must end episodes by
a crash and by the step limit (asserted, seeds fixed below): full-scale random accelerations crash
agents into the bound, a building or each other within a few steps; the envs flown at 2 % of them
wander around their starts past the limit."""
import numpy as np
import pytest
import torch

import stats_ref

pytestmark = pytest.mark.gpu

#         kind    E   N  episode_length  steps  action seed
RUNS = [("att", 64, 3, None, 60, 1), ("att", 64, 3, 4, 16, 2),
        ("wgru", 64, 3, None, 160, 3), ("wgru", 64, 3, 4, 16, 4),
        ("uam", 32, 4, None, 160, 5), ("uam", 32, 4, 4, 16, 6)]


def _make_env(kind, E, N, ep, occ):
    from multi_agent_aac_amd import uam, world
    from multi_agent_aac_amd.env import BatchedEnv
    if kind == "uam":
        env = uam.BatchedUAM(E, N, **({} if ep is None else {"episode_length": ep}))
        env.set_bank(uam.build_bank(2048, N, seed=7), seed=11)
        return env
    env = BatchedEnv(E, N, occ, radar_mode="combined" if kind == "att" else None, variant=kind, episode_length=ep)
    env.set_od_bank(world.ODBank(occ, n_pairs=4096, seed=5, max_wp=32), seed=11)
    return env


@pytest.mark.parametrize("kind,E,N,ep,steps,seed", RUNS)
def test_real_env_tallies(native_lib, occ, kind, E, N, ep, steps, seed):
    from multi_agent_aac_amd.stats import EpisodeStats
    env = _make_env(kind, E, N, ep, occ)
    st = EpisodeStats.for_env(env, log=32)
    L = int(env.cfg.episode_length)
    assert L == (ep or {"att": 50, "wgru": 150, "uam": 150}[kind])
    assert (st.goal_bit, st.return_mode) == {"att": (5, 1), "wgru": (5, 0), "uam": (4, 0)}[kind]
    ref = stats_ref.StatsRef(E, N, L, st.goal_bit, st.return_mode, log=32)
    bufs = [env.alloc_buffers(), env.alloc_buffers()]
    env.auto_reset(None, out=bufs[0])
    g = torch.Generator(device="cuda").manual_seed(seed)
    adt = torch.float64 if kind == "uam" else torch.float32
    fused = kind != "uam" and ep is None
    # even envs: full-scale random accelerations (crashes within a few steps); odd envs: 2 % of them,
    # a slow random walk around the start that outlasts the step limit
    scale = torch.where(torch.arange(E, device="cuda") % 2 == 0, 1.0, 0.02).to(adt).view(E, 1, 1)
    for t in range(steps):
        n = bufs[1 - (t & 1)]
        act = (torch.rand(E, N, 2, device="cuda", generator=g, dtype=adt) * 2 - 1) * scale
        if fused:
            env.step_tail(act, out=n, replay=None)
            st.accumulate(n)
        else:
            env.step(act, out=n)
            st.accumulate(n)
            env.auto_reset(n.env_done, out=n)
        ref.accumulate(*[getattr(n, f).cpu().numpy() for f in ("reward", "done", "mask", "env_done", "bbc")])
    got = st.read()
    print(kind, ep, {k: got[k] for k in stats_ref.COUNTERS}, got["reach_hist"])
    stats_ref.check_totals(got, ref)
    stats_ref.check_state(st, ref)
    stats_ref.check_log(st, ref)
    assert got["crash"] > 0 and got["timeout"] > 0, got
    assert got["episodes"] == got["timeout"] + got["crash"] + got["goal"]
    assert got["episodes"] == got["collision_count"] + got["all_steps_used"] == sum(got["reach_hist"])
