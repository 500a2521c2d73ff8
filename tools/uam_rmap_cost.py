"""What a UAM reward map costs: ``UamRewardMap.at`` (one launch, aac_uam_reward_map) per launch, eager and as a
graph replay, next to ``BatchedUAM.step`` of the same handle for scale.

  N = 16, E = 1      2 500 rows (the default 50 x 50 grid of env 0)
  N = 16, E = 8192   2 500 rows (env 0), and 160 000 rows (64 envs x 2 500)

The env is reset from an episode bank and flown for 10 random steps (finished envs replaced); that state is the
snapshot every window starts from.  HIP events around back-to-back launches after 20 warm-up launches; 5 windows
of 200 (2 500 rows, step) or 50 (160 000 rows) launches; printed: every window's us per launch, the median and
the spread (max - min).  Eager = ``at`` with device-resident inputs and outputs, graph = replays of one captured
launch.

    python tools/uam_rmap_cost.py > profiles/uam_rmap_cost.txt
"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import graphs, uam  # noqa: E402
from multi_agent_aac_amd.rewardmap import UamRewardMap  # noqa: E402

N, WARM, WINDOWS = 16, 20, 5


def build(E):
    env = uam.BatchedUAM(E, N)
    env.set_bank(uam.build_bank(max(256, min(4 * E, 16384)), N, seed=2026), seed=1234)
    env.auto_reset()
    g = torch.Generator(device="cuda").manual_seed(E)
    for _ in range(10):
        b = env.step(torch.rand(E, N, 2, device="cuda", generator=g, dtype=torch.float64) * 2 - 1)
        env.auto_reset(b.env_done)
    act = torch.rand(E, N, 2, device="cuda", generator=g, dtype=torch.float64) * 2 - 1
    torch.cuda.synchronize()
    return env, act, {k: v.clone() for k, v in env.get_state().items()}


def windows(fn, n, before):
    us = []
    for _ in range(WINDOWS):
        before()
        for _ in range(WARM):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / n)
    return us


def report(name, us):
    print(f"  {name:34s} " + " ".join(f"{x:8.2f}" for x in us) +
          f"   median {statistics.median(us):8.2f}   spread {max(us) - min(us):6.2f}")


def main():
    print(f"device {torch.cuda.get_device_name(0)}; N = {N}; {WINDOWS} windows after {WARM} warm-up launches, us per launch")
    for E, cases in ((1, (1,)), (8192, (1, 64))):
        env, act, snap = build(E)
        rm = UamRewardMap.for_uam(env)
        restore = lambda: env.set_state(**snap)         # noqa: E731
        print(f"E = {E}")
        report("env.step (eager)", windows(lambda: env.step(act), 200, restore))
        b = [float(v) for v in env.cfg.bound]
        X, Y = np.meshgrid(np.linspace(b[0], b[1], 50), np.linspace(b[2], b[3], 50))
        grid = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
        for nenv in cases:
            pts = torch.as_tensor(np.tile(grid, (nenv, 1)), device="cuda")
            ei = torch.arange(nenv, dtype=torch.int32, device="cuda").repeat_interleave(2500) if nenv > 1 else 0
            M, n = len(pts), (200 if nenv == 1 else 50)
            restore()
            out = rm.at(pts, env=ei)
            report(f"map {M} rows, eager", windows(lambda: rm.at(pts, env=ei, out=out), n, restore))
            g = torch.cuda.CUDAGraph()
            with graphs.capture(g):
                rm.at(pts, env=ei, out=out)
            report(f"map {M} rows, graph replay", windows(g.replay, n, restore))
            kinds = np.bincount(np.minimum(rm.read(out)["done"], 1), minlength=2)
            print(f"    rows not done / done on the snapshot: {kinds.tolist()}")


if __name__ == "__main__":
    main()
