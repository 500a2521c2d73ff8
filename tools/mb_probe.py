"""What a radar probe costs: ``RadarProbe.run()`` (one launch, aac_env_probe) against the env step
(``BatchedEnv.step``: the step kernel and its band fix, aac_env_step) on the same states, in one process,
alternating.

  config 3   4096 envs x 5 agents, combined radar (ATT)
  config 4   4096 envs x 8 agents, obstacle radar (``variant="wgru"``)

The env is reset from an OD bank and flown for 10 random steps; that state is the snapshot.  After an untimed
round of each, ROUNDS rounds of LAUNCHES launches are timed for each in turn (step, probe, step, ...), a host
clock around work that ends in a device synchronise.  Every round starts from the snapshot (``set_state``): the
step rounds fly the same 300 steps from it with one fixed action tensor, the probe rounds probe it 300 times.
Printed per config: every round's us per launch, the medians, probe / step, and the spread (max - min) of the
step rounds, which is what a difference has to exceed to mean anything; then the probe's rays per kind.

    python tools/mb_probe.py [--configs 3 4] [--rounds 7] [--launches 300] > profiles/probe_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import world  # noqa: E402
from multi_agent_aac_amd.env import BatchedEnv  # noqa: E402
from multi_agent_aac_amd.probe import RadarProbe  # noqa: E402

E = 4096


def build(config):
    occ = world.synthetic_map(2026)
    if config == 4:
        env = BatchedEnv(E, 8, occ, variant="wgru")
    else:
        env = BatchedEnv(E, 5, occ, radar_mode="combined")
    env.set_od_bank(world.ODBank(occ, n_pairs=16384, seed=2026, max_wp=32), seed=1234)
    env.auto_reset(None)
    g = torch.Generator(device="cuda").manual_seed(config)
    for _ in range(10):
        env.step(torch.rand(E, env.N, 2, device="cuda", generator=g) * 2 - 1)
    act = torch.rand(E, env.N, 2, device="cuda", generator=g) * 2 - 1
    torch.cuda.synchronize()
    return env, act, {k: v.clone() for k, v in env.get_state().items()}


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=300)
    a = ap.parse_args()
    print(f"device {torch.cuda.get_device_name(0)}; {a.rounds} rounds of {a.launches} launches, us per launch")
    for config in a.configs:
        env, act, snap = build(config)
        probe = RadarProbe.for_env(env)
        runs = {"step": lambda: env.step(act), "probe": probe.run}
        us = {k: [] for k in runs}
        for rnd in range(a.rounds + 1):
            for k, fn in runs.items():
                env.set_state(**snap)
                t = timed(fn, a.launches)
                if rnd:                     # round 0: untimed warm-up
                    us[k].append(t)
        med = {k: statistics.median(v) for k, v in us.items()}
        print(f"config {config}: E {E} N {env.N} radar_mode {env.radar_mode} variant {env.variant}")
        for k, v in us.items():
            print(f"  {k:5s} rounds " + " ".join(f"{x:7.2f}" for x in v) + f"   median {med[k]:7.2f}")
        print(f"  probe / step {med['probe'] / med['step']:.2f}   probe - step {med['probe'] - med['step']:+.2f} us"
              f"   spread of the step rounds {max(us['step']) - min(us['step']):.2f} us")
        env.set_state(**snap)
        probe.run()
        print(f"  rays per kind on the snapshot: {probe.summary()}")


if __name__ == "__main__":
    main()
