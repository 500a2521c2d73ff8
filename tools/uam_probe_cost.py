"""What a UAM radar probe costs: ``UamRadarProbe.run`` (one launch, aac_uam_probe) at E = 8192, N = 16, next to
``BatchedUAM.step`` of the same handle for scale.

The env is reset from an episode bank and flown for 10 random steps (finished envs replaced); that state is
the snapshot every step launch starts from.  Each launch sits between its own pair of HIP events: 20 launches
after 5 warm-up launches; printed: every launch's us, the median and the spread (max - min).

    python tools/uam_probe_cost.py > profiles/uam_probe_cost.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import uam  # noqa: E402
from multi_agent_aac_amd.probe import UamRadarProbe  # noqa: E402

E, N, WARM, LAUNCHES = 8192, 16, 5, 20


def build():
    env = uam.BatchedUAM(E, N)
    env.set_bank(uam.build_bank(16384, N, seed=2026), seed=1234)
    env.auto_reset()
    g = torch.Generator(device="cuda").manual_seed(E)
    for _ in range(10):
        b = env.step(torch.rand(E, N, 2, device="cuda", generator=g, dtype=torch.float64) * 2 - 1)
        env.auto_reset(b.env_done)
    act = torch.rand(E, N, 2, device="cuda", generator=g, dtype=torch.float64) * 2 - 1
    torch.cuda.synchronize()
    return env, act, {k: v.clone() for k, v in env.get_state().items()}


def launches(fn, before=None):
    us = []
    for k in range(WARM + LAUNCHES):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= WARM:
            us.append(a.elapsed_time(b) * 1e3)
    return us


def report(name, us):
    print(f"  {name:22s} " + " ".join(f"{x:7.1f}" for x in us))
    print(f"  {'':22s} median {statistics.median(us):8.2f}   spread {max(us) - min(us):6.2f}")


def main():
    print(f"device {torch.cuda.get_device_name(0)}; E = {E}, N = {N}; {LAUNCHES} launches after {WARM} warm-ups, "
          "us per launch (one HIP event pair each)")
    env, act, snap = build()
    pr = UamRadarProbe.for_uam(env)
    step = launches(lambda: env.step(act), before=lambda: env.set_state(**snap))
    env.set_state(**snap)
    probe = launches(pr.run)
    report("env.step", step)
    report("probe.run", probe)
    print(f"  probe / step {statistics.median(probe) / statistics.median(step):.2f}")
    print(f"  rays per kind on the snapshot: {pr.summary()}")


if __name__ == "__main__":
    main()
