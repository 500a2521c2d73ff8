"""What gradient clipping costs per captured ``update``: grad_clip off against 1.0 and inf, in one
process, alternating, on ONE model per config.

  config 3   maddpg.MADDPG, N = 5, B = 1024, replay of 16384 synthetic transitions
  config 4   gru.MADDPG, N = 8, B = 512, the same (``--configs 3 4``)

Each variant keeps its own update plan and captured graph on the same model (weights, optimiser state and
replay are shared; two model instances in one process differ by more than what is measured,
tools/stats_cost.py).  After an untimed round per variant, ROUNDS rounds of UPDATES graph replays are timed
for each variant in turn (off, 1.0, inf, off, ...), a host clock around work that ends in a device
synchronise.  Printed per config: the plans' launch counts, every round's us per update, the medians, each
variant minus off and the spread (max - min) of the off rounds, which is what a difference has to exceed to
mean anything; then the clip record of the 1.0 variant.  "off" builds the launch list the learner has
without the feature.

    python tools/mb_clip.py [--configs 3 4] [--rounds 7] [--updates 300] > profiles/clip_cost.txt
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import gru, maddpg  # noqa: E402

ATTRS = ("clip", "_fplans", "_plans", "_graph", "_graph_B", "_graph_stats", "_side")
VALUES = {"off": None, "1.0": 1.0, "inf": math.inf}


def fill(rep, N, D0, hidden, E=4096, pushes=4, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    K = N - 1
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)          # noqa: E731
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)           # noqa: E731
    for _ in range(pushes):
        rows = [r(E, N, D0), u(E, N, 18) * 15, r(E, N, K, 6) * 0.5, u(E, N, 2) * 2 - 1, r(E, 1).repeat(1, N) * 5,
                (u(E, N) < 0.1).float(), r(E, N, D0), u(E, N, 18) * 15, r(E, N, K, 6) * 0.5]
        if hidden:
            rows += [torch.tanh(r(E, N, 64)), torch.tanh(r(E, N, 64))]
        rep.push_batch(*rows)


def build(config):
    if config == 4:
        N, B = 8, 512
        m = gru.MADDPG([6, 18, 6], [6, 18, 6], 2, 64, 10, n_agents=N, seed=777, batch_size=B, memory_length=16384)
    else:
        N, B = 5, 1024
        D0 = 6 + 4 * (N - 1)
        m = maddpg.MADDPG([D0, 18, 6], [D0, 18, 6], 2, n_agents=N, seed=777, batch_size=B, memory_length=16384)
    rep = m.attach_replay(16384, seed=3)
    fill(rep, N, m.D0, config == 4)
    return m, B


class Variants:
    """One model under several grad_clip values; each keeps its own plans, graph and clip state."""

    def __init__(self, m):
        self.m, self.cur, self.kept = m, None, {}
        self.opts = (m.critic_optimizer, m.actor_optimizer)

    def select(self, name):
        m = self.m
        if self.cur is not None:
            self.kept[self.cur] = ({k: getattr(m, k) for k in ATTRS if hasattr(m, k)}, [o.clip_step for o in self.opts])
        if name in self.kept:
            attrs, steps = self.kept[name]
            for k, v in attrs.items():
                setattr(m, k, v)
            for o, s in zip(self.opts, steps):
                o.clip_step = s
        else:
            m.set_grad_clip(VALUES[name])        # fresh plans; the graph is captured by the next update
        self.cur = name


def timed(m, B, updates):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        m.update(B, want_stats=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / updates * 1e6


def n_launches(m, B):
    p = m._plan(B) if hasattr(m, "_plan") else m._fused_plan(B)
    return len(p.ops())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=int, nargs="+", default=[3])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--updates", type=int, default=300)
    a = p.parse_args()
    assert a.rounds >= 5
    torch.backends.cuda.matmul.allow_tf32 = False
    names = list(VALUES)
    for c in a.configs:
        m, B = build(c)
        var = Variants(m)
        counts = {}
        for name in names:                       # plans, captures and one untimed round each
            var.select(name)
            timed(m, B, a.updates)
            counts[name] = n_launches(m, B)
        us = {n: [] for n in names}
        for _ in range(a.rounds):
            for name in names:
                var.select(name)
                us[name].append(timed(m, B, a.updates))
        med = {n: statistics.median(v) for n, v in us.items()}
        print(f"config {c} (captured update, {a.rounds} rounds x {a.updates} updates, us per update)")
        for n in names:
            print(f"  grad_clip {n:4s} launches {counts[n]:3d} ", " ".join(f"{v:.2f}" for v in us[n]), f" median {med[n]:.2f}")
        for n in names[1:]:
            print(f"  {n} - off {med[n] - med['off']:+.2f} us per update ({counts[n] - counts['off']} launches more), "
                  f"ratio {med[n] / med['off']:.4f}")
        print(f"  spread of the off rounds {max(us['off']) - min(us['off']):.2f} us")
        var.select("1.0")
        rec = m.clip_record()
        print("  grad_clip 1.0 record:", {k: {n: v.tolist() for n, v in d.items()} for k, d in rec.items()}, flush=True)
        del var, m
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
