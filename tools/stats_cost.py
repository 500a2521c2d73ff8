"""What the episode statistics cost per training step: statistics on against off on the benchmark's
timed loops, in one process, alternating, on ONE trainer.

  config 3   Trainer(4096, 5, B = 1024, replay 1e5, combined radar), ``step_graph_pair``
  config 4   Trainer(4096, 8, B = 512, replay 1e5, model="gru"), ``step_graph_pair``
  config 5   UamTrainer(8192, 16, B = 512, replay 2^20), host-launched ``step``

One trainer per config is built with ``stats=True``, pre-filled and warmed up.  "Off" is the same
trainer with the statistics left out of ``trainer.tally`` and whole-step graphs of its own (captured without the tally
node): both variants run on the same env, buffers, replay and learner.  (Two trainer instances in one
process differ by more than the tally: with the launch replaced by a no-op, the instance built second
still ran config 5 43 us per step slower than the first.)  Then ROUNDS rounds of STEPS steps each are
timed for each variant in turn (off, on, off, on, ...), a host clock around work that ends in a device
synchronise.  Printed per config: every round's ms per step, the medians, the difference on - off and
the spread (max - min) of the off rounds, which is what a difference has to exceed to mean anything.

    python tools/stats_cost.py [--configs 3 4 5] [--rounds 6] [--steps 400] > profiles/stats_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import trainer  # noqa: E402


def build(config):
    if config == 5:
        return trainer.UamTrainer(8192, 16, 512, 1 << 20, seed=0, stats=True)
    if config == 4:
        return trainer.Trainer(4096, 8, 512, 100000, "combined", seed=0, model="gru", stats=True)
    return trainer.Trainer(4096, 5, 1024, 100000, "combined", seed=0, stats=True)


class Variants:
    """The trainer with its statistics on or off; each variant keeps its own captured graphs."""

    def __init__(self, tr):
        self.tr, self.stats, self.on = tr, tr.stats, True
        self.tally = {True: tr.tally, False: tr.tally.without(tr.stats)}
        self.graphs = {True: ({}, {}), False: ({}, {})}

    def select(self, on):
        tr = self.tr
        self.graphs[self.on] = (tr._sg, getattr(tr, "_sg2", None) or {})
        tr._sg, tr._sg2 = self.graphs[on]
        tr.stats, tr.tally = self.stats if on else None, self.tally[on]
        self.on = on


def prepare(tr, warmup):
    while len(tr.replay) < 100000:
        tr.step(update=False)
    for _ in range(warmup):
        tr.step(update=True)
    graphed = tr.graph_ok()
    v = Variants(tr)
    for on in (True, False):
        v.select(on)
        if graphed:
            for _ in range(2):          # capture and replay once
                tr.step_graph_pair()
    torch.cuda.synchronize()
    return v, graphed


def timed(tr, graphed, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if graphed:
        for _ in range(steps // 2):
            tr.step_graph_pair()
    else:
        for _ in range(steps):
            tr.step(update=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--warmup", type=int, default=10)
    a = p.parse_args()
    assert a.rounds >= 5 and a.steps % 2 == 0
    torch.backends.cuda.matmul.allow_tf32 = False
    for c in a.configs:
        torch.manual_seed(777)
        tr = build(c)
        var, graphed = prepare(tr, a.warmup)
        for stats in (False, True):          # one untimed round each
            var.select(stats)
            timed(tr, graphed, a.steps)
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for stats in (False, True):
                var.select(stats)
                ms[stats].append(timed(tr, graphed, a.steps))
        off, on = statistics.median(ms[False]), statistics.median(ms[True])
        mode = "step_graph_pair" if graphed else "step"
        print(f"config {c} ({mode}, {a.rounds} rounds x {a.steps} steps, ms per step)")
        print("  stats off  ", " ".join(f"{v:.4f}" for v in ms[False]), f" median {off:.4f}")
        print("  stats on   ", " ".join(f"{v:.4f}" for v in ms[True]), f" median {on:.4f}")
        print(f"  on - off {1e3 * (on - off):+.2f} us per step; spread of the off rounds "
              f"{1e3 * (max(ms[False]) - min(ms[False])):.2f} us", flush=True)
        var.select(True)
        tot = tr.finish()
        print(f"  episodes tallied in the on rounds: {tot['episodes']}")
        del var, tr
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
