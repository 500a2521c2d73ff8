"""What the reward ledger costs per training step: ``terms=True`` against off on the benchmark's timed
loops, in one process, alternating, on ONE trainer (the method of tools/monitor_cost.py).

  config 3   Trainer(4096, 5, B = 1024, replay 1e5, combined radar), ``step_graph_pair``
  config 4   Trainer(4096, 8, B = 512, replay 1e5, model="gru"), ``step_graph_pair``
  config 5   UamTrainer(8192, 16, B = 512, replay 2^20), host-launched ``step`` (its whole-step graph is
             off by default)

The trainer is built with ``terms=True``, pre-filled and warmed up.  "Off" is the same trainer with the
terms buffer detached from the env (its step launches are the plain instantiations again), no ledger
launch, and whole-step graphs of its own.  ROUNDS rounds of STEPS steps are timed for each variant in
turn (off, on, off, on, ...), a host clock around work that ends in a device synchronise.  Printed per
config: every round's ms per step, the medians, on - off, their ratio and the spread (max - min) of the
off rounds, which is what a difference has to exceed to mean anything.

    python tools/terms_cost.py [--configs 3 4 5] [--rounds 6] [--steps 400] > profiles/terms_cost.txt
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
        return trainer.UamTrainer(8192, 16, 512, 1 << 20, seed=0, terms=True)
    if config == 4:
        return trainer.Trainer(4096, 8, 512, 100000, "combined", seed=0, model="gru", terms=True)
    return trainer.Trainer(4096, 5, 1024, 100000, "combined", seed=0, terms=True)


class Variants:
    """The trainer with its ledger on or off; each variant keeps its own captured graphs."""

    def __init__(self, tr):
        self.tr, self.cur = tr, "on"
        self.ledger, self.buf = tr.ledger, tr.env.terms
        self.tally = {"on": tr.tally, "off": tr.tally.without(tr.ledger)}
        if not hasattr(tr, "_sg2"):
            tr._sg2 = {}
        self.kept = {}

    def select(self, name):
        tr = self.tr
        self.kept[self.cur] = (tr._sg, tr._sg2)
        tr._sg, tr._sg2 = self.kept.get(name, ({}, {}))
        if name == "on":
            tr.env.use_terms_buffer(self.buf)
            tr.ledger = self.ledger
        else:
            tr.env.use_terms_buffer(detach=True)
            tr.ledger = None
        tr.tally = self.tally[name]
        self.cur = name


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
    p.add_argument("--configs", type=int, nargs="+", default=[3, 4])
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--warmup", type=int, default=10)
    a = p.parse_args()
    assert a.rounds >= 5 and a.steps % 2 == 0
    torch.backends.cuda.matmul.allow_tf32 = False
    names = ["off", "on"]
    for c in a.configs:
        torch.manual_seed(777)
        tr = build(c)
        while len(tr.replay) < 100000:
            tr.step(update=False)
        for _ in range(a.warmup):
            tr.step(update=True)
        graphed = tr.graph_ok()
        var = Variants(tr)
        for name in names:                       # captures and one untimed round each
            var.select(name)
            timed(tr, graphed, a.steps)
        ms = {n: [] for n in names}
        for _ in range(a.rounds):
            for name in names:
                var.select(name)
                ms[name].append(timed(tr, graphed, a.steps))
        med = {n: statistics.median(v) for n, v in ms.items()}
        mode = "step_graph_pair" if graphed else "step"
        print(f"config {c} ({mode}, {a.rounds} rounds x {a.steps} steps, ms per step)")
        for n in names:
            print(f"  terms {n:3s}", " ".join(f"{v:.4f}" for v in ms[n]), f" median {med[n]:.4f}")
        print(f"  on - off {1e3 * (med['on'] - med['off']):+.2f} us per step, on / off {med['on'] / med['off']:.4f}; "
              f"spread of the off rounds {1e3 * (max(ms['off']) - min(ms['off'])):.2f} us")
        var.select("on")
        out = tr.terms()
        shares = {k: round(v["share"], 4) for k, v in out["terms"].items()}
        print(f"  episodes in the ledger {out['episodes']}, mean return {out['return_mean']:.4f}, shares {shares}",
              flush=True)
        del var, tr
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
