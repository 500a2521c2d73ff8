"""What the exploration maps cost per training step: ``visits`` on against off on the benchmark's timed
loops, in one process, alternating, on ONE trainer (the manner of tools/stats_cost.py), and the
accumulate launch on its own beside the episode statistics' accumulate launch.

  config 3   Trainer(4096, 5, B = 1024, replay 1e5, combined radar), ``step_graph_pair``
  config 5   UamTrainer(8192, 16, B = 512, replay 2^20), host-launched ``step``

One trainer per config is built with ``visits=True, stats=True``, pre-filled and warmed up.  "Off" is
the same trainer with the maps left out of ``trainer.tally`` and whole-step graphs of its own (captured without the
launch): both variants run on the same env, buffers, replay and learner.  ROUNDS rounds of STEPS steps
are timed for each variant in turn (off, on, off, on, ...), a host clock around work that ends in a
device synchronise.  Printed per config: every round's ms per step, the medians, the difference
on - off and the spread (max - min) of the off rounds, which a difference has to exceed to mean anything.

The launches on their own: a graph of LAUNCHES identical launches between two events, replayed REPS
times, the median per launch -- for the visits launch on the trainer's live positions with the actions
of a real step, with every action at the (1, -1) corner (a saturated actor: every row of a workgroup in
one LDS bin), and for ``EpisodeStats.accumulate`` on the same trainer's step outputs.

    python tools/visits_cost.py [--configs 3 5] [--rounds 6] [--steps 400] > profiles/visits_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import graphs, trainer  # noqa: E402

LAUNCHES, REPS = 100, 20


def build(config):
    if config == 5:
        return trainer.UamTrainer(8192, 16, 512, 1 << 20, seed=0, stats=True, visits=True)
    if config == 4:
        return trainer.Trainer(4096, 8, 512, 100000, "combined", seed=0, model="gru", stats=True, visits=True)
    return trainer.Trainer(4096, 5, 1024, 100000, "combined", seed=0, stats=True, visits=True)


class Variants:
    """The trainer with its visit map on or off; each variant keeps its own captured graphs."""

    def __init__(self, tr):
        self.tr, self.visits, self.on = tr, tr.visits, True
        self.tally = {True: tr.tally, False: tr.tally.without(tr.visits)}
        self.graphs = {True: ({}, {}), False: ({}, {})}

    def select(self, on):
        tr = self.tr
        self.graphs[self.on] = (tr._sg, getattr(tr, "_sg2", None) or {})
        tr._sg, tr._sg2 = self.graphs[on]
        tr.visits, tr.tally = self.visits if on else None, self.tally[on]
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


def launch_us(fn):
    """Median microseconds per launch of ``fn`` over REPS replays of a graph of LAUNCHES of them."""
    fn()
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        for _ in range(LAUNCHES):
            fn()
    g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return statistics.median(us)


def launches(tr):
    """The accumulate launches alone, on the trainer's live state and the actions of a real step."""
    seen = []
    tr.post_step_hooks.append(lambda t, act, c, n: seen.append(act.clone()))
    tr.step(update=False)
    tr.post_step_hooks.clear()
    act = seen[0]
    corner = torch.ones_like(act)
    corner[..., 1] = -1.0
    vm, st = tr.visits, tr.stats
    out = [("visits, a real step's actions", launch_us(lambda: vm.accumulate(act))),
           ("visits, every action at one corner", launch_us(lambda: vm.accumulate(corner))),
           ("stats accumulate", launch_us(lambda: st.accumulate(tr.cur)))]
    return out, vm.E * vm.N


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--configs", type=int, nargs="+", default=[3, 5])
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
        for on in (False, True):          # one untimed round each
            var.select(on)
            timed(tr, graphed, a.steps)
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for on in (False, True):
                var.select(on)
                ms[on].append(timed(tr, graphed, a.steps))
        off, on = statistics.median(ms[False]), statistics.median(ms[True])
        mode = "step_graph_pair" if graphed else "step"
        print(f"config {c} ({mode}, {a.rounds} rounds x {a.steps} steps, ms per step)")
        print("  visits off ", " ".join(f"{v:.4f}" for v in ms[False]), f" median {off:.4f}")
        print("  visits on  ", " ".join(f"{v:.4f}" for v in ms[True]), f" median {on:.4f}")
        print(f"  on - off {1e3 * (on - off):+.2f} us per step; spread of the off rounds "
              f"{1e3 * (max(ms[False]) - min(ms[False])):.2f} us", flush=True)
        var.select(True)
        out = tr.finish()["visits"]
        print(f"  rows counted in the on rounds: {int(out['samples'].sum())} "
              f"(outside the bound {int(out['pos_outside'].sum())}, actions outside {int(out['act_outside'].sum())}); "
              f"position bins used {int((out['pos'] > 0).sum())} of {out['pos'].size}, "
              f"action bins used {int((out['act'] > 0).sum())} of {out['act'].size}")
        rows, n = launches(tr)
        print(f"  one launch alone ({n} rows, graph of {LAUNCHES} launches, median of {REPS} replays):")
        for name, us in rows:
            print(f"    {name:<36s} {us:7.2f} us", flush=True)
        del var, tr
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
