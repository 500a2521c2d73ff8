"""What the learner monitor costs per training step: monitor on against off on the benchmark's timed
loops, in one process, alternating, on ONE trainer.

  config 3   Trainer(4096, 5, B = 1024, replay 1e5, combined radar), ``step_graph_pair``
  config 4   Trainer(4096, 8, B = 512, replay 1e5, model="gru"), ``step_graph_pair``
  config 5   UamTrainer(8192, 16, B = 512, replay 2^20), host-launched ``step``

One trainer per config is built with ``monitor=True``, pre-filled and warmed up.  "Off" is the same
trainer with the monitor detached and update plans and whole-step graphs of its own (built without the
monitor's launches): both variants run on the same env, replay and learner state (two trainer
instances in one process differ by more than what is measured, tools/stats_cost.py).  Then ROUNDS
rounds of STEPS steps each are timed for each variant in turn (off, on, off, on, ...), a host clock
around work that ends in a device synchronise.  Printed per config: every round's ms per step, the
medians, on - off, their ratio and the spread (max - min) of the off rounds, which is what a difference
has to exceed to mean anything; ``--parts`` adds a third variant whose update plan carries the commit
launch only (no vec launches), which splits the cost between the two kinds of launch.

    python tools/monitor_cost.py [--configs 3 4 5] [--rounds 6] [--steps 400] [--parts] > profiles/monitor_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import monitor, trainer  # noqa: E402

MODEL_STATE = ("_fplans", "_plans", "_fu", "_graph", "_graph_B", "_graph_stats")
TRAINER_STATE = ("_sg", "_sg2")


def build(config):
    if config == 5:
        return trainer.UamTrainer(8192, 16, 512, 1 << 20, seed=0, monitor=True)
    if config == 4:
        return trainer.Trainer(4096, 8, 512, 100000, "combined", seed=0, model="gru", monitor=True)
    return trainer.Trainer(4096, 5, 1024, 100000, "combined", seed=0, monitor=True)


class _NoVec(monitor.LearnerMonitor):
    """The monitor with its vec launches left out of the plans (``--parts``): same tensors."""

    def __init__(self, mon):
        self.__dict__.update(mon.__dict__)

    def vec(self, *jobs):
        return lambda: None


def _fresh(v):
    return {} if isinstance(v, dict) else None


class Variants:
    """The trainer with its monitor on ("on"), off ("off") or commit-only ("commit"); each variant keeps
    its own update plans and captured graphs."""

    def __init__(self, tr):
        self.tr, self.cur = tr, "on"
        for k in TRAINER_STATE:                     # (Trainer makes _sg2 on first use)
            if not hasattr(tr, k):
                setattr(tr, k, {})
        self.mon = {"on": tr.monitor, "off": None, "commit": _NoVec(tr.monitor)}
        self.kept = {}

    def select(self, name):
        tr, m = self.tr, self.tr.model
        self.kept[self.cur] = ({k: getattr(m, k) for k in MODEL_STATE if hasattr(m, k)},
                               {k: getattr(tr, k) for k in TRAINER_STATE if hasattr(tr, k)})
        if name in self.kept:
            ms, ts = self.kept[name]
        else:
            ms = {k: _fresh(getattr(m, k)) for k in MODEL_STATE if hasattr(m, k)}
            ts = {k: {} for k in TRAINER_STATE if hasattr(tr, k)}
        for k, v in ms.items():
            setattr(m, k, v)
        for k, v in ts.items():
            setattr(tr, k, v)
        m.monitor = tr.monitor = self.mon[name]
        tr._sg_mon = m.monitor                      # (the trainers drop their graphs when these move)
        if hasattr(m, "_fu"):
            tr._sg_fu = m._fu
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
    p.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--parts", action="store_true")
    a = p.parse_args()
    assert a.rounds >= 5 and a.steps % 2 == 0
    torch.backends.cuda.matmul.allow_tf32 = False
    names = ["off", "on"] + (["commit"] if a.parts else [])
    for c in a.configs:
        torch.manual_seed(777)
        tr = build(c)
        while len(tr.replay) < 100000:
            tr.step(update=False)
        for _ in range(a.warmup):
            tr.step(update=True)
        graphed = tr.graph_ok()
        var = Variants(tr)
        for name in names:                       # plans, captures and one untimed round each
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
            print(f"  monitor {n:7s}", " ".join(f"{v:.4f}" for v in ms[n]), f" median {med[n]:.4f}")
        print(f"  on - off {1e3 * (med['on'] - med['off']):+.2f} us per step, on / off {med['on'] / med['off']:.4f}; "
              f"spread of the off rounds {1e3 * (max(ms['off']) - min(ms['off'])):.2f} us")
        if a.parts:
            print(f"  commit only - off {1e3 * (med['commit'] - med['off']):+.2f} us per step "
                  f"(the rest of on - off is the vec launches)")
        var.select("on")
        out = tr.monitor.read()
        print(f"  updates recorded {out['updates']}, first non-finite update {out['bad_update']}; last loss_q "
              f"{out['loss_q'][-1].tolist()}, grad_norm_critic {out['grad_norm_critic'][-1].tolist()}", flush=True)
        del var, tr
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
