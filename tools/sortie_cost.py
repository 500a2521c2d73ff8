"""What the sortie statistics cost: the accumulate launch on its own, and an evaluation with the
accumulator on against off.

  UAM   UamTrainer(8192, 16): ``trainer.sorties.accumulate`` on the outputs of a real step
  ATT   Trainer(4096, 5, combined radar) with an ``Evaluator`` of 4096 envs: ``ev.sorties.accumulate`` on the
        outputs of a real evaluation step, and ``Evaluator.evaluate(1)`` with sorties on (the split launch
        sequence) against off (the fused step tail), alternating, wall clock around a call that ends in a
        device synchronise

The launches on their own: a graph of LAUNCHES identical launches between two events, replayed REPS times,
the median per launch, beside ``EpisodeStats.accumulate`` on the same step outputs; and LAUNCHES launches
from the host between one event pair (launch-bound: what a loop that is not a graph pays).  Nothing here is
inside a timed region of bench.py.

    python tools/sortie_cost.py > profiles/sortie_cost.txt
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import graphs, trainer  # noqa: E402
from multi_agent_aac_amd.evaluate import Evaluator  # noqa: E402

LAUNCHES, REPS, ROUNDS = 200, 20, 5


def graph_us(fn):
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


def host_us(fn):
    """Microseconds per launch of LAUNCHES host launches between one event pair (median of 5)."""
    us = []
    for _ in range(5):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return statistics.median(us)


def report(name, E, N, so, st, bufs):
    """The launch on the step's own outputs, then with no env finishing and with every env finishing in a
    collision at the same length (``env_done`` and ``done`` rewritten, and put back): the repeated launch
    ends the same envs every time, so "every env" is the worst case for the histogram's adds."""
    print(f"{name}: {E} envs x {N} aircraft, one accumulate launch (graph of {LAUNCHES}, median of {REPS} replays; "
          f"{LAUNCHES} host launches between one event pair)")
    keep = bufs.env_done.clone(), bufs.done.clone()
    for case, ed in (("as the step left it", None), ("no env finishing", 0), ("every env finishing", 1)):
        if ed is not None:
            bufs.env_done.fill_(ed)
            bufs.done.fill_(ed)
        print(f"  {case} ({int(bufs.env_done.sum())} envs done)")
        for what, fn in (("sorties accumulate", lambda: so.accumulate(bufs)), ("stats accumulate", lambda: st.accumulate(bufs))):
            print(f"    {what:<22s} {graph_us(fn):7.2f} us in a graph   {host_us(fn):7.2f} us from the host", flush=True)
    bufs.env_done.copy_(keep[0])
    bufs.done.copy_(keep[1])


def main():
    torch.manual_seed(777)
    tr = trainer.UamTrainer(8192, 16, 512, 1 << 18, seed=0, stats=True, sorties=True)
    for _ in range(20):
        tr.step(update=False)
    report("UAM", tr.E, tr.N, tr.sorties, tr.stats, tr.cur)
    out = tr.finish()["sorties"]
    print(f"    sorties counted {out['sorties']}, reached {out['reached']}")
    del tr
    torch.cuda.synchronize()

    tr = trainer.Trainer(4096, 5, 1024, 100000, "combined", seed=0)
    for _ in range(10):
        tr.step(update=False)
    ev = {on: Evaluator(tr, E=4096, sorties=on) for on in (False, True)}
    for on in (False, True):
        ev[on].evaluate(1)          # captures the graphs
    ms = {False: [], True: []}
    for _ in range(ROUNDS):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = ev[on].evaluate(1)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3)
    e = ev[True]
    so = e.sorties.read()
    print(f"ATT: Evaluator.evaluate(1), 4096 envs x 5, {st['episodes']} episodes, {st['steps']} env steps counted, "
          f"{ROUNDS} rounds alternating, ms per call")
    print("    sorties off (fused tail)     ", " ".join(f"{v:.2f}" for v in ms[False]), f" median {statistics.median(ms[False]):.2f}")
    print("    sorties on  (split sequence) ", " ".join(f"{v:.2f}" for v in ms[True]), f" median {statistics.median(ms[True]):.2f}")
    print(f"    sorties {so['sorties']}: bound {so['bound']} obstacle {so['obstacle']} drone {so['drone']} reached {so['reached']} "
          f"idle {so['idle']}; ratio mean {so['ratio_mean']:.4f} std {so['ratio_std']:.4f}", flush=True)
    # the launch alone, on a real evaluation step's outputs, every env counting (no quota)
    e._start()
    e._step(0)
    e._step(1)
    report("ATT eval env", e.E, e.N, e.sorties, e.stats, e.bufs[0])


if __name__ == "__main__":
    main()
