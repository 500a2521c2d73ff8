"""What the flight recorder costs per evaluation step: ``Evaluator.record(k)`` against
``Evaluator.evaluate(k)`` of the same commit, on one evaluator, alternating, in one process.

  ATT   Trainer(256, 5, B = 256, replay 4096, combined radar), 256 eval envs, all tracked
  UAM   UamTrainer(256, 16, B = 256, replay 4096), 256 eval envs, all tracked

``evaluate`` replays the fused step (act, step + tail, tally); ``record`` the split sequence (act, step,
record, tally, [hidden reset,] auto-reset, record) from its own graphs.  Both play the same episodes,
stop after the same number of steps (the first multiple of the poll interval at which every env has
finished its k episodes) and end with the same download of the statistics.  The download of the
recording (``FlightRecorder.read``) is timed on its own and reported beside the rollout.  Printed per
config: every round's us per step for both, the medians, and their difference.  No threshold: the
figure is reported.

    python tools/record_cost.py [--rounds 5] [--episodes 2] > profiles/record_cost.txt
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multi_agent_aac_amd import evaluate, trainer  # noqa: E402

E = 256


def build(kind):
    if kind == "uam":
        return trainer.UamTrainer(E, 16, 256, 4096, seed=0)
    return trainer.Trainer(E, 5, 256, 4096, "combined", seed=0)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=2)
    a = ap.parse_args()
    k = a.episodes
    print(f"# flight recorder cost, {torch.cuda.get_device_name(0)}; E = {E} eval envs, all tracked, "
          f"{k} episodes per env, {a.rounds} rounds")
    for kind in ("att", "uam"):
        tr = build(kind)
        for _ in range(4):
            tr.step(update=True)
        ev = evaluate.Evaluator(tr, E=E, seed=0)
        want = ev.evaluate(k)               # captures
        got, tj = ev.record(k)              # captures
        assert all(got[f] == want[f] for f in ("episodes", "steps", "return_sum")), (got, want)
        mb = sum(v.numel() * v.element_size() for v in ev._rec.rows.values()) / 2 ** 20
        ev_us, rec_us, read_us = [], [], []

        def recorded():
            n = ev._record_rollout(k)
            ev.stats.read()
            return n
        steps = recorded()
        for _ in range(a.rounds):
            ev_us.append(clock(lambda: ev.evaluate(k))[0] / steps)
            t, n = clock(recorded)
            assert n == steps
            rec_us.append(t / steps)
            read_us.append(clock(ev._rec.read)[0])
        me, mr = statistics.median(ev_us), statistics.median(rec_us)
        print(f"{kind}: N = {tr.N}, episode_length {ev.episode_length}, {steps} steps per rollout, "
              f"{len(tj.episodes())} episodes, rows {mb:.1f} MiB on the device")
        print("  evaluate  us/step  " + "  ".join(f"{v:8.1f}" for v in ev_us) + f"   median {me:8.1f}")
        print("  record    us/step  " + "  ".join(f"{v:8.1f}" for v in rec_us) + f"   median {mr:8.1f}")
        print(f"  record - evaluate  {mr - me:+.1f} us/step (rollout only; spread of evaluate "
              f"{max(ev_us) - min(ev_us):.1f})")
        print(f"  read() download    median {statistics.median(read_us) / 1e3:.1f} ms per recording")
        ms = tj.min_separation()
        print(f"  closest approach   min {ms.min():.4f}  median {statistics.median(ms.tolist()):.4f}")
        del ev, tr
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
