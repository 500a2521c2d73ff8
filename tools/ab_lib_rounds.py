"""Interleaved A/B of builds of libaac_env.so on the benchmark's timed loop, in the form of
profiles/terms_cost.txt: one worker process per library (``AAC_LIB``), all alive for the whole
measurement, each with its own trainer, pre-filled, warmed up and with its whole-step graphs captured;
then SETTLE uncounted and ROUNDS counted rounds of STEPS steps, the workers taking turns (A, B, A, B,
...) so only one of them has work on the GPU at a time.  A host clock around work that ends in a device synchronise.

  config 3   Trainer(4096, 5, B = 1024, replay 1e5, combined radar), ``step_graph_pair``
  config 4   Trainer(4096, 8, B = 512, replay 1e5, model="gru"), ``step_graph_pair``
  config 5   UamTrainer(8192, 16, B = 512, replay 2^20), ``step`` (its whole-step graph is off by
             default, as in bench.py: profiles/r06_uam_step_graph_ab.txt)

Printed per config: every round's ms per step, the medians, each library's median minus A's and the
spread (max - min) of A's rounds, which is what a difference has to exceed to mean anything.

    python tools/ab_lib_rounds.py libA.so libB.so [libC.so ...] [--configs 3 4 5] [--rounds 6] [--steps 400]
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(config, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from multi_agent_aac_amd import trainer
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(777)
    if config == 5:
        tr = trainer.UamTrainer(8192, 16, 512, 1 << 20, seed=0)
    elif config == 4:
        tr = trainer.Trainer(4096, 8, 512, 100000, "combined", seed=0, model="gru")
    else:
        tr = trainer.Trainer(4096, 5, 1024, 100000, "combined", seed=0)
    while len(tr.replay) < 100000:
        tr.step(update=False)
    for _ in range(warmup):
        tr.step(update=True)
    graphed = tr.graph_ok()

    def timed():
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

    timed()                                  # captures and one untimed round
    print("ready", "step_graph_pair" if graphed else "step", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(f"ms {timed():.6f}", flush=True)


def expect(proc, word):
    while True:
        line = proc.stdout.readline()
        if not line:
            raise SystemExit(f"worker ended (exit {proc.wait()}) before '{word}'")
        if line.startswith(word):
            return line.split()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("libs", nargs="*")
    p.add_argument("--configs", type=int, nargs="+", default=[3, 4, 5])
    p.add_argument("--rounds", type=int, default=6)
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--settle", type=int, default=4,
                   help="untimed rounds of every worker, interleaved like the timed ones, before the first counted "
                        "round: the step time falls by some 5 us over the first seconds of steady load whatever the "
                        "library, which would otherwise be most of the spread")
    p.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)
    a = p.parse_args()
    assert a.steps % 2 == 0
    if a.worker:
        return worker(a.worker, a.steps, a.warmup)
    assert len(a.libs) >= 2 and a.rounds >= 5
    for c in a.configs:
        procs, mode = [], None
        for lib in a.libs:
            env = dict(os.environ, AAC_LIB=os.path.abspath(lib))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(c), "--steps",
                                           str(a.steps), "--warmup", str(a.warmup)], env=env, text=True,
                                          stdin=subprocess.PIPE, stdout=subprocess.PIPE))
            mode = expect(procs[-1], "ready")[1]     # one at a time: the others are idle while this one sets up
        ms = [[] for _ in procs]
        for r in range(a.settle + a.rounds):
            for k, pr in enumerate(procs):
                pr.stdin.write("go\n")
                pr.stdin.flush()
                v = float(expect(pr, "ms")[1])
                if r >= a.settle:            # the settling rounds run like the others and are not counted
                    ms[k].append(v)
        for pr in procs:
            pr.stdin.close()
            if pr.wait() != 0:
                raise SystemExit(f"worker exit {pr.returncode}")
        med = [statistics.median(v) for v in ms]
        print(f"config {c} ({mode}, {a.rounds} rounds x {a.steps} steps after {a.settle} settling rounds, ms per step)")
        for k, (lib, v, m) in enumerate(zip(a.libs, ms, med)):
            print(f"  {'ABCDEFGH'[k]} {lib:34s}", " ".join(f"{x:.4f}" for x in v), f" median {m:.4f}")
        for k in range(1, len(med)):
            print(f"  {'ABCDEFGH'[k]} - A {1e3 * (med[k] - med[0]):+.2f} us per step, "
                  f"{'ABCDEFGH'[k]} / A {med[k] / med[0]:.4f}")
        print(f"  spread of A's rounds {1e3 * (max(ms[0]) - min(ms[0])):.2f} us", flush=True)


if __name__ == "__main__":
    main()
