"""Noise-free evaluation rollouts (the reference's eval mode, ATT/main:669-882: ``choose_action``
with ``noisy=False`` and the training tallies), on the device.

``Evaluator(trainer)`` builds its OWN env from the trainer's maps and OD bank (or the UAM episode
bank) with its own draw seed, episode counters and output buffers, and rolls the trainer's current
actor in it with no exploration noise and no replay push.  The training env, the replay, the
learner's noise counter and the trainer's captured graphs are never touched, so an evaluation can
run between any two training steps.  Every ``evaluate`` call replays the same episode set (the eval
env's episode counters are zeroed first): common random numbers across checkpoints.

With several ranks each rank evaluates its own envs; the results are not combined.
"""
import torch

from . import trainer as _trainer
from .stats import EpisodeStats

POLL = 16      # steps between two reads of the "envs still under quota" word


class Evaluator:
    """``evaluate(k)`` plays k episodes in each of E eval envs and returns their statistics
    (``EpisodeStats.read()``: exactly E * k episodes)."""

    def __init__(self, trainer, E=None, seed=0, log=0):
        self.tr, self.model = trainer, trainer.model
        tenv = trainer.env
        self.E, self.N = int(E or trainer.E), trainer.N
        self.uam = isinstance(trainer, _trainer.UamTrainer)
        self.gru = bool(getattr(trainer, "gru", False))
        c = tenv.cfg
        if self.uam:
            from .uam import BatchedUAM
            self.env = BatchedUAM(self.E, self.N, episode_length=c.episode_length, device=tenv.device,
                                  neighbours=tenv.neighbours, p3=tenv.p3, tdcpa=tenv.tdcpa, dt=c.dt, acc_max=c.acc_max,
                                  vmax=c.vmax, pB=c.pB, radar_len=c.radar_len, bound=tuple(c.bound))
            self.env.set_bank(tenv.bank, seed=seed)
        else:
            from .env import VARIANTS, BatchedEnv
            variant = {v: k for k, v in VARIANTS.items()}[tenv.variant]
            self.env = BatchedEnv(self.E, self.N, tenv.occ, radar_mode=tenv.radar_mode, compat=bool(c.compat),
                                  team_reward=bool(c.team_reward), max_wp=tenv.W, episode_length=c.episode_length,
                                  device=tenv.device, bound=tuple(c.bound), cell=c.cell, dt=c.dt, acc_max=c.acc_max,
                                  vmax=c.vmax, pB=c.pB, radar_len=c.radar_len, variant=variant)
            self.env.set_od_bank(tenv.bank, seed=seed)
        self.episode_length = int(c.episode_length)
        dev = self.env.device
        self.episode = self.env.use_episode_buffer(torch.zeros(self.E, dtype=torch.int32, device=dev))
        self.bufs = [self.env.alloc_buffers(), self.env.alloc_buffers()]
        self.stats = EpisodeStats.for_env(self.env, log=log)
        self.quota = torch.zeros(self.E, dtype=torch.int32, device=dev)
        if self.gru:
            from . import gru
            # hidden states as the trainer's ping-pong pair, and act plans of this object's own: the
            # learner's plan cache (shaped to the training buffers) is left alone
            self.hp = [torch.zeros(self.E, self.N, gru.H, device=dev) for _ in range(2)]
            self._acts = [gru._ActPlan(self.model, self.bufs[p].own, self.bufs[p].radar, self.hp[p], self.hp[1 - p])
                          for p in range(2)]
        self._graphs = None

    def _start(self):
        """The eval env at the start of its episode set: counters zeroed, every env redrawn."""
        self.episode.zero_()
        if self.gru:
            self.hp[0].zero_()
        self.env.auto_reset(None, out=self.bufs[0])

    @torch.no_grad()
    def _step(self, p):
        """One eval step from buffer parity p: act without noise (the learner's noise counter does not
        advance), env step with auto-reset and no replay push, tally."""
        c, n = self.bufs[p], self.bufs[1 - p]
        if self.uam:
            act = self.model.act(c.own, c.radar, self.episode, noisy=False)
            self.env.step(act, out=n)
            self.stats.accumulate(n, quota=self.quota)
            self.env.auto_reset(n.env_done, out=n)
        elif self.gru:
            act, hn, _ = self._acts[p](None)
            # a new episode starts from a zero hidden state, as in training (WGRU/ma_main:476-478)
            self.env.step_tail(act, out=n, replay=None, zero_rows=hn)
            self.stats.accumulate(n, quota=self.quota)
        else:
            act = self.model.act(c.own, c.radar, c.nei, self.episode, noisy=False)
            self.env.step_tail(act, out=n, replay=None)
            self.stats.accumulate(n, quota=self.quota)

    def _capture(self):
        # one eager step per parity first: act plans and buffers are built outside the captures
        self._start()
        self._step(0)
        self._step(1)
        torch.cuda.synchronize()
        graphs = []
        for p in (0, 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._step(p)
            graphs.append(g)
        return graphs

    def evaluate(self, episodes_per_env=1):
        k = int(episodes_per_env)
        assert k >= 1
        use_graph = not _trainer.NO_GRAPH
        if use_graph and self._graphs is None:
            self._graphs = self._capture()
        self._start()
        self.stats.reset()
        self.quota.fill_(k)
        # an episode takes at most episode_length + 1 steps (timeout: episode_length < len)
        most = k * (self.episode_length + 1)
        for s in range(most):
            if use_graph:
                self._graphs[s & 1].replay()
            else:
                self._step(s & 1)
            if (s + 1) % POLL == 0 and self.stats.under_quota() == 0:
                break
        return self.stats.read()
