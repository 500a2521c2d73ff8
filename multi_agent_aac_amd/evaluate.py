"""Noise-free evaluation rollouts (the reference's eval mode, ATT/main:669-882: ``choose_action``
with ``noisy=False`` and the training tallies), on the device.

``Evaluator(trainer)`` builds its OWN env from the trainer's maps and OD bank (or the UAM episode
bank) with its own draw seed, episode counters and output buffers, and rolls the trainer's current
actor in it with no exploration noise and no replay push.  The training env, the replay, the
learner's noise counter and the trainer's captured graphs are never touched, so an evaluation can
run between any two training steps.  Every ``evaluate`` call replays the same episode set (the eval
env's episode counters are zeroed first): common random numbers across checkpoints.

``record`` plays the same episode set with a flight recorder (``record.FlightRecorder``) and also
returns the flown paths and per-step status as ``record.Trajectories``.

With several ranks each rank evaluates its own envs; the results are not combined.
"""
import torch

from . import graphs as _graphs
from . import trainer as _trainer
from .stats import EpisodeStats
from .tally import ACT, STEP, Tallies

POLL = 16      # steps between two reads of the "envs still under quota" word


class Evaluator:
    """``evaluate(k)`` plays k episodes in each of E eval envs and returns their statistics
    (``EpisodeStats.read()``: exactly E * k episodes).

    ``terms=True`` (ATT, GRU and UAM trainers): the eval env gets a reward-terms buffer and a reward ledger
    (``terms.RewardLedger``) fed beside the statistics under the same quota, so it holds the same
    episode set; ``evaluate`` then returns ``(stats, ledger.read())`` and ``record``
    ``(stats, Trajectories, ledger.read())``, the trajectories with a ``terms`` array.

    ``visits=True`` (or a dict of ``visits.VisitMap`` keywords): ``self.visits`` keeps the exploration maps
    of the noise-free rollout -- the positions and actions of the episodes the statistics count (an env
    at its quota adds nothing more) -- emptied at the start of every ``evaluate`` / ``record`` call and
    read with ``self.visits.read()``.  The eval env counts episodes of its own, so every sample of a call
    goes into ONE period: the one the training loop is in, read at the start of the call from the
    TRAINING env's per-env episode counter (``trainer.episode``, the counter the noise schedule reads):
    "explore" while its minimum over the envs is ``<= explore_until``, i.e. until every training env has
    left the noise schedule, "exploit" afterwards.  The read synchronises.

    ``sorties=True`` (or a dict of ``sorties.SortieStats`` keywords: log, reach_margin): ``self.sorties``
    keeps the by-sortie report of the reference (UAM/main:1130-1144: every aircraft of every finished
    episode in one class, the flight-distance ratio of those that reached their goals, the
    steps-before-collision histogram), emptied at the start of every ``evaluate`` / ``record`` call, fed
    under the same quota as ``self.stats`` (the same episode set) and read with ``self.sorties.read()``.
    The accumulator needs the terminal positions, which the fused step tail has already reset, so with
    sorties on the ATT and GRU rollouts of ``evaluate`` run the split launch sequence of ``record`` (act,
    step, tallies, hidden-state zeroing, auto-reset): the same results, a few more launches a step.  The
    return values of ``evaluate`` / ``record`` do not change; off (the default) not one launch or tensor
    changes."""

    def __init__(self, trainer, E=None, seed=0, log=0, terms=False, visits=False, sorties=False):
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
        self.quota = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.tally = Tallies()      # fed under the quota, emptied at the start of every call
        self.stats = self.tally.add(EpisodeStats.for_env(self.env, log=log), STEP)
        self.ledger = self.visits = self.sorties = None
        self._period = None     # the period of this call's samples (None without a visit map)
        if terms:
            from .terms import RewardLedger
            self.ledger = self.tally.add((RewardLedger.for_uam if self.uam else RewardLedger.for_env)(self.env), STEP)
        if visits:
            from .visits import VisitMap
            self.visits = self.tally.add(VisitMap(self.env, **(dict(visits) if isinstance(visits, dict) else {})), ACT)
            self._vis_sel = torch.zeros(self.E, dtype=torch.bool, device=dev)
            self._vis_sel_u8 = self._vis_sel.view(torch.uint8)
        if sorties:
            from .sorties import SortieStats
            kw = dict(sorties) if isinstance(sorties, dict) else {}
            self.sorties = self.tally.add((SortieStats.for_uam if self.uam else SortieStats.for_env)(self.env, **kw),
                                          STEP)
        # the sortie accumulator reads the terminal positions, which the fused step tail has already reset
        self._split = self.sorties is not None and not self.uam
        self._reads = [t.read for t in (self.stats, self.ledger) if t is not None]      # what a call returns
        if self.gru:
            from . import gru
            # hidden states as the trainer's ping-pong pair, and act plans of this object's own: the
            # learner's plan cache (shaped to the training buffers) is left alone
            self.hp = [torch.zeros(self.E, self.N, gru.H, device=dev) for _ in range(2)]
            self._acts = [gru._ActPlan(self.model, self.bufs[p].own, self.bufs[p].radar, self.hp[p], self.hp[1 - p])
                          for p in range(2)]
        self._graphs = {}       # period -> the pair of step graphs
        self._rec = self._rec_key = self._rec_graphs = None     # built by the first record()

    def _start(self):
        """The eval env at the start of its episode set: counters zeroed, every env redrawn."""
        self.episode.zero_()
        if self.gru:
            self.hp[0].zero_()
        self.env.auto_reset(None, out=self.bufs[0])

    def _visit(self, act):
        """The visit map's launch, after the act launch: the envs still under their quota, as the
        statistics count them."""
        if self.tally.act:
            torch.lt(self.stats.ep_count, self.quota, out=self._vis_sel)
            self.tally.after_act(act, sel=self._vis_sel_u8, period=self._period)

    def _begin(self, k):
        """The start of an ``evaluate`` / ``record`` call: the quota, and the period of its samples."""
        self.quota.fill_(k)
        if self.tally.act:
            self._period = 0 if int(self.tr.episode.min()) <= self.visits.explore_until else 1

    @torch.no_grad()
    def _step(self, p):
        """One eval step from buffer parity p: act without noise (the learner's noise counter does not
        advance), env step with auto-reset and no replay push, tally."""
        c, n = self.bufs[p], self.bufs[1 - p]
        if self._split:
            # the split sequence, no recorder
            return self._record_step(p, rec=None)
        if self.uam:
            act = self.model.act(c.own, c.radar, self.episode, noisy=False)
            self._visit(act)
            self.env.step(act, out=n)
            self.tally.after_step(n, self.quota)
            self.env.auto_reset(n.env_done, out=n)
            return
        if self.gru:
            act, hn, _ = self._acts[p](None)
            self._visit(act)
            # a new episode starts from a zero hidden state, as in training (WGRU/ma_main:476-478)
            self.env.step_tail(act, out=n, replay=None, zero_rows=hn)
        else:
            act = self.model.act(c.own, c.radar, c.nei, self.episode, noisy=False)
            self._visit(act)
            self.env.step_tail(act, out=n, replay=None)
        self.tally.after_step(n, self.quota)

    @torch.no_grad()
    def _record_step(self, p, rec=True):
        """``_step`` as separate launches, so that the recorder sees the terminal state before the reset
        and the fresh state after it: act, env step, record, tally, zero the finished envs' hidden
        states, auto-reset, record the reset rows.  Same results as the fused tail.  ``rec=None``: the
        same sequence without the recorder's launches (``evaluate`` with sorties on)."""
        rec = self._rec if rec else None
        c, n = self.bufs[p], self.bufs[1 - p]
        hn = None
        if self.uam:
            act = self.model.act(c.own, c.radar, self.episode, noisy=False)
        elif self.gru:
            act, hn, _ = self._acts[p](None)
        else:
            act = self.model.act(c.own, c.radar, c.nei, self.episode, noisy=False)
        self._visit(act)
        self.env.step(act, out=n)
        if rec is not None:
            rec.after_step(n, act)
        self.tally.after_step(n, self.quota)
        if hn is not None:
            from . import gru
            gru.reset_hidden(hn, n.env_done)
        self.env.auto_reset(n.env_done, out=n)
        if rec is not None:
            rec.after_reset(n.env_done)

    def _capture(self, step=None):
        # one eager step per parity first: act plans and buffers are built outside the captures
        step = step or self._step
        self._start()
        step(0)
        step(1)
        torch.cuda.synchronize()
        graphs = []
        for p in (0, 1):
            g = torch.cuda.CUDAGraph()
            with _graphs.capture(g):
                step(p)
            graphs.append(g)
        return graphs

    def evaluate(self, episodes_per_env=1):
        k = int(episodes_per_env)
        assert k >= 1
        use_graph = not _trainer.NO_GRAPH
        self._begin(k)
        if use_graph and self._period not in self._graphs:
            self._graphs[self._period] = self._capture()
        self._start()
        self.tally.reset()
        # an episode takes at most episode_length + 1 steps (timeout: episode_length < len)
        most = k * (self.episode_length + 1)
        for s in range(most):
            if use_graph:
                self._graphs[self._period][s & 1].replay()
            else:
                self._step(s & 1)
            if (s + 1) % POLL == 0 and self.stats.under_quota() == 0:
                break
        out = [read() for read in self._reads]
        return out[0] if len(out) == 1 else tuple(out)

    def record(self, episodes_per_env=1, env_ids=None, steps=None):
        """``evaluate(k)`` with a flight recorder on the envs ``env_ids`` (None: all): the same episode
        set, quota rule and early stop; returns ``(stats, Trajectories)``.  ``steps`` rows are kept per
        track; the default, k * (episode_length + 2), never drops one.  The rollout runs the split
        launch sequence (``_record_step``) from a pair of graphs of its own, captured on first use;
        ``evaluate`` and its graphs are not involved."""
        steps_run = self._record_rollout(episodes_per_env, env_ids, steps)
        assert steps_run > 0
        out = [read() for read in self._reads]
        return tuple(out[:1] + [self._rec.read()] + out[1:])

    def _record_rollout(self, episodes_per_env=1, env_ids=None, steps=None):
        """The device part of ``record``: nothing is downloaded but the poll word.  Returns the number
        of steps played."""
        from .record import FlightRecorder
        k = int(episodes_per_env)
        assert k >= 1
        S = int(steps) if steps is not None else k * (self.episode_length + 2)
        self._begin(k)
        key = (None if env_ids is None else tuple(int(e) for e in env_ids), S, k, self._period)
        if self._rec_key != key:
            self._rec_graphs = None
            self._rec = FlightRecorder.for_env(self.env, env_ids, steps=S, episodes=k)
            self._rec_key = key
        rec = self._rec
        use_graph = not _trainer.NO_GRAPH
        if use_graph and self._rec_graphs is None:
            self._rec_graphs = self._capture(self._record_step)
        self._start()
        self.tally.reset()
        rec.reset()
        rec.after_reset(None)
        for s in range(k * (self.episode_length + 1)):
            if use_graph:
                self._rec_graphs[s & 1].replay()
            else:
                self._record_step(s & 1)
            if (s + 1) % POLL == 0 and self.stats.under_quota() == 0:
                break
        return s + 1
