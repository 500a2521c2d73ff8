"""Episode statistics on the device (include/aac_stats.h): the per-episode tallies the reference
prints every 100 episodes (ATT/main:563-637), kept beside a loop that never leaves the GPU.

``EpisodeStats.accumulate(bufs)`` is one small launch after each env step (two with a log) on torch's
current stream; it may be captured in a HIP graph with the step.  ``read()`` folds the per-workgroup
slots and downloads the totals.  Everything the kernels touch is a torch tensor this object owns
(``tensors()`` names the ones a checkpoint needs), so a resumed run continues its tallies exactly.

Counters and the reference's names (ATT/main):
  episodes          len(score_history)            return_sum / episodes   mean of score_history
  collision_count   collision_count               crash_bound             crash_to_bound
  crash_building    crash_to_building             crash_drone             crash_to_drone
  crash_nearest     crash_due_to_nearest          all_steps_used          all_steps_used
  reach_hist[1]     one_drone_reach               reach_hist[2]           two_drone_reach
  reach_hist[N]     all_drone_reach               timeout / crash / goal  the branch of :448-462 taken
"""
import math

import numpy as np
import torch

from . import _native
from .tally import SlotTally, check

EPW = 256             # AAC_STATS_EPW: envs per workgroup (= per slot)
FIELDS = 81           # AAC_STATS_FIELDS
COUNTERS = ("episodes", "steps", "timeout", "crash", "goal", "collision_count", "crash_bound", "crash_building",
            "crash_drone", "crash_nearest", "all_steps_used", "under_quota")
F_SUM, F_SQ, F_MIN, F_MAX, F_HIST = 12, 13, 14, 15, 16
REASONS = ("timeout", "crash", "goal")
ROW = np.dtype([("ret", "<f8"), ("step", "<i8"), ("len", "<i4"), ("env", "<i4"), ("reason", "<i4"),
                ("crash", "<i2"), ("reach", "<i2")])      # aac_stats_row
assert ROW.itemsize == 32


class EpisodeStats(SlotTally):
    """Running per-env episode state + totals for E envs x N agents.

    reward_dtype  torch.float32 (``StepBuffers``) or torch.float64 (``UamBuffers``)
    goal_bit      the mask bit "goal branch taken this step": 5 (aac_env.h) or 4 (aac_uam.h)
    return_mode   1: agent 0's reward (the team reward every agent carries); 0: the sum over agents
    log           > 0: keep the last ``log`` finished episodes as rows, in (step, env) order
    """
    EPW, FIELDS, ROW = EPW, FIELDS, ROW
    MIN, MAX = slice(F_MIN, F_MIN + 1), slice(F_MAX, F_MAX + 1)
    STATE = ("run_return", "run_len", "run_reach", "ep_count", "slots")
    REDUCE, ERROR = "aac_stats_reduce", "aac_stats_last_error"

    def __init__(self, E, N, episode_length, reward_dtype=torch.float32, goal_bit=5, return_mode=1, log=0,
                 device=None):
        if not 1 <= N <= 64:
            raise ValueError("EpisodeStats: 1 <= N <= 64")
        if reward_dtype not in (torch.float32, torch.float64):
            raise ValueError("EpisodeStats: reward_dtype float32 or float64")
        self.E, self.N, self.episode_length = int(E), int(N), int(episode_length)
        self.reward_dtype, self.goal_bit, self.return_mode = reward_dtype, int(goal_bit), int(return_mode)
        d = self.device = torch.device(device if device is not None else "cuda")
        self.run_return = torch.zeros(self.E, dtype=torch.float64, device=d)
        self.run_len = torch.zeros(self.E, dtype=torch.int32, device=d)
        self.run_reach = torch.zeros(self.E, dtype=torch.int64, device=d)          # uint64 bit sets
        self.ep_count = torch.zeros(self.E, dtype=torch.int32, device=d)
        self._accumulate = _native.lib().aac_stats_accumulate
        self._alloc(_native.StatsState(), log)

    @classmethod
    def for_env(cls, env, log=0):
        """For a ``BatchedEnv`` (att: agent 0's reward under the team reward, else the sum; wgru: the
        sum of the per-agent rewards) or a ``BatchedUAM`` (float64 rewards, summed)."""
        from .uam import BatchedUAM
        ep = int(env.cfg.episode_length)
        if isinstance(env, BatchedUAM):
            return cls(env.E, env.N, ep, torch.float64, goal_bit=4, return_mode=0, log=log, device=env.device)
        return cls(env.E, env.N, ep, torch.float32, goal_bit=5, return_mode=1 if env.cfg.team_reward else 0,
                   log=log, device=env.device)

    def accumulate(self, bufs, quota=None, step_index=-1):
        """Tally the step whose outputs are in ``bufs`` (a ``StepBuffers`` / ``UamBuffers``), after the
        step launch on the same stream.  ``quota``: int32 [E] tensor (or an int, kept in
        ``self.quota``): an env with that many finished episodes contributes nothing more.
        ``step_index`` >= 0 is logged with the rows instead of the device's call count.  A buffer
        set's tensors are taken as fixed: its launch arguments are built on the first call."""
        args = self._args(bufs, self._quota(quota), (step_index,))
        rc = self._accumulate(self._st_ref, args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            check(rc, "aac_stats_accumulate", self.ERROR)

    def _build(self, bufs, quota, step_index):
        r = bufs.reward
        if r.dtype != self.reward_dtype or tuple(r.shape) != (self.E, self.N) or not r.is_contiguous():
            raise ValueError(f"reward {tuple(r.shape)} {r.dtype}: expected ({self.E}, {self.N}) {self.reward_dtype}")
        for name, shape in (("done", (self.E, self.N)), ("mask", (self.E, self.N)), ("env_done", (self.E,)),
                            ("bbc", (self.E, 4))):
            t = getattr(bufs, name)
            if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} {tuple(t.shape)} {t.dtype}: expected {shape} uint8")
        p = _native.StatsStep()
        p.quota = self._quota_ptr(quota)
        p.reward, p.reward_f64 = r.data_ptr(), int(r.dtype == torch.float64)
        p.done, p.mask = bufs.done.data_ptr(), bufs.mask.data_ptr()
        p.env_done, p.bbc = bufs.env_done.data_ptr(), bufs.bbc.data_ptr()
        p.E, p.N, p.episode_length = self.E, self.N, self.episode_length
        p.goal_bit, p.return_mode = self.goal_bit, self.return_mode
        p.step_index = int(step_index)
        return p

    def under_quota(self):
        """Envs whose finished-episode count was below its quota after the last ``accumulate``
        (synchronises)."""
        return int(self._reduce()[COUNTERS.index("under_quota")])

    def read(self, clear=False):
        """Totals as a dict (synchronises): the named counters, ``reach_hist`` (N + 1 bins), the
        return sums, and derived mean / std return, mean length and per-episode rates.  ``clear``
        empties the totals afterwards (a per-window report); running episodes carry on."""
        raw = self._reduce(clear)
        out = {k: int(raw[i]) for i, k in enumerate(COUNTERS)}
        d = raw.view(np.float64)
        n = out["episodes"]
        out["return_sum"], out["return_sqsum"] = float(d[F_SUM]), float(d[F_SQ])
        out["return_min"] = float(d[F_MIN]) if n else math.nan
        out["return_max"] = float(d[F_MAX]) if n else math.nan
        out["reach_hist"] = [int(v) for v in raw[F_HIST:F_HIST + self.N + 1]]
        mean = out["return_sum"] / n if n else math.nan
        out["return_mean"] = mean
        out["return_std"] = math.sqrt(max(out["return_sqsum"] / n - mean * mean, 0.0)) if n else math.nan
        out["length_mean"] = out["steps"] / n if n else math.nan
        for k in ("timeout", "crash", "goal", "collision_count"):
            out[k.replace("_count", "") + "_rate"] = out[k] / n if n else math.nan
        out["all_reach_rate"] = out["reach_hist"][self.N] / n if n else math.nan
        return out
