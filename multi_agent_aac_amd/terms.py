"""Reward ledger (include/aac_terms.h): which terms an episode's return is made of, kept on the device.

With a terms buffer attached (``BatchedEnv.use_terms_buffer``, ``BatchedUAM.use_terms_buffer``) the env
step kernels store one row of ``WIDTH`` doubles per (env, agent): the eight contribution slots ``CONTRIB``
-- what the taken reward branch added, sign included; their left-to-right sum is the agent's own reward --
and four gauges.  ``RewardLedger.accumulate(bufs)`` is one small launch after each env step on torch's
current stream (it may be captured in a HIP graph with the step) and keeps, per finished episode, the sum
of every contribution slot over the episode's steps and agents; ``read()`` folds the per-workgroup slots
and downloads count, mean, std, min, max and each slot's share of the mean return.

Scope: the ATT and WGRU variants of ``BatchedEnv`` (``RewardLedger.for_env``) and the UAM env
(``BatchedUAM``, ``RewardLedger.for_uam``), whose rows carry the order-dependent crash and near-drone
coefficients in effect for each aircraft.  The MPE env emits
no terms; with several ranks each rank keeps its own ledger; a checkpoint does not carry the ledger (a
resumed run starts an empty one).
"""
import math

import numpy as np
import torch

from . import _native
from .tally import SlotTally, check

EPW = 256             # AAC_STATS_EPW: envs per workgroup (= per slot)
WIDTH = 12            # AAC_TERMS_W
SLOTS = 8             # AAC_TERMS_SLOTS
FIELDS = 33           # AAC_TERMS_FIELDS: episodes, then sum / sqsum / min / max of the 8 slots
F_SUM, F_SQ, F_MIN, F_MAX = 1, 1 + SLOTS, 1 + 2 * SLOTS, 1 + 3 * SLOTS
_names = None


def names():
    """The ``WIDTH`` slot names in row order: the header's table (AAC_TERMS_NAMES), read from the library."""
    global _names
    if _names is None:
        _names = tuple(_native.lib().aac_terms_names().decode().split(","))
        assert len(_names) == WIDTH
    return _names


class RewardLedger(SlotTally):
    """Per-episode totals of the reward terms of E envs x N agents."""
    EPW, FIELDS = EPW, FIELDS
    MIN, MAX = slice(F_MIN, F_MAX), slice(F_MAX, FIELDS)
    STATE = ("run", "ep_count", "slots")
    REDUCE, ERROR = "aac_terms_reduce", "aac_terms_last_error"

    def __init__(self, env):
        self.env, self.E, self.N = env, env.E, env.N
        d = self.device = env.device
        self.run = torch.zeros(self.E, self.N, SLOTS, dtype=torch.float64, device=d)
        self.ep_count = torch.zeros(self.E, dtype=torch.int32, device=d)
        self._accumulate = _native.lib().aac_terms_accumulate
        self._alloc(_native.TermsState())

    @classmethod
    def for_env(cls, env):
        """For a ``BatchedEnv`` (att or wgru).  The env's terms buffer is attached if it has none.  Any
        other env is refused, as before the UAM env had terms: a ``BatchedUAM`` goes through ``for_uam``."""
        from .env import BatchedEnv
        if not isinstance(env, BatchedEnv):
            raise NotImplementedError(f"RewardLedger.for_env: {type(env).__name__} is no BatchedEnv; it covers the ATT "
                                      "and WGRU variants (the UAM env: RewardLedger.for_uam; the MPE env emits no terms)")
        if env.terms is None:
            env.use_terms_buffer()
        return cls(env)

    @classmethod
    def for_uam(cls, env):
        """For a ``BatchedUAM``.  The env's terms buffer is attached if it has none."""
        from .uam import BatchedUAM
        if not isinstance(env, BatchedUAM):
            raise NotImplementedError(f"RewardLedger.for_uam: {type(env).__name__} is no BatchedUAM")
        if env.terms is None:
            env.use_terms_buffer()
        return cls(env)

    def accumulate(self, bufs, quota=None):
        """Add the step whose outputs are in ``bufs`` (``StepBuffers`` / ``UamBuffers``; its ``env_done`` is
        read) and whose terms are in the env's attached buffer, after the step launch on the same stream.
        ``quota``: int32 [E] tensor (or an int, kept in ``self.quota``), the rule of
        ``EpisodeStats.accumulate``: an env with that many finished episodes contributes nothing more."""
        quota = self._quota(quota)
        terms = self.env.terms
        if terms is None:
            raise RuntimeError("RewardLedger.accumulate: the env has no terms buffer attached (use_terms_buffer)")
        args = self._args(bufs, quota, (terms.data_ptr(),), (terms,))
        rc = self._accumulate(self._st_ref, args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            check(rc, "aac_terms_accumulate", self.ERROR)

    def _build(self, bufs, quota, terms_ptr):
        t = bufs.env_done
        if t.dtype != torch.uint8 or tuple(t.shape) != (self.E,) or not t.is_contiguous():
            raise ValueError(f"env_done {tuple(t.shape)} {t.dtype}: expected ({self.E},) uint8")
        p = _native.TermsStep()
        p.quota = self._quota_ptr(quota)
        p.terms, p.env_done, p.E, p.N = terms_ptr, t.data_ptr(), self.E, self.N
        return p

    raw = SlotTally._reduce

    def read(self, clear=False):
        """``{"episodes": n, "return_mean": sum of the slot means, "terms": {name: {"mean", "std", "min",
        "max", "sum", "share"}}}`` over the finished episodes (synchronises); a term's ``share`` is its
        mean over ``return_mean``.  ``clear`` empties the totals afterwards; running episodes carry on."""
        return summarize(self.raw(clear))


def summarize(raw):
    """``RewardLedger.read()`` from a totals record (int64 [FIELDS])."""
    raw = np.ascontiguousarray(raw, dtype=np.int64)
    d = raw.view(np.float64)
    n = int(raw[0])
    nm = names()[:SLOTS]
    mean = [float(d[F_SUM + k]) / n if n else math.nan for k in range(SLOTS)]
    total = math.fsum(mean) if n else math.nan
    out = {"episodes": n, "return_mean": total, "terms": {}}
    for k, name in enumerate(nm):
        out["terms"][name] = {
            "sum": float(d[F_SUM + k]), "mean": mean[k],
            "std": math.sqrt(max(float(d[F_SQ + k]) / n - mean[k] * mean[k], 0.0)) if n else math.nan,
            "min": float(d[F_MIN + k]) if n else math.nan, "max": float(d[F_MAX + k]) if n else math.nan,
            "share": mean[k] / total if n and total != 0.0 else math.nan}
    return out
