"""What the device-side diagnostics share.

``SlotTally`` is the base of the three slot-based accumulators (``stats.EpisodeStats``,
``terms.RewardLedger``, ``sorties.SortieStats``; device side: csrc/aac_slots.h): every accumulate workgroup
folds its finished episodes into a slot of its own, ``_reduce`` folds the slots into ``totals`` in a fixed
order, and an optional ring keeps the last finished rows.  The base owns those tensors, ``reset()`` /
``tensors()`` over the subclass's ``STATE`` names, the ``quota`` rule, the per-buffer-set argument cache
and ``log_rows()``; a subclass keeps its step struct, its ``read()`` and its error texts.

``Tallies`` is the list of the diagnostics a loop has switched on, in launch order, so that the loops
call one object instead of testing each attribute.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what, last_error):
    """RuntimeError with the library's message (``last_error``: the name of its last-error call)."""
    if rc != 0:
        msg = getattr(_native.lib(), last_error)().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


class SlotTally:
    EPW = FIELDS = None         # envs per workgroup (= per slot), 8-byte fields of a slot / totals record
    MIN = MAX = None            # the columns of the record that hold minima / maxima (slices)
    STATE = ()                  # the tensors the kernels keep state in: attribute = state struct field names
    ROW = None                  # numpy dtype of a log row
    REDUCE = ERROR = None       # names of the library's reduce and last-error calls

    def _alloc(self, st, log=0, rows_per_env=1):
        """Slots, totals, quota and the optional log ring of ``log`` rows (``rows_per_env`` per finished
        env), beside the running-state tensors the subclass has made; fills the state struct ``st``."""
        E, d = self.E, self.device
        i32, i64, u8 = (dict(dtype=t, device=d) for t in (torch.int32, torch.int64, torch.uint8))
        self.slots = torch.zeros((E + self.EPW - 1) // self.EPW, self.FIELDS, **i64)
        self.totals = torch.zeros(self.FIELDS, **i64)
        self.quota = torch.zeros(E, **i32)              # used by accumulate(quota=<int>)
        self.L = int(log)
        self.log = self.log_meta = None
        for k in self.STATE:
            setattr(st, k, getattr(self, k).data_ptr())
        if self.L:
            self.log = torch.zeros(self.L, self.ROW.itemsize, **u8)
            self.log_meta = torch.zeros(2, **i64)
            self._fin = (torch.zeros(E, **u8), torch.zeros(E * rows_per_env, self.ROW.itemsize, **u8),
                         torch.zeros(E + 1, **i32))
            st.log, st.log_len, st.log_meta = self.log.data_ptr(), self.L, self.log_meta.data_ptr()
            st.fin_flag, st.fin_row, st.fin_list = (t.data_ptr() for t in self._fin)
        self._st, self._st_ref = st, ctypes.byref(st)
        self._steps = {}        # id(bufs), quota pointer, ... -> the step struct of a buffer set
        self.reset()

    # ------------------------------------------------------------------- state
    def reset(self):
        """Empty totals, running state, episode counts and log."""
        for k in self.STATE:
            getattr(self, k).zero_()
        sd = self.slots.view(torch.float64)
        sd[:, self.MIN] = math.inf
        sd[:, self.MAX] = -math.inf
        if self.L:
            self.log.zero_()
            self.log_meta.zero_()

    def tensors(self):
        """The device tensors a checkpoint must carry (loaded in place)."""
        t = {k: getattr(self, k) for k in self.STATE}
        if self.L:
            t["log"], t["log_meta"] = self.log, self.log_meta
        return t

    # ------------------------------------------------------------------- calls
    def _quota(self, quota):
        """``accumulate``'s quota argument as a tensor (an int is kept in ``self.quota``) or None."""
        if isinstance(quota, int):
            self.quota.fill_(quota)
            return self.quota
        return quota

    def _quota_ptr(self, quota):
        if quota is None:
            return None
        if quota.dtype != torch.int32 or tuple(quota.shape) != (self.E,) or not quota.is_contiguous():
            raise ValueError("quota: int32 [E]")
        return quota.data_ptr()

    def _args(self, bufs, quota, key=(), keep=()):
        """The launch arguments of a buffer set, built once by ``self._build(bufs, quota)`` (the loops
        alternate two sets): the call itself is a dictionary lookup and the launch.  ``key``: what else
        the arguments depend on; ``keep``: what else they point into."""
        key = (id(bufs), None if quota is None else quota.data_ptr()) + key
        hit = self._steps.get(key)
        if hit is None or hit[0] is not bufs:
            p = self._build(bufs, quota, *key[2:])
            if len(self._steps) > 64:
                self._steps.clear()
            hit = self._steps[key] = (bufs, ctypes.byref(p), quota, p) + keep
        return hit[1]

    def _reduce(self, clear=False):
        """The folded totals record as int64 [FIELDS] (view as float64 for the sums); synchronises."""
        check(getattr(_native.lib(), self.REDUCE)(self._st_ref, self.E, ctypes.c_void_p(self.totals.data_ptr()),
                                                   int(bool(clear)), stream()), self.REDUCE, self.ERROR)
        return self.totals.cpu().numpy()

    def log_rows(self):
        """The logged rows, oldest first, as a numpy record array (fields of ``ROW``)."""
        if not self.L:
            return np.zeros(0, dtype=self.ROW)
        n = int(self.log_meta[0])
        rows = self.log.cpu().numpy().view(self.ROW).reshape(-1)
        if n <= self.L:
            return rows[:n].copy()
        return np.roll(rows, -(n % self.L)).copy()


ACT, STEP = "act", "step"       # a tally's launch position: after the act launch / after the env step


class Tallies:
    """The diagnostics a loop keeps, in launch order.  ``add(obj, phase, ckpt, key)``: ``obj`` None is
    skipped; ``phase`` ACT / STEP (None: fed elsewhere); ``ckpt`` the prefix its ``tensors()`` are
    checkpointed under (None: not checkpointed); ``key`` the name ``report`` puts its ``read()`` under
    ("": the report's base dict; None: not reported)."""

    def __init__(self):
        self.items, self.act, self.step = [], [], []

    def add(self, obj, phase=None, ckpt=None, key=None):
        if obj is not None:
            self.items.append((obj, phase, ckpt, key))
            if phase is not None:
                (self.act if phase == ACT else self.step).append(obj)
        return obj

    def without(self, obj):
        """A copy of the list that leaves ``obj`` out (an "off" variant for a cost measurement)."""
        t = Tallies()
        for item in self.items:
            if item[0] is not obj:
                t.add(*item)
        return t

    def after_act(self, act, **kw):
        for t in self.act:
            t.accumulate(act, **kw)

    def after_step(self, bufs, quota=None):
        for t in self.step:
            t.accumulate(bufs, quota=quota)

    def reset(self):
        for obj, phase, _, _ in self.items:
            if phase is not None:
                obj.reset()

    def checkpoint_extra(self):
        return {f"{ckpt}.{k}": v for obj, _, ckpt, _ in self.items if ckpt for k, v in obj.tensors().items()}

    def report(self, out=None, keys=None):
        """``out`` (None: nothing yet) with the ``read()`` of every reported tally, of those under
        ``keys`` only if given; None while there is nothing to report.  Synchronises."""
        for obj, _, _, key in self.items:
            if key is None or (keys is not None and key not in keys):
                continue
            out = dict(out or {}, **(obj.read() if key == "" else {key: obj.read()}))
        return out
