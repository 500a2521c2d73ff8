"""The learner's records on the device (include/aac_monitor.h): per-update losses, Q / target ranges
and gradient / parameter norms, kept beside update loops that never leave the GPU.

A ``LearnerMonitor`` attached to a model (``model.attach_monitor``) makes the fused learners append
small launches to their launch lists -- one ``aac_monitor_vec`` launch after each Adam launch, the two
launches of ``aac_monitor_commit`` after the Polyak launch -- so every execution form carries them: eager,
the update graph and the whole-step graphs.  The last ``ring`` updates' records, running aggregates
since ``reset()`` and a sticky "first non-finite update" word live in torch tensors this object owns
(``tensors()`` names the ones a checkpoint needs), so a resumed run continues its records exactly.

One update has A columns: the N gradient iterations (ATT), the N agents (GRU) or 1 (UAM).  Fields and
the reference's names (ATT/main:575-580, ATT/maddpg:372-379, :442-453):
  loss_q                c_loss                    loss_a                  a_loss
  pre_min / pre_max     tar_Q_before_rew min/max  y_mean / y_min / y_max  tar_Q_after_rew
  r_mean / r_min / r_max  the batch rewards       grad_norm_* / *_grad_nonfinite   has_gradients
"""
import ctypes
import math

import numpy as np
import torch

from . import _native
from .fused import adam4_order  # noqa: F401  (the order field of a vec job that follows adam_sum / sum_partials)
from .tally import check, stream

FIELDS = 27           # AAC_MONITOR_FIELDS
VEC_WG = 64           # AAC_MONITOR_VEC_WG
VEC_VALUES = 6        # AAC_MONITOR_VEC_VALUES
NETS = ("critic", "actor")
MAX_COLS = 64         # AAC_MONITOR_MAX_COLS
AGG = ("count", "sum", "sumsq", "min", "max")
# the record's field order (include/aac_monitor.h)
FIELD_NAMES = ("loss_q", "loss_a", "q_mean", "q_min", "q_max", "y_mean", "y_min", "y_max", "r_mean", "r_min",
               "r_max", "td_absmax", "pre_min", "pre_max", "rows_nonfinite") + tuple(
    f"{net}_{what}_{k}" for net in NETS for what in ("grad", "param") for k in ("sumsq", "absmax", "nonfinite"))
assert len(FIELD_NAMES) == FIELDS
COUNT_FIELDS = tuple(i for i, n in enumerate(FIELD_NAMES) if n.endswith("nonfinite"))


class VecLaunch:
    """One aac_monitor_vec launch over one or two jobs.  ``reads`` describes what each job reads, as
    (gradient tensor, parameter tensor, job) with the job's offsets in elements, for tools and tests."""

    def __init__(self, mon, jobs, f64):
        assert 1 <= len(jobs) <= 2
        self.mon, self.f64 = mon, int(bool(f64))
        self.reads = jobs
        self.arr = (_native.MonitorVecJob * len(jobs))()
        esz = 8 if f64 else 4
        for k, (g, p, j) in enumerate(jobs):
            a = self.arr[k]
            a.g, a.param = g.data_ptr() + esz * j.get("g_off", 0), p.data_ptr() + esz * j.get("p_off", 0)
            a.n, a.gstride, a.seg_stride = j["n"], j.get("gstride", j["n"]), j.get("seg_stride", j["n"])
            a.nsplit, a.nseg, a.order = j.get("nsplit", 1), j.get("nseg", 1), j.get("order", 0)
            a.col0, a.net, a.cols = j.get("col0", 0), j["net"], mon.A
            a.gscale, a.scratch = j.get("gscale", 1.0), mon.scratch.data_ptr()
        self._fn = _native.lib().aac_monitor_vec

    def __call__(self):
        rc = self._fn(self.arr, len(self.reads), self.f64, stream())
        if rc != 0:
            check(rc, "aac_monitor_vec", "aac_monitor_last_error")


class CommitLaunch:
    """The aac_monitor_commit launch of an update; ``rows`` maps the field names (q, y, q_a, reward, qn,
    done) to (tensor, element offset, column stride, row stride)."""

    def __init__(self, mon, B, rows, a_off=0.0, gamma=0.0, done_width=0, f64=False):
        self.mon, self.rows = mon, rows
        a = self.args = _native.MonitorCommitArgs()
        esz = 8 if f64 else 4
        for name in ("q", "y", "q_a", "reward", "qn", "done"):
            if rows.get(name) is None:
                continue
            t, off, cs, rs = rows[name]
            r = getattr(a, name)
            r.p, r.col_stride, r.row_stride = t.data_ptr() + esz * off, cs, rs
        a.done_width, a.f64, a.A, a.B, a.R = done_width, int(bool(f64)), mon.A, B, mon.R
        a.a_off, a.gamma = a_off, gamma
        a.scratch, a.rec = mon.scratch.data_ptr(), mon.rec.data_ptr()
        a.ring, a.ring_update = mon.ring.data_ptr(), mon.ring_update.data_ptr()
        a.agg, a.state = mon.agg.data_ptr(), mon.state.data_ptr()
        self._ref = ctypes.byref(a)
        self._fn = _native.lib().aac_monitor_commit

    def __call__(self):
        rc = self._fn(self._ref, stream())
        if rc != 0:
            check(rc, "aac_monitor_commit", "aac_monitor_last_error")


def unwrap(counter, ring, ring_update, agg, bad):
    """``LearnerMonitor.read()``'s dict from host copies of the buffers: ring [R][A][FIELDS], ring_update
    [R], agg [5][A][FIELDS]."""
    R = ring.shape[0]
    n = min(int(counter), R)
    first = int(counter) - n
    # (after a reset() the ring holds fewer records than the counter says: a slot counts only if it
    # carries the index it would hold)
    order = [(first + k) % R for k in range(n) if int(ring_update[(first + k) % R]) == first + k]
    n = len(order)
    rec = ring[order] if n else np.zeros((0,) + ring.shape[1:])
    out = {"updates": int(counter), "bad_update": int(bad),
           "update": (ring_update[order] if n else np.zeros(0)).astype(np.int64)}
    for i, name in enumerate(FIELD_NAMES):
        out[name] = rec[:, :, i].copy()
    for net in NETS:
        for what in ("grad", "param"):
            out[f"{what}_norm_{net}"] = np.sqrt(out[f"{net}_{what}_sumsq"])
    cnt, s, ss = agg[0], agg[1], agg[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(cnt > 0, s / cnt, np.nan)
        var = np.where(cnt > 0, ss / cnt - mean * mean, np.nan)
    stats = {"count": cnt, "mean": mean, "std": np.sqrt(np.maximum(var, 0.0)),
             "min": np.where(cnt > 0, agg[3], np.nan), "max": np.where(cnt > 0, agg[4], np.nan)}
    for k, v in stats.items():
        out[k] = {name: v[:, i].copy() for i, name in enumerate(FIELD_NAMES)}
    return out


class LearnerMonitor:
    """Records of the last ``ring`` updates of A columns + aggregates since ``reset()``.

    dtype   the learner's element type: torch.float32 (ATT, GRU) or torch.float64 (UAM)
    """

    def __init__(self, A, ring=64, dtype=torch.float32, device=None):
        if not 1 <= int(A) <= MAX_COLS:
            raise ValueError(f"LearnerMonitor: 1 <= A <= {MAX_COLS}")
        if int(ring) < 1:
            raise ValueError("LearnerMonitor: ring >= 1")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("LearnerMonitor: dtype float32 or float64")
        self.A, self.R, self.dtype = int(A), int(ring), dtype
        d = self.device = torch.device(device if device is not None else "cuda")
        f64 = dict(dtype=torch.float64, device=d)
        self.scratch = torch.zeros(self.A, len(NETS), VEC_WG, VEC_VALUES, **f64)
        self.rec = torch.zeros(self.A, FIELDS, **f64)          # the record between the commit's two launches
        self.ring = torch.zeros(self.R, self.A, FIELDS, **f64)
        self.ring_update = torch.zeros(self.R, dtype=torch.int64, device=d)
        self.agg = torch.zeros(len(AGG), self.A, FIELDS, **f64)
        self.state = torch.zeros(2, dtype=torch.int64, device=d)       # update counter, first non-finite update
        self.reset()

    # ------------------------------------------------------------------- state
    def reset(self):
        """Clear the aggregates, the ring and the sticky word; the update counter runs on."""
        self.ring.zero_()
        self.ring_update.fill_(-1)
        self.agg.zero_()
        self.agg[3] = math.inf
        self.agg[4] = -math.inf
        self.state[1] = -1

    def tensors(self):
        """The device tensors a checkpoint must carry (loaded in place)."""
        return {"ring": self.ring, "ring_update": self.ring_update, "agg": self.agg, "state": self.state}

    # ------------------------------------------------------------------- launches
    def vec(self, *jobs):
        """A launch over one or two jobs (gradient tensor, parameter tensor, dict(n, net, col0, nsplit,
        gstride, nseg, seg_stride, order, g_off, p_off, gscale))."""
        for g, p, _ in jobs:
            if g.dtype != self.dtype or p.dtype != self.dtype:
                raise ValueError(f"monitor vec job: {self.dtype} tensors")
        return VecLaunch(self, list(jobs), self.dtype == torch.float64)

    def commit(self, B, rows, a_off=0.0, gamma=0.0, done_width=0):
        for name, r in rows.items():
            if r is not None and r[0].dtype != self.dtype:
                raise ValueError(f"monitor commit rows {name}: {self.dtype} tensors")
        return CommitLaunch(self, int(B), rows, float(a_off), float(gamma), int(done_width),
                            self.dtype == torch.float64)

    # ------------------------------------------------------------------- reads
    def read(self):
        """The kept records and the aggregates as plain numpy (synchronises): ``updates`` the total
        count, ``update`` the kept records' indices (ascending), one [n][A] array per field name plus
        ``grad_norm_<net>`` / ``param_norm_<net>``, and ``count`` / ``mean`` / ``std`` / ``min`` / ``max``
        dicts of [A] arrays per field over the updates since ``reset()``."""
        st = self.state.cpu().numpy()
        return unwrap(st[0], self.ring.cpu().numpy(), self.ring_update.cpu().numpy(), self.agg.cpu().numpy(), st[1])

    def bad_update(self):
        """Index of the first update since ``reset()`` with a non-finite count in its record, else -1
        (downloads one word)."""
        return int(self.state[1])

    def check(self):
        bad = self.bad_update()
        if bad >= 0:
            raise FloatingPointError(f"learner monitor: non-finite values first seen in update {bad}")

