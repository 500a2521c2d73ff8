"""Gradient-norm clipping inside the learners' launch lists (include/aac_clip.h).

The reference clips each network's gradient before its optimiser step
(``torch.nn.utils.clip_grad_norm_(net.parameters(), 1)``, ATT/maddpg:187, :205-206).  With
``grad_clip`` set on a model, every Adam boundary of its launch lists becomes two launches:
``aac_clip_sumsq`` (the copies' sum, written to ``flat.grad``, and per-workgroup sums of squares) and
``aac_adam_flat_clip`` (the norm, ``coef = min(1, max_norm / (norm + 1e-6))`` and the Adam step on
``g * coef``).  ``coef`` lives in registers: ``flat.grad`` and the learner monitor keep showing the
pre-clip gradient.  A ``GradClip`` owns the bounds, the partials and the per-unit record
``[net][unit][RECORD]`` (per rank, not checkpointed).

A unit is what the reference hands one ``clip_grad_norm_`` call: the whole flat buffer of a network
(ATT), or one agent's segment of it (GRU).
"""
import ctypes
import math

import numpy as np
import torch

from . import _native

THREADS = 256         # AAC_CLIP_THREADS
CHUNK = 1024          # AAC_CLIP_CHUNK
ADAM_MAX_WG = 1024    # AAC_CLIP_ADAM_MAX_WG
RECORD = 6            # AAC_CLIP_RECORD
FIELDS = ("steps", "clipped", "nonfinite", "last_norm", "last_coef", "max_norm_seen")
NETS = ("critic", "actor")
vp = ctypes.c_void_p


def _chk(rc, what):
    if rc != 0:
        msg = _native.lib().aac_clip_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def partials(n):
    """P: partials per unit of n elements (aac_clip_partials)."""
    return (int(n) + CHUNK - 1) // CHUNK


def parse(value):
    """``grad_clip`` -> None (off) or a (critic, actor) pair of bounds, each a float >= 0 (``inf``
    allowed) or None (that network is not clipped)."""
    if value is None:
        return None
    pair = tuple(value) if isinstance(value, (tuple, list)) else (value, value)
    if len(pair) != 2:
        raise ValueError("grad_clip: None, a float or a (critic, actor) pair")
    out = []
    for v in pair:
        if v is not None:
            v = float(v)
            if math.isnan(v) or v < 0.0:
                raise ValueError("grad_clip: bounds are >= 0 (float('inf') allowed)")
        out.append(v)
    return None if out == [None, None] else tuple(out)


class Launch:
    """One aac_clip_sumsq or aac_adam_flat_clip launch over one or two jobs."""

    def __init__(self, name, jobs, f64=False):
        assert 1 <= len(jobs) <= 2
        self.name, self.f64 = name, int(bool(f64))
        self.jobs = list(jobs)
        self.arr = (_native.ClipJob * len(jobs))(*jobs)
        self._fn = getattr(_native.lib(), name)

    def __call__(self):
        rc = self._fn(self.arr, len(self.jobs), self.f64, _stream())
        if rc != 0:
            _chk(rc, self.name)


def job(g, param, exp_avg, exp_avg_sq, step, part, record, n, max_norm, lr, betas, eps, nsplit=1, gstride=0,
        order=0, grad_out=None, step_add=0, gscale=1.0, nseg=1, seg_stride=0):
    """An aac_clip_job over torch tensors (all of one element type)."""
    j = _native.ClipJob()
    j.g, j.grad_out = g.data_ptr(), (grad_out.data_ptr() if grad_out is not None else None)
    j.param, j.exp_avg, j.exp_avg_sq = param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    j.step, j.partials, j.record = step.data_ptr(), part.data_ptr(), record.data_ptr()
    j.n, j.gstride, j.seg_stride = int(n), int(gstride or n), int(seg_stride or n)
    j.nsplit, j.nseg, j.order, j.step_add = int(nsplit), int(nseg), int(order), int(step_add)
    j.gscale, j.max_norm = float(gscale), float(max_norm)
    j.lr, j.beta1, j.beta2, j.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
    return j


class Step:
    """One clipped Adam boundary of one network: ``sumsq`` then ``adam``."""

    def __init__(self, j, f64=False):
        self.job, self.f64 = j, f64
        self.sumsq, self.adam = Launch("aac_clip_sumsq", [j], f64), Launch("aac_adam_flat_clip", [j], f64)


def pair(a, b):
    """Two networks' boundaries as two two-job launches [sumsq, adam]."""
    return [Launch("aac_clip_sumsq", [a.job, b.job], a.f64), Launch("aac_adam_flat_clip", [a.job, b.job], a.f64)]


class GradClip:
    """The clipping state of one model: bounds per network, ``units`` units per network, the record."""

    def __init__(self, bounds, units, device):
        self.bounds, self.units = tuple(bounds), int(units)
        self.device = torch.device(device)
        self.record = torch.zeros(len(NETS), self.units, RECORD, dtype=torch.float64, device=self.device)
        self._parts = {}

    def on(self, net):
        return self.bounds[net] is not None

    def step(self, net, opt, g, nsplit=1, gstride=0, order=0, grad_out=None, step_add=0, gscale=1.0):
        """The boundary of network ``net`` (0 critic, 1 actor) with optimiser ``opt`` (maddpg._Adam) on
        the gradient copies ``g``: its ``units`` segments are equal parts of the flat buffer."""
        n = opt.flat.numel // self.units
        key = (net, n)
        if key not in self._parts:
            self._parts[key] = torch.zeros(self.units, partials(n), dtype=torch.float64, device=self.device)
        return Step(job(g, opt.flat.data, opt.exp_avg, opt.exp_avg_sq, opt.step_t, self._parts[key], self.record[net],
                        n, self.bounds[net], opt.lr, opt.betas, opt.eps, nsplit=nsplit, gstride=gstride, order=order,
                        grad_out=grad_out, step_add=step_add, gscale=gscale, nseg=self.units, seg_stride=n))

    def read(self, clear=False):
        """{field: {"critic": [units], "actor": [units]}} as plain numpy (synchronises); counters as
        int64.  ``clear`` zeroes the record afterwards."""
        r = self.record.cpu().numpy()
        if clear:
            self.record.zero_()
        out = {}
        for k, name in enumerate(FIELDS):
            out[name] = {nn: (r[i, :, k].astype(np.int64) if k < 3 else r[i, :, k].copy()) for i, nn in enumerate(NETS)}
        return out


def make(value, units, device):
    """A GradClip for ``grad_clip=value``, or None when it is off."""
    bounds = parse(value)
    return None if bounds is None else GradClip(bounds, units, device)
