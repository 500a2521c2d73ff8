"""numpy float64 restatement of include/aac_monitor.h, for the monitor tests.

The split-order sum of the partial gradient copies is done in the element type first (as the Adam
kernels do); everything after it is float64.  Sums are formed with ``math.fsum`` (the correctly rounded
sum of the float64 terms), so a kernel's double sum of the same terms in any order lies within
``count * 2^-53 * sum|terms|`` of them (the worst case of count - 1 roundings, each at most half an ulp
of a partial sum that never exceeds sum|terms|).
"""
import math

import numpy as np

from multi_agent_aac_amd.monitor import COUNT_FIELDS, FIELD_NAMES, FIELDS

U = 2.0 ** -53
F = {n: i for i, n in enumerate(FIELD_NAMES)}


def sum_copies(g, order):
    """g [nsplit][n] in the element type -> [n] in the element type.  order 0: copies in sequence;
    order 1: the groups s % 4 each in sequence from zero, then (g0 + g1) + (g2 + g3)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if order == 0:
            acc = g[0].copy()
            for s in range(1, g.shape[0]):
                acc = acc + g[s]
            return acc
        a = [np.zeros_like(g[0]) for _ in range(4)]
        for s in range(g.shape[0]):
            a[s % 4] = a[s % 4] + g[s]
        return (a[0] + a[1]) + (a[2] + a[3])


def norms(x):
    """(sumsq, absmax, nonfinite, finite count) of a vector, over its finite elements, in float64."""
    d = x.astype(np.float64)
    ok = np.isfinite(d)
    f = d[ok]
    return math.fsum(f * f), float(np.abs(f).max()) if f.size else 0.0, int((~ok).sum()), int(ok.sum())


def vec(g, param, gscale=1.0, order=0):
    """One segment: g [nsplit][n], param [n] in the element type -> (grad norms, param norms)."""
    with np.errstate(invalid="ignore", over="ignore"):
        gi = sum_copies(g, order) * g.dtype.type(gscale)
    return norms(gi), norms(param)


def rows(q, y, qa, r, a_off=0.0, qn=None, done=None, gamma=0.0):
    """One column's row fields from [B] arrays (done [B][w]) -> ({field: value}, {field: tolerance})."""
    q64, y64, a64, r64 = (np.asarray(v).astype(np.float64) for v in (q, y, qa, r))
    ok = np.isfinite(q64) & np.isfinite(y64) & np.isfinite(a64)
    n = int(ok.sum())
    e = q64[ok] - y64[ok]
    out, tol = {}, {}

    def mean(name, terms, off=None):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.float64(math.fsum(terms)) / np.float64(n)
            v = m if off is None else np.float64(off) - m
        out[name] = float(v)
        # the sum's bound over n, plus one rounding each for the division (and the subtraction)
        tol[name] = (n * U * math.fsum(np.abs(terms)) / n + 2 * U * abs(float(m)) + (U * abs(float(v)) if off is not None else 0.0)
                     if n else 0.0)

    mean("loss_q", e * e)
    mean("loss_a", a64[ok], off=a_off)
    for name, v in (("q", q64[ok]), ("y", y64[ok]), ("r", r64[ok])):
        mean(name + "_mean", v)
        out[name + "_min"] = float(v.min()) if n else math.inf
        out[name + "_max"] = float(v.max()) if n else -math.inf
    out["td_absmax"] = float(np.abs(e).max()) if n else 0.0
    if qn is None:
        out["pre_min"] = out["pre_max"] = math.nan
    else:
        # float, in the TD head's operation order: (gamma * Q') * (1 - any done)
        f32 = np.float32
        any_done = (np.asarray(done) == 1).reshape(len(q), -1).any(axis=1).astype(f32)
        with np.errstate(invalid="ignore", over="ignore"):
            pre = (f32(gamma) * np.asarray(qn, dtype=f32)) * (f32(1.0) - any_done)
        pre = pre[ok]
        pre = pre[~np.isnan(pre)]
        out["pre_min"] = float(pre.min()) if pre.size else math.inf
        out["pre_max"] = float(pre.max()) if pre.size else -math.inf
    out["rows_nonfinite"] = float((~ok).sum())
    return out, tol


def record_row(rowfields, rowtol, nets):
    """A column's record [FIELDS] and tolerance [FIELDS] from ``rows``' output and
    nets = {"critic": (grad norms, param norms), "actor": ...} (``vec``'s output; missing = zeros)."""
    rec, tol = np.zeros(FIELDS), np.zeros(FIELDS)
    for k, v in rowfields.items():
        rec[F[k]] = v
        tol[F[k]] = rowtol.get(k, 0.0)
    for net in ("critic", "actor"):
        for what, nm in zip(("grad", "param"), nets.get(net, ((0.0, 0.0, 0, 0), (0.0, 0.0, 0, 0)))):
            ss, mx, nf, cnt = nm
            rec[F[f"{net}_{what}_sumsq"]], tol[F[f"{net}_{what}_sumsq"]] = ss, cnt * U * ss
            rec[F[f"{net}_{what}_absmax"]] = mx
            rec[F[f"{net}_{what}_nonfinite"]] = nf
    return rec, tol


def is_bad(rec):
    """Whether a record [A][FIELDS] sets the sticky word."""
    return bool((np.asarray(rec)[..., list(COUNT_FIELDS)] != 0).any())


class Aggregates:
    """The running aggregates' sequential fold: every finite field value, in update order."""

    def __init__(self, A):
        self.a = np.zeros((5, A, FIELDS))
        self.a[3], self.a[4] = math.inf, -math.inf

    def add(self, rec):
        ok = np.isfinite(rec)
        v = np.where(ok, rec, 0.0)
        self.a[0] += ok
        self.a[1] = np.where(ok, self.a[1] + v, self.a[1])
        self.a[2] = np.where(ok, self.a[2] + v * v, self.a[2])
        self.a[3] = np.where(ok, np.fmin(self.a[3], v), self.a[3])
        self.a[4] = np.where(ok, np.fmax(self.a[4], v), self.a[4])


def close(got, want, tol):
    """got within tol of want, elementwise; equal NaN / infinities count as equal."""
    got, want, tol = np.broadcast_arrays(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64),
                                         np.asarray(tol, dtype=np.float64))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        near = np.abs(got - want) <= tol
    return same | near
