"""The learner monitor's kernels (include/aac_monitor.h) against tests/monitor_ref.py.

Bounds (derived, not measured): non-finite counts, maxima and minima are exact / bit-equal; a double sum
of ``count`` terms formed in any order lies within ``count * 2^-53 * sum|terms|`` of the exact sum, which
the restatement forms with math.fsum; a mean adds the roundings of its division (monitor_ref.rows)."""
import itertools
import math

import numpy as np
import pytest
import torch

import monitor_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NS = [1, 3, 255, 256, 257, 4100]
KINDS = ["random", "zero", "nan0", "inf_last", "inf_pair"]


def _values(rng, shape, dt):
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)).astype(dt)


def _vec_case(rng, dt, n, nsplit, gmode, nseg, off, gscale, kind, order):
    """Host buffers, the job and the per-segment expectation of one vec job."""
    seg_stride = n if gmode == 0 else n + 3
    width = nseg * seg_stride
    gstride = width if gmode == 0 else (width + 63) // 64 * 64 + 8        # == n, or rounded up to 64 plus padding
    g = np.zeros((nsplit, gstride), dtype=dt)
    p = np.zeros(width, dtype=dt)
    if kind != "zero":
        g[:] = _values(rng, g.shape, dt)
        p[:] = _values(rng, p.shape, dt)
    if kind == "nan0":
        g[0, 0] = p[0] = np.nan
    elif kind == "inf_last":
        g[nsplit - 1, (nseg - 1) * seg_stride + n - 1] = np.inf
        p[(nseg - 1) * seg_stride + n - 1] = -np.inf
    elif kind == "inf_pair":        # +Inf and -Inf in two copies of one middle element: their sum is NaN
        g[0, n // 2], g[nsplit - 1, n // 2] = np.inf, -np.inf
    want = [monitor_ref.vec(g[:, s * seg_stride:s * seg_stride + n], p[s * seg_stride:s * seg_stride + n], gscale, order)
            for s in range(nseg)]
    job = dict(n=n, nsplit=nsplit, gstride=gstride, nseg=nseg, seg_stride=seg_stride, order=order, gscale=gscale,
               g_off=off, p_off=off)
    return g, p, job, want


def _upload(a, off):
    """The array on the device, ``off`` elements past a 16-byte boundary."""
    t = torch.zeros(a.size + 4, dtype=torch.from_numpy(a).dtype, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[off:off + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
    return t


def _check_vec(scratch, col0, net, want, ctx):
    for s, (gw, pw) in enumerate(want):
        slots = scratch[col0 + s, net]                        # [64][6]
        for k, (ss, mx, nf, cnt) in ((0, gw), (3, pw)):
            got_ss, got_mx, got_nf = math.fsum(slots[:, k]), slots[:, k + 1].max(), slots[:, k + 2].sum()
            assert got_nf == nf, (ctx, s, k, got_nf, nf)
            assert got_mx == mx, (ctx, s, k, got_mx, mx)
            # count terms in the kernel's fold, 64 more roundings where the test folds the slots exactly
            assert abs(got_ss - ss) <= cnt * U * ss, (ctx, s, k, got_ss, ss)


@pytest.mark.parametrize("dt,nsplit,order", [(np.float32, 1, 0), (np.float32, 4, 0), (np.float32, 4, 1),
                                             (np.float32, 20, 0), (np.float32, 20, 1), (np.float64, 1, 0),
                                             (np.float64, 4, 0), (np.float64, 20, 0)])
def test_vec(native_lib, dt, nsplit, order):
    from multi_agent_aac_amd import monitor
    rng = np.random.default_rng(1234 + nsplit + 7 * order)
    tdt = torch.float32 if dt == np.float32 else torch.float64
    mon = monitor.LearnerMonitor(4, ring=2, dtype=tdt)
    kinds = [k for k in KINDS if not (k == "inf_pair" and nsplit == 1)]
    prev = None
    for n, gmode, nseg, off, gscale, kind in itertools.product(NS, (0, 1), (1, 3), (0, 1), (1.0, 0.5), kinds):
        g, p, job, want = _vec_case(rng, dt, n, nsplit, gmode, nseg, off, gscale, kind, order)
        gt, pt = _upload(g, off), _upload(p, off)
        ctx = (n, gmode, nseg, off, gscale, kind)
        # one job per launch (net 1, from column 1 where it fits)
        mon.scratch.fill_(-1.0)
        col0 = 4 - nseg
        mon.vec((gt, pt, dict(job, net=1, col0=col0)))()
        _check_vec(mon.scratch.cpu().numpy(), col0, 1, want, ctx)
        # two jobs per launch: this case beside the previous one
        if prev is not None:
            mon.scratch.fill_(-1.0)
            (g0, p0, job0, want0, ctx0) = prev
            mon.vec((g0, p0, dict(job0, net=0, col0=0)), (gt, pt, dict(job, net=1, col0=col0)))()
            sc = mon.scratch.cpu().numpy()
            _check_vec(sc, 0, 0, want0, ("pair0",) + ctx0)
            _check_vec(sc, col0, 1, want, ("pair1",) + ctx)
            prev = None
        else:
            prev = (gt, pt, job, want, ctx)


def test_vec_rejects_bad_jobs(native_lib):
    from multi_agent_aac_amd import monitor
    mon = monitor.LearnerMonitor(2, ring=2)
    t = torch.zeros(64, device="cuda")
    with pytest.raises(RuntimeError, match="col0"):
        mon.vec((t, t, dict(n=8, net=0, col0=1, nseg=2, seg_stride=8)))()
    with pytest.raises(RuntimeError, match="stride"):
        mon.vec((t, t, dict(n=8, net=0, nsplit=2, gstride=4)))()
    with pytest.raises(ValueError):
        mon.vec((t.double(), t, dict(n=8, net=0)))


# ----------------------------------------------------------------------------------------- commit
def _commit_case(rng, A, B, layout, with_qn, nan, dt):
    """Host row fields [A][B] (the restatement's view), device tensors in ``layout`` and the rows dict."""
    f = {k: rng.normal(0, 3, size=(A, B)).astype(dt) for k in ("q", "y", "q_a", "reward", "qn")}
    done = (rng.random((A, B, A)) < 0.2).astype(dt)
    if nan:
        f["q"][A - 1, B // 2] = np.nan
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    rows = {}
    for k in ("q", "y", "q_a"):
        t = dev(f[k] if layout == "cols" else f[k].T)                     # [A][B] or [B][A]
        rows[k] = (t, 0, B, 1) if layout == "cols" else (t, 0, 1, A)
    if layout == "cols":
        # the ATT reward array [A * B][A]: column c reads its own agent's entry
        r = rng.normal(0, 1, size=(A * B, A)).astype(dt)
        for c in range(A):
            r[c * B:(c + 1) * B, c] = f["reward"][c]
        rows["reward"] = (dev(r), 0, B * A + 1, A)
        if with_qn:
            rows["qn"] = (dev(f["qn"]), 0, B, 1)
            rows["done"] = (dev(done), 0, B * A, A)
    else:
        rows["reward"] = (dev(f["reward"].T), 0, 1, A)
        if with_qn:
            rows["qn"] = (dev(f["qn"].T), 0, 1, A)
            rows["done"] = (dev(done.transpose(1, 0, 2)), 0, A, A * A)
    return f, done, rows


def _expected(f, done, A, a_off, with_qn, gamma, scratch):
    rec, tol = np.zeros((A, len(monitor_ref.F))), np.zeros((A, len(monitor_ref.F)))
    for c in range(A):
        rf, rt = monitor_ref.rows(f["q"][c], f["y"][c], f["q_a"][c], f["reward"][c], a_off,
                                  f["qn"][c] if with_qn else None, done[c] if with_qn else None, gamma)
        nets = {}
        for i, net in enumerate(("critic", "actor")):
            sl = scratch[c, i]
            nets[net] = tuple((math.fsum(sl[:, k]), sl[:, k + 1].max(), sl[:, k + 2].sum(), 64) for k in (0, 3))
        rec[c], tol[c] = monitor_ref.record_row(rf, rt, nets)
    return rec, tol


def _scratch(rng, A, poison=False):
    s = rng.random((A, 2, 64, 6)) * 100
    s[..., 2] = s[..., 5] = 0
    if poison:
        s[0, 1, 17, 2] = 2.0
    return s


@pytest.mark.parametrize("B", [1, 5, 64, 257, 1024])
def test_commit_record(native_lib, B):
    from multi_agent_aac_amd import monitor
    rng = np.random.default_rng(99 + B)
    cases = [(A, lay, a_off, qn, nan, np.float32) for A, lay, a_off, qn, nan in
             itertools.product((1, 3, 5), ("cols", "rows"), (0.0, 3.0), (False, True), (False, True))]
    cases += [(1, lay, 0.0, qn, nan, np.float64) for lay, qn, nan in itertools.product(("cols", "rows"), (False, True),
                                                                                       (False, True))]
    for A, layout, a_off, with_qn, nan, dt in cases:
        mon = monitor.LearnerMonitor(A, ring=2, dtype=torch.float32 if dt == np.float32 else torch.float64)
        f, done, rows = _commit_case(rng, A, B, layout, with_qn, nan, dt)
        sc = _scratch(rng, A)
        mon.scratch.copy_(torch.from_numpy(sc))
        gamma = 0.95
        mon.commit(B, rows, a_off=a_off, gamma=gamma, done_width=A if with_qn else 0)()
        out = mon.read()
        want, tol = _expected(f, done, A, a_off, with_qn, gamma, sc)
        got = mon.ring.cpu().numpy()[0]
        ok = monitor_ref.close(got, want, tol)
        assert ok.all(), ((A, layout, a_off, with_qn, nan, dt), np.argwhere(~ok), got[~ok], want[~ok])
        assert out["updates"] == 1 and list(out["update"]) == [0]
        assert out["bad_update"] == (0 if nan else -1) == mon.bad_update()
        if nan:
            assert got[A - 1, monitor_ref.F["rows_nonfinite"]] == 1 and (B > 1 or np.isnan(got[A - 1, 0]))


def _sequence(rng_seed, steps=10, R=4, A=3, B=5, poisoned=(3, 5), extra_clean=True):
    """``steps`` commits of changing inputs (NaN in q at the poisoned ones); returns the monitor and the
    records read back after every commit."""
    from multi_agent_aac_amd import monitor
    rng = np.random.default_rng(rng_seed)
    mon = monitor.LearnerMonitor(A, ring=R)
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    q, y, qa, r = z(A, B), z(A, B), z(A, B), z(A, B)
    op = mon.commit(B, {"q": (q, 0, B, 1), "y": (y, 0, B, 1), "q_a": (qa, 0, B, 1), "reward": (r, 0, B, 1)}, a_off=3.0)
    recs = []
    for u in range(steps):
        for t in (q, y, qa, r):
            t.copy_(torch.from_numpy(rng.normal(0, 2, size=(A, B)).astype(np.float32)))
        if u in poisoned:
            q[1, 2] = math.nan
        mon.scratch.copy_(torch.from_numpy(_scratch(rng, A)))
        op()
        recs.append(mon.ring[u % R].cpu().numpy().copy())
    return mon, recs


def test_commit_sequence(native_lib):
    mon, recs = _sequence(5)
    out = mon.read()
    np.testing.assert_array_equal(out["update"], [6, 7, 8, 9])
    assert out["updates"] == 10
    for k, u in enumerate(range(6, 10)):
        for f, name in enumerate(monitor_ref.FIELD_NAMES):
            np.testing.assert_array_equal(out[name][k], recs[u][:, f])
    # the aggregates: the sequential fold of the records, in update order
    agg = monitor_ref.Aggregates(3)
    for rec in recs:
        agg.add(rec)
    np.testing.assert_array_equal(mon.agg.cpu().numpy(), agg.a)
    assert [monitor_ref.is_bad(r) for r in recs] == [u in (3, 5) for u in range(10)]
    assert mon.bad_update() == 3          # the first poisoned commit; later commits, clean or not, leave it
    with pytest.raises(FloatingPointError, match="update 3"):
        mon.check()
    mon.reset()
    assert mon.bad_update() == -1 and int(mon.state[0]) == 10
    out = mon.read()
    assert out["updates"] == 10 and len(out["update"]) == 0 and out["loss_q"].shape == (0, 3)
    assert (mon.ring_update.cpu().numpy() == -1).all() and float(mon.agg[0].sum()) == 0


def test_commit_sequences_are_reproducible(native_lib):
    a, _ = _sequence(11)
    b, _ = _sequence(11)
    for k, t in a.tensors().items():      # bit for bit (the records hold NaN where qn is not supplied)
        assert torch.equal(t.view(torch.int64), b.tensors()[k].view(torch.int64)), k
