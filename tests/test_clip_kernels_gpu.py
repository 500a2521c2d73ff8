"""aac_clip_sumsq and aac_adam_flat_clip called directly (include/aac_clip.h), float and double, every
operand carved from a poisoned arena (tests/arena.py): the element-type operands from one, the partials
and the record (doubles) from a second.

Lengths, from the kernels' constants (V = elements per 16 bytes: 4 float, 2 double): 1, 63, 64, 65, 255;
1000 (a ragged last Adam workgroup of 256 elements); THREADS * V + 1 (float 1025 = CHUNK + 1: the smallest
n with P = 2 partials, its second workgroup ragged -- a float chunk is one trip of the workgroup, so no
float sumsq thread takes a second one; double 513: a sumsq thread's second trip); CHUNK + 1 = 1025 (P = 2
for double too); 3 * CHUNK + 77 (P = 4, a ragged last chunk); ADAM_MAX_WG * THREADS + 257 (an Adam thread's second grid-stride trip, and P = 257: a
thread's second trip over the partials).

Tolerances: the norm against numpy float64 at 1e-12 relative (squares of float32 are exact in float64, so
only the order of the double additions differs).  p / m / v against the float64 restatement
(tests/clip_ref.py) as tests/test_adam_fold_gpu.py holds the unclipped kernels to torch: float p at atol
1e-6 with eps 1e-3, double p at rtol 1e-12 / atol 1e-14 with eps 1e-8.  m and v at 4 ulp of the larger
operand (2^-22 float, 2^-50 double): their expressions are three and four operations of the element type,
and exp_avg = b1 m + (1 - b1) g cancels in single elements, so the error is an ulp of the operands, not of
the result (the fold test's rtol 1e-13 on its 257 elements is the same bound without such an element).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import clip_ref
from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2 = 1e-3, 0.9, 0.999
STEP, STEP_ADD = 3, 2
LENGTHS = [1, 63, 64, 65, 255, 1000]
vp = ctypes.c_void_p


def _v(dt):
    return 4 if dt == torch.float32 else 2


def _eps(dt):
    return 1e-3 if dt == torch.float32 else 1e-8


def _npdt(dt):
    return np.float32 if dt == torch.float32 else np.float64


class Problem:
    """One job's operands.  layout: "aligned" (every copy and segment on the 16-byte grid: the 16-byte
    path), "offgrid" (every base one element off it: the scalar path), "oddstride" (aligned bases, odd
    segment and copy strides: segments on either path)."""

    def __init__(self, dt, n, ns=1, nseg=1, layout="aligned", seed=0, nan_at=None, out=True):
        from multi_agent_aac_amd import clip
        V = _v(dt)
        self.dt, self.n, self.ns, self.nseg, self.f64 = dt, n, ns, nseg, dt == torch.float64
        up = (n + V - 1) // V * V
        if layout == "oddstride":
            ss = n + 3 if (n + 3) % 2 else n + 4
            gs = nseg * ss + (1 if (nseg * ss) % 2 == 0 else 2)
        else:
            ss, gs = up + V, nseg * (up + V) + 2 * V
        self.ss, self.gs = ss, gs                        # seg_stride > n, gstride > the segments' span
        mis = 1 if layout == "offgrid" else 0
        span1 = (nseg - 1) * ss + n
        gspan = (ns - 1) * gs + span1
        self.P = clip.partials(n)
        self.ar = Arena(gspan + 4 * span1 + 6 * 64, dt, DEV, max_ld=max(ss, 64) if nseg > 1 else 64)
        self.aux = Arena(nseg * (self.P + clip.RECORD) + 4 * 64, torch.float64, DEV, max_ld=64)
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dt)     # noqa: E731
        self.copies = r(ns, nseg, n) * 1e-2
        if nan_at is not None:
            self.copies[nan_at] = float("nan")
        self.p0, self.m0, self.v0 = r(nseg, n), r(nseg, n) * 1e-2, r(nseg, n).abs() * 1e-4
        self.G = self.ar.take(1, gspan, misalign=mis, name="g", payload=False)
        self.Gc = [self.G.carve(s * gs, nseg, n, ld=ss, name=f"g copy {s}", data=self.copies[s]) for s in range(ns)]
        box = lambda name: self.ar.take(1, span1, misalign=mis, name=name, payload=False)       # noqa: E731
        self.p = box("p").carve(0, nseg, n, ld=ss, name="param", data=self.p0)
        self.m = box("m").carve(0, nseg, n, ld=ss, name="exp_avg", data=self.m0)
        self.v = box("v").carve(0, nseg, n, ld=ss, name="exp_avg_sq", data=self.v0)
        self.gout = box("gout").carve(0, nseg, n, ld=ss, name="grad_out") if out else None
        self.part = self.aux.take(nseg, self.P, name="partials")
        self.rec = self.aux.take(nseg, clip.RECORD, name="record", data=torch.zeros(nseg, clip.RECORD))
        self.step_t = torch.full((1,), STEP, dtype=torch.int32, device=DEV)

    def job(self, order, gscale, max_norm):
        """The job of both launches, its extents asserted to lie inside the arenas (without a grad_out the
        Adam launch reads g itself: ns == 1)."""
        from multi_agent_aac_amd import _native
        j = _native.ClipJob()
        j.g, j.grad_out = self.G.ptr, (self.gout.ptr if self.gout is not None else None)
        j.param, j.exp_avg, j.exp_avg_sq = self.p.ptr, self.m.ptr, self.v.ptr
        j.step, j.partials, j.record = self.step_t.data_ptr(), self.part.ptr, self.rec.ptr
        j.n, j.gstride, j.seg_stride = self.n, self.gs, self.ss
        j.nsplit, j.nseg, j.order, j.step_add = self.ns, self.nseg, order, STEP_ADD
        j.gscale, j.max_norm = gscale, max_norm
        j.lr, j.beta1, j.beta2, j.eps = LR, B1, B2, _eps(self.dt)
        span1 = (self.nseg - 1) * self.ss + self.n
        self.ar.inside(j.g, (self.ns - 1) * self.gs + span1, "g")
        for ptr in (j.grad_out, j.param, j.exp_avg, j.exp_avg_sq):
            self.ar.inside(ptr, span1)
        self.aux.inside(j.partials, self.nseg * self.P, "partials")
        self.aux.inside(j.record, self.rec.rows * self.rec.cols, "record")
        return j

    def norms(self):
        """sqrt of each segment's partials summed in numpy (float64)."""
        return np.sqrt(self.part.get().numpy().sum(1))


def _launch(name, jobs, f64):
    from multi_agent_aac_amd import clip
    clip.Launch(name, jobs, f64)()


def _ref(pb, order, gscale, max_norm, records=None):
    """The restatement per segment: (grad_out, norm, coef, p, m, v) lists."""
    out = []
    for k in range(pb.nseg):
        out.append(clip_ref.clip_adam(pb.copies[:, k].numpy(), order, gscale, max_norm, pb.p0[k].numpy(), pb.m0[k].numpy(),
                                      pb.v0[k].numpy(), STEP + STEP_ADD, lr=LR, b1=B1, b2=B2, eps=_eps(pb.dt),
                                      record=None if records is None else records[k]))
    return out


def _bound(pb, order, gscale, kind):
    """max_norm below every segment's norm, above every one, or inf -- from the numpy norms."""
    if kind == "inf":
        return math.inf
    norms = [r[1] for r in _ref(pb, order, gscale, math.inf)]
    return 0.5 * min(norms) if kind == "below" else 2.0 * max(norms)


def _run_checked(pb, order, gscale, max_norm):
    """Both launches with every arena check between; returns the device results and the record."""
    j = pb.job(order, gscale, max_norm)
    _launch("aac_clip_sumsq", [j], pb.f64)
    outs = [pb.gout] if pb.gout is not None else []
    pb.ar.check(writable=outs)                        # inputs untouched, grad_out written in full
    pb.aux.check(writable=[pb.part])                  # every partial written, the record untouched
    pb.ar.freeze(outs)
    pb.aux.freeze([pb.part])
    norms = pb.norms()
    _launch("aac_adam_flat_clip", [j], pb.f64)
    pb.ar.check(writable=[pb.p, pb.m, pb.v])          # grad_out and the copies are inputs now
    pb.aux.check(writable=[pb.rec])
    assert int(pb.step_t.item()) == STEP
    return norms


def _compare(pb, order, gscale, max_norm, norms):
    recs = [clip_ref.new_record() for _ in range(pb.nseg)]
    ref = _ref(pb, order, gscale, max_norm, recs)
    got = {k: getattr(pb, k).get().double().numpy() for k in "pmv"}
    rec = pb.rec.get().numpy()
    dt = _npdt(pb.dt)
    for k, (g, norm, coef, p, m, v) in enumerate(ref):
        print(f"seg {k}: norm {norms[k]!r} ref {norm!r} coef {rec[k, 4]!r} ref {coef!r}")
        if math.isnan(norm):
            assert math.isnan(norms[k]) and math.isnan(rec[k, 3]) and math.isnan(rec[k, 4])
            assert np.isnan(got["p"][k]).all()
            assert list(rec[k, :3]) == [1, 0, 1] and rec[k, 5] == 0.0
            continue
        np.testing.assert_allclose(norms[k], norm, rtol=1e-12, atol=0)
        np.testing.assert_allclose(rec[k, 3], norm, rtol=1e-12, atol=0)
        if pb.gout is not None:
            assert np.array_equal(pb.gout.get().numpy()[k].view(np.uint8), g.view(np.uint8)), "grad_out bits"
        # the record: counters exact, coef from the device's own norm exact
        assert rec[k, 0] == 1 and rec[k, 1] == int(clip_ref.coef_of(rec[k, 3], max_norm) < 1.0) and rec[k, 2] == 0
        assert rec[k, 1] == recs[k]["clipped"]
        assert rec[k, 4] == clip_ref.coef_of(rec[k, 3], max_norm) and rec[k, 5] == rec[k, 3]
        ga = np.abs(g.astype(np.float64) * dt(gscale) * coef)
        ulp4 = 2.0 ** -50 if pb.f64 else 2.0 ** -22
        if pb.f64:
            np.testing.assert_allclose(got["p"][k], p, rtol=1e-12, atol=1e-14)
        else:
            np.testing.assert_allclose(got["p"][k], p, rtol=0, atol=1e-6)
        np.testing.assert_allclose(got["m"][k], m, rtol=0, atol=ulp4 * max(np.abs(pb.m0[k].numpy()).max(), ga.max()))
        np.testing.assert_allclose(got["v"][k], v, rtol=0, atol=ulp4 * max(np.abs(pb.v0[k].numpy()).max(), (ga * ga).max()))


def _lengths(dt):
    from multi_agent_aac_amd import clip
    return LENGTHS + [clip.THREADS * _v(dt) + 1, clip.CHUNK + 1, 3 * clip.CHUNK + 77]


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("k", range(9))
def test_lengths(native_lib, dt, k):
    n = _lengths(dt)[k]
    pb = Problem(dt, n, ns=2, seed=n)
    mx = _bound(pb, 1, 1.0, "below")
    _compare(pb, 1, 1.0, mx, _run_checked(pb, 1, 1.0, mx))
    assert pb.P == (n + clip_ref.CHUNK - 1) // clip_ref.CHUNK and (pb.P >= 2) == (n > clip_ref.CHUNK)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", ["aligned", "offgrid", "oddstride"])
@pytest.mark.parametrize("nseg", [1, 3, 8])
@pytest.mark.parametrize("ns", [1, 2, 5])
def test_layouts(native_lib, dt, ns, nseg, layout):
    """Copies and segments at strides > n on the 16-byte grid, one element off it and at odd strides, both
    copy orders, at the sumsq second-trip length; gscale and the bound cycle over the cases."""
    from multi_agent_aac_amd import clip
    n = clip.THREADS * _v(dt) + 1
    case = ns + nseg + len(layout)
    gscale = (1.0, 0.5)[case % 2]
    kind = ("below", "above", "inf")[(ns * 3 + nseg) % 3]
    for order in (0, 1):
        pb = Problem(dt, n, ns=ns, nseg=nseg, layout=layout, seed=case)
        mx = _bound(pb, order, gscale, kind)
        _compare(pb, order, gscale, mx, _run_checked(pb, order, gscale, mx))
        rec = pb.rec.get().numpy()
        assert (rec[:, 1] == (1 if kind == "below" else 0)).all()


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["below", "above", "inf"])
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_values_runs_and_counters(native_lib, dt, gscale, kind):
    """gscale x bound, P = 5, three segments of five copies: two runs bit-equal, and a second clipped step
    on the same operands advances the counters by one and keeps max_norm_seen."""
    pbs = []
    for rep in range(2):
        pb = Problem(dt, 5000, ns=5, nseg=3, seed=5)
        mx = _bound(pb, 1, gscale, kind)
        norms = _run_checked(pb, 1, gscale, mx)
        if rep == 0:
            _compare(pb, 1, gscale, mx, norms)
        pbs.append(pb)
    a, b = pbs
    it = torch.int32 if dt == torch.float32 else torch.int64
    for x, y in ((a.p, b.p), (a.m, b.m), (a.v, b.v), (a.gout, b.gout)):
        assert torch.equal(x.get().view(it), y.get().view(it))
    for x, y in ((a.part, b.part), (a.rec, b.rec)):
        assert torch.equal(x.get().view(torch.int64), y.get().view(torch.int64))
    first = a.rec.get().numpy().copy()
    j = a.job(1, gscale, mx)
    _launch("aac_clip_sumsq", [j], a.f64)
    _launch("aac_adam_flat_clip", [j], a.f64)
    a.aux.check(writable=[a.part, a.rec])
    rec = a.rec.get().numpy()
    assert (rec[:, 0] == 2).all() and (rec[:, 1] == 2 * first[:, 1]).all() and (rec[:, 2] == 0).all()
    assert np.array_equal(rec[:, 3:], first[:, 3:])          # the gradient did not change


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_nan_element_counts_nonfinite(native_lib, dt):
    """One NaN in segment 1 of 3: that unit's norm, coef and parameters go NaN and nonfinite advances; the
    other units are untouched by it."""
    pb = Problem(dt, 300, ns=2, nseg=3, seed=9, nan_at=(1, 1, 17))
    norms = _run_checked(pb, 0, 1.0, 0.01)
    _compare(pb, 0, 1.0, 0.01, norms)
    rec = pb.rec.get().numpy()
    assert list(rec[:, 2]) == [0, 1, 0] and list(rec[:, 1]) == [1, 0, 1]


def test_adam_second_trip(native_lib):
    """n = ADAM_MAX_WG * THREADS + 257: the Adam grid is capped, so the first 257 threads take a second
    grid-stride trip; one copy read in place (no grad_out); P = 257 partials, so thread 0 of every
    workgroup folds two of them."""
    from multi_agent_aac_amd import clip
    n = clip.ADAM_MAX_WG * clip.THREADS + 257
    pb = Problem(torch.float32, n, ns=1, seed=2, out=False)
    assert pb.P == clip.THREADS + 1
    mx = _bound(pb, 0, 1.0, "below")
    _compare(pb, 0, 1.0, mx, _run_checked(pb, 0, 1.0, mx))


def _fused_state(pb):
    """Fresh device copies of the problem's state as one contiguous segment (nseg == 1)."""
    from types import SimpleNamespace
    p, m, v = (x[0].clone().to(DEV) for x in (pb.p0, pb.m0, pb.v0))
    gout = torch.zeros_like(p)
    step_t = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
    opt = SimpleNamespace(flat=SimpleNamespace(data=p, grad=gout), exp_avg=m, exp_avg_sq=v, lr=LR, betas=(B1, B2),
                          eps=_eps(pb.dt), step_t=step_t)
    return opt


@pytest.mark.parametrize("layout", ["aligned", "oddstride"])
@pytest.mark.parametrize("ns", [1, 2, 5, 20])
@pytest.mark.parametrize("n", [65, 1025, 5000])
def test_inf_bound_is_the_unclipped_kernels_bits(native_lib, n, ns, layout):
    """max_norm = inf (coef = 1): p / m / v / grad_out bit-equal to aac_adam_flat_sum_strided (gscale 1)
    and to aac_sum_partials_strided + aac_adam_flat_at_scaled (gscale 0.5) on the same copies, in the
    order those kernels take for them (monitor.adam4_order: the four-group order on 16-byte aligned
    copies, the plain order otherwise)."""
    from multi_agent_aac_amd import fused
    from multi_agent_aac_amd.monitor import adam4_order
    for gscale in (1.0, 0.5):
        pb = Problem(torch.float32, n, ns=ns, layout=layout, seed=n + ns)
        gpart = torch.as_strided(pb.ar.buf, (ns, pb.gs), (pb.gs, 1), pb.G.base) if ns > 1 else \
            torch.as_strided(pb.ar.buf, (1, n), (n, 1), pb.G.base)
        order = adam4_order(gpart, ns)
        assert order == (1 if layout == "aligned" and ns > 1 else 0)
        _run_checked(pb, order, gscale, math.inf)
        opt = _fused_state(pb)
        if gscale == 1.0:
            fused.adam_sum(opt, gpart, ns, STEP_ADD, grad_out=opt.flat.grad)
        else:
            fused._chk(fused.lib().aac_sum_partials_strided(vp(opt.flat.grad.data_ptr()), vp(gpart.data_ptr()), ns,
                                                            gpart.shape[-1], n, fused._stream()), "sum_partials")
            fused.adam_at(opt, STEP_ADD, gscale)
        torch.cuda.synchronize()
        for mine, theirs, what in ((pb.p, opt.flat.data, "param"), (pb.m, opt.exp_avg, "exp_avg"),
                                   (pb.v, opt.exp_avg_sq, "exp_avg_sq"), (pb.gout, opt.flat.grad, "grad_out")):
            assert torch.equal(mine.get()[0].view(torch.int32), theirs.cpu().view(torch.int32)), (what, gscale)
        assert pb.rec.get().numpy()[0, 4] == 1.0


@pytest.mark.parametrize("ns", [1, 3])
def test_inf_bound_is_adam64_bits(native_lib, ns):
    """The double instantiation at coef = 1 against aac_adam64_sum_scaled (copies n apart, plain order)."""
    from multi_agent_aac_amd import _native, clip, fused
    from multi_agent_aac_amd import uam_learner as L
    n, F64 = 1027, torch.float64
    g = torch.Generator().manual_seed(ns)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    parts, p0, m0, v0 = (r(ns, n) * 1e-2).to(DEV), r(n), r(n) * 1e-2, r(n).abs() * 1e-4
    for gscale in (1.0, 0.5):
        mine, theirs = [[x.clone().to(DEV) for x in (p0, m0, v0)] for _ in range(2)]
        st = torch.full((1,), STEP, dtype=torch.int32, device=DEV)
        gout = torch.zeros(n, dtype=F64, device=DEV)
        part = torch.zeros(clip.partials(n), dtype=F64, device=DEV)
        rec = torch.zeros(clip.RECORD, dtype=F64, device=DEV)
        j = clip.job(parts, *mine, st, part, rec, n, math.inf, LR, (B1, B2), 1e-8, nsplit=ns, gstride=n, order=0,
                     grad_out=gout, step_add=STEP_ADD, gscale=gscale)
        clip.Launch("aac_clip_sumsq", [j], True)()
        clip.Launch("aac_adam_flat_clip", [j], True)()
        L._ok(L._learn_lib().aac_adam64_sum_scaled(vp(theirs[0].data_ptr()), vp(parts.data_ptr()), ns,
                                                   vp(theirs[1].data_ptr()), vp(theirs[2].data_ptr()), n, LR, B1, B2, 1e-8,
                                                   vp(st.data_ptr()), STEP_ADD, gscale, fused._stream()), "adam64")
        torch.cuda.synchronize()
        for a, b in zip(mine, theirs):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), gscale
        assert _native.lib().aac_clip_partials(n) == clip.partials(n)


@pytest.mark.parametrize("swap", [False, True])
def test_two_job_launches_equal_lone_launches(native_lib, swap):
    """A one-element job beside three 5000-element segments in one launch, in both orders: bit-equal to
    the lone launches, every arena intact."""
    specs = [dict(n=1, ns=4, nseg=1, seed=1), dict(n=5000, ns=5, nseg=3, seed=2)]
    if swap:
        specs.reverse()
    lone, both = [], []
    for group in (lone, both):
        for s in specs:
            group.append(Problem(torch.float32, **s))
    bounds = [_bound(pb, 1, 1.0, "below") for pb in lone]
    for pb, mx in zip(lone, bounds):
        _run_checked(pb, 1, 1.0, mx)
    jobs = [pb.job(1, 1.0, mx) for pb, mx in zip(both, bounds)]
    _launch("aac_clip_sumsq", jobs, False)
    for pb in both:
        pb.ar.check(writable=[pb.gout])
        pb.aux.check(writable=[pb.part])
        pb.ar.freeze([pb.gout])
        pb.aux.freeze([pb.part])
    _launch("aac_adam_flat_clip", jobs, False)
    for pb, ref in zip(both, lone):
        pb.ar.check(writable=[pb.p, pb.m, pb.v])
        pb.aux.check(writable=[pb.rec])
        for x, y in ((pb.p, ref.p), (pb.m, ref.m), (pb.v, ref.v), (pb.gout, ref.gout)):
            assert torch.equal(x.get().view(torch.int32), y.get().view(torch.int32))
        for x, y in ((pb.part, ref.part), (pb.rec, ref.rec)):
            assert torch.equal(x.get().view(torch.int64), y.get().view(torch.int64))


def test_bad_jobs_are_refused(native_lib):
    from multi_agent_aac_amd import _native, clip
    pb = Problem(torch.float32, 100, ns=2, seed=1)
    L = _native.lib()
    for field, value, where in (("n", 0, "n, nsplit"), ("order", 2, "order"), ("gstride", 50, "copy stride"),
                                ("max_norm", -1.0, "max_norm"), ("partials", None, "partials")):
        j = pb.job(0, 1.0, 1.0)
        setattr(j, field, value)
        arr = (_native.ClipJob * 1)(j)
        assert L.aac_adam_flat_clip(arr, 1, 0, None) != 0
        assert where in L.aac_clip_last_error().decode()
    assert L.aac_clip_sumsq((_native.ClipJob * 1)(pb.job(0, 1.0, 1.0)), 3, 0, None) != 0
    torch.cuda.synchronize()
    pb.ar.check()
    pb.aux.check()
    assert clip.partials(100) == 1
