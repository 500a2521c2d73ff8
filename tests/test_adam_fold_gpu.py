"""The Adam kernels' bias corrections come from wave 0 of each workgroup through LDS, behind one
workgroup barrier that every thread reaches after issuing its first loads (csrc/aac_adam_bc.h).
These tests walk the shapes at which that structure could go wrong: workgroups whose later waves
have no element (n = 1, 63, 65, 257: a wave past n must still arrive at the barrier), exact
multiples of the wave and the block, more than one block, the second grid-stride trip, both sides
of the pair launch with a one-element job, copy counts on both sides of the four copy groups, and
step counters from 1 to 100000 given through the step tensor, through step_add, and split between
the two.

Each summed form (the copy-parallel kernel, the element kernel, the pair launch) is held to
aac_adam_flat_at on the summed gradient it wrote, bit for bit; that one to torch's CPU Adam
(atol 1e-6; eps 1e-3 as test_adam_sum_matches_torch explains).  Every buffer carries a canary in
element n.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
vp = ctypes.c_void_p
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-3
CANARY = 12345.0
COUNTERS = [1, 2, 10, 1000, 100000]


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _guarded(x):
    """x on the device with one canary element behind it; (buffer of n + 1, view of n)."""
    buf = torch.cat([x.reshape(-1).float(), torch.tensor([CANARY])]).to(DEV)
    return buf, buf[:x.numel()]


class State:
    """One network's parameters, moments, gradient output and step tensor, each guarded."""

    def __init__(self, p0, m0, v0):
        n = p0.numel()
        self.n = n
        self.bufs = {}
        for name, x in (("p", p0), ("m", m0), ("v", v0), ("gout", torch.zeros(n))):
            self.bufs[name], view = _guarded(x)
            setattr(self, name, view)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.opt = SimpleNamespace(flat=SimpleNamespace(data=self.p, grad=self.gout), exp_avg=self.m,
                                   exp_avg_sq=self.v, lr=LR, betas=(B1, B2), eps=EPS, step_t=self.step_t)

    def bits(self):
        return [self.bufs[k].clone().view(torch.int32) for k in ("p", "m", "v")]

    def check_canaries(self):
        for k, b in self.bufs.items():
            assert float(b[self.n]) == CANARY, f"{k}[n] was written"


def _copies(n, ns, stride, seed):
    """[ns][stride] partial copies; columns >= n hold NaN (the copy-parallel kernel's 16-B loads read
    a whole group of four, and only the elements below n may count)."""
    g = torch.full((ns, stride), float("nan"))
    g[:, :n] = _rand((ns, n), seed) * 1e-2
    return g.to(DEV)


def _sum4_stride(n):
    from multi_agent_aac_amd import fused
    return fused.padded(n) + 4


def _elem_stride(n):
    s = n + 1
    return s if s % 4 else s + 1


def _flat_at(st, grad, step_add):
    """aac_adam_flat_at on ``grad`` with st's state."""
    from multi_agent_aac_amd import fused
    L = fused.lib()
    rc = L.aac_adam_flat_at(vp(st.p.data_ptr()), vp(grad.data_ptr()), vp(st.m.data_ptr()), vp(st.v.data_ptr()), st.n,
                            LR, B1, B2, EPS, vp(st.step_t.data_ptr()), step_add, fused._stream())
    assert rc == 0


def _torch_adam(p0, m0, v0, grad, t):
    """Step t of torch.optim.Adam on the CPU from the given moments."""
    p = p0.clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=EPS)
    p.grad = grad.clone()
    opt.step()                                   # creates the state in torch's own layout
    with torch.no_grad():
        p.copy_(p0)
    s = opt.state[p]
    s["exp_avg"].copy_(m0)
    s["exp_avg_sq"].copy_(v0)
    if torch.is_tensor(s["step"]):
        s["step"].fill_(t - 1)
    else:
        s["step"] = t - 1
    opt.step()
    return p.detach()


def _splits(t):
    """(step tensor, step_add) pairs for counter t: all in the tensor, all in step_add, and split."""
    out = [(t, 0), (0, t)]
    if t > 1:
        out.append((t - 1, 1))
    return out


def _fresh(n, seed):
    p0, m0, v0 = _rand((n,), seed), _rand((n,), seed + 1) * 1e-2, _rand((n,), seed + 2).abs() * 1e-4
    return p0, m0, v0


def _same(a, b, what):
    for x, y, k in zip(a.bits(), b.bits(), ("param", "exp_avg", "exp_avg_sq")):
        assert torch.equal(x, y), f"{what}: {k} differs"


@pytest.mark.parametrize("ns", [1, 2, 4, 20])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_adam_forms_shapes_and_counters(native_lib, n, ns):
    """fused.adam_sum through the copy-parallel kernel (ns > 1, copy stride % 4 == 0) and through the
    element kernel (odd copy stride, or ns = 1), fused.adam_sum_pair with this job on either side,
    and aac_adam_flat_at: per counter and per way of giving it, run to run bit-equal, each summed
    form bit-equal to aac_adam_flat_at on the gradient it summed, that within 1e-6 of torch."""
    from multi_agent_aac_amd import fused
    p0, m0, v0 = _fresh(n, 11 * n + ns)
    for t in COUNTERS:
        elem = _copies(n, ns, _elem_stride(n), 1000 * ns + n + t)
        quad = _copies(n, ns, _sum4_stride(n), 2000 * ns + n + t) if ns > 1 else None
        other = _copies(4100, 4, _sum4_stride(4100), 7) if ns > 1 else None
        ref_bits = {}
        for step, add in _splits(t):
            forms = {}
            for name, gpart in (("element", elem), ("copy-parallel", quad)):
                if gpart is None:
                    continue
                for rep in range(2):
                    st = State(p0, m0, v0)
                    st.step_t.fill_(step)
                    fused.adam_sum(st.opt, gpart, ns, add, grad_out=st.gout)
                    forms[(name, rep)] = st
            if ns > 1:
                for side in (0, 1):
                    st, ot = State(p0, m0, v0), State(*_fresh(4100, 5))
                    st.step_t.fill_(step)
                    ot.step_t.fill_(3)
                    a, b = (st.opt, quad, ns, add, st.gout), (ot.opt, other, 4, 1, ot.gout)
                    fused.adam_sum_pair(*((a, b) if side == 0 else (b, a)))
                    forms[("pair", side)] = st
                    forms[("pair-other", side)] = ot
            for (name, rep), st in forms.items():
                if name == "pair-other":
                    continue
                flat = State(p0, m0, v0)
                flat.step_t.fill_(step)
                _flat_at(flat, st.gout, add)
                torch.cuda.synchronize()
                _same(st, flat, f"{name} vs aac_adam_flat_at, t = {step} + {add}")
                for s in (st, flat):
                    s.check_canaries()
                    assert int(s.step_t.item()) == step           # the kernels only read the counter
                key = "element" if name == "element" else "quad"
                if key in ref_bits:                # the same counter however it is given, and run to run
                    for x, y in zip(ref_bits[key], st.bits()):
                        assert torch.equal(x, y), f"{name}: t = {step} + {add} differs from the first run"
                else:
                    ref_bits[key] = st.bits()
                    want = _torch_adam(p0, m0, v0, st.gout.cpu(), t)
                    np.testing.assert_allclose(st.p.cpu().numpy(), want.numpy(), rtol=0, atol=1e-6)
            if ns > 1:
                _same(forms[("pair-other", 0)], forms[("pair-other", 1)], "the pair's other job")
                forms[("pair-other", 0)].check_canaries()
                # the copy sum itself: the world > 1 path's aac_sum_partials gives the same bits
                summed = torch.empty(n, device=DEV)
                fused.sum_partials(summed, quad, ns)
                assert torch.equal(summed, forms[("copy-parallel", 0)].gout)
                np.testing.assert_allclose(summed.cpu().double(), quad[:, :n].double().sum(0).cpu(), rtol=1e-5, atol=1e-8)


def test_adam_sum4_second_trip(native_lib):
    """n = 8192 * 256 + 257, ns = 2: the copy-parallel kernel's grid is capped at 8192 workgroups of
    256 elements, so the first 257 elements' waves take a second trip (its loads are issued at the
    end of the first, after the barrier) and the last wave of that trip is ragged."""
    from multi_agent_aac_amd import fused
    n, ns = 8192 * 256 + 257, 2
    p0, m0, v0 = _fresh(n, 3)
    gpart = _copies(n, ns, _sum4_stride(n), 4)
    runs = []
    for rep in range(2):
        st = State(p0, m0, v0)
        st.step_t.fill_(6)
        fused.adam_sum(st.opt, gpart, ns, 4, grad_out=st.gout)
        runs.append(st)
    flat = State(p0, m0, v0)
    flat.step_t.fill_(10)
    _flat_at(flat, runs[0].gout, 0)
    torch.cuda.synchronize()
    _same(runs[0], runs[1], "run to run")
    _same(runs[0], flat, "copy-parallel vs aac_adam_flat_at")
    assert torch.equal(runs[0].gout, gpart[0, :n] + gpart[1, :n])
    for s in runs + [flat]:
        s.check_canaries()
    want = _torch_adam(p0, m0, v0, runs[0].gout.cpu(), 10)
    np.testing.assert_allclose(runs[0].p.cpu().numpy(), want.numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("first", [(1, 4), (4100, 20)], ids=["1-then-4100", "4100-then-1"])
def test_adam_pair_one_element_job(native_lib, first):
    """A one-element job beside a 4100-element job in one launch, in both orders: the one-element
    job's only workgroup has three waves with nothing to do.  Each job is bit-equal to its own lone
    launch and to aac_adam_flat_at on its summed gradient, at different counters."""
    from multi_agent_aac_amd import fused
    jobs = [first, (4100, 20) if first[0] == 1 else (1, 4)]
    data = [(_fresh(n, 31 + n), _copies(n, ns, _sum4_stride(n), 17 + n), ns, t) for (n, ns), t in zip(jobs, (7, 1000))]
    pair, lone, flat = [], [], []
    for (pmv, gpart, ns, t) in data:
        for group in (pair, lone, flat):
            st = State(*pmv)
            st.step_t.fill_(t - 2)
            group.append(st)
    fused.adam_sum_pair(*[(st.opt, gpart, ns, 2, st.gout) for st, (_, gpart, ns, _) in zip(pair, data)])
    for st, (_, gpart, ns, _) in zip(lone, data):
        fused.adam_sum(st.opt, gpart, ns, 2, grad_out=st.gout)
    for st, src in zip(flat, pair):
        _flat_at(st, src.gout, 2)
    torch.cuda.synchronize()
    for a, b, c, (pmv, _, _, t) in zip(pair, lone, flat, data):
        _same(a, b, "pair vs lone launch")
        _same(a, c, "pair vs aac_adam_flat_at")
        assert torch.equal(a.gout, b.gout)
        for s in (a, b, c):
            s.check_canaries()
        want = _torch_adam(*pmv, a.gout.cpu(), t)
        np.testing.assert_allclose(a.p.cpu().numpy(), want.numpy(), rtol=0, atol=1e-6)


@pytest.mark.parametrize("n", [1, 257])
def test_adam64_shapes_and_counters(native_lib, n):
    """aac_adam64_sum (config 5's float64 Adam) at one element and at a block plus one, three copies,
    every counter: float64 torch Adam at the rtol 1e-12 / atol 1e-14 of test_gemm64_layouts_gpu, run
    to run bit-equal, the canary behind every buffer intact."""
    from multi_agent_aac_amd import fused
    from multi_agent_aac_amd import uam_learner as L
    lib = L._learn_lib()
    F64, ns, eps = torch.float64, 3, 1e-8
    g = torch.Generator().manual_seed(n)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1   # noqa: E731
    p0, m0, v0, parts = r(n), r(n) * 0.1, r(n).abs() * 0.01, r(ns, n)
    gp = parts.to(DEV).contiguous()
    gsum = parts[0] + parts[1] + parts[2]
    for t in COUNTERS:
        first = None
        for step, add in _splits(t):
            bufs = [torch.cat([x, torch.tensor([CANARY], dtype=F64)]).to(DEV) for x in (p0, m0, v0)]
            st = torch.full((1,), step, dtype=torch.int32, device=DEV)
            L._ok(lib.aac_adam64_sum(vp(bufs[0].data_ptr()), vp(gp.data_ptr()), ns, vp(bufs[1].data_ptr()),
                                     vp(bufs[2].data_ptr()), n, LR, B1, B2, eps, vp(st.data_ptr()), add,
                                     fused._stream()), "adam64")
            torch.cuda.synchronize()
            got = [b.cpu() for b in bufs]
            assert all(float(b[n]) == CANARY for b in got) and int(st.item()) == step
            if first is None:
                first = got
                p = p0.clone().requires_grad_()
                opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=eps)
                p.grad = gsum.clone()
                opt.step()
                with torch.no_grad():
                    p.copy_(p0)
                s = opt.state[p]
                s["exp_avg"].copy_(m0)
                s["exp_avg_sq"].copy_(v0)
                if torch.is_tensor(s["step"]):
                    s["step"].fill_(t - 1)
                else:
                    s["step"] = t - 1
                opt.step()
                np.testing.assert_allclose(got[0][:n], p.detach(), rtol=1e-12, atol=1e-14)
                np.testing.assert_allclose(got[1][:n], s["exp_avg"], rtol=1e-13, atol=0)
                np.testing.assert_allclose(got[2][:n], s["exp_avg_sq"], rtol=1e-13, atol=0)
            else:
                for a, b in zip(first, got):
                    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
