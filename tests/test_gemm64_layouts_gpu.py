"""aac_gemm64_batch, aac_adam64_sum and aac_sum64_partials (include/aac_uam_learn.h) inside the
poisoned arena (tests/arena.py), against float64 torch at the 1e-12 of test_gemm64_products: ragged
16 x 16 tiles, every ld above its natural value, bases shifted by one double, ldc > N, an addend
with ldadd > N, the dual output, the ones column with split-K copies farther apart than a copy,
and one launch whose padding waves sit between a one-wave and a four-wave product.  Every case ends
in ``arena.check``: only the declared outputs changed, and they were written in full."""
import ctypes

import numpy as np
import pytest
import torch

from tests.arena import Arena
from tests.test_gemm_layouts_gpu import EPI, Product

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
ALL = ("A", "B", "C", "bias", "addend", "mask", "dvec", "C2", "cextra")


def P64(*a, **k):
    from multi_agent_aac_amd import uam_learner as L
    return Product(L.Gemm64Prob, *a, dtype=F64, **k)


def run64(products):
    """One aac_gemm64_batch launch; values, then every product's arena."""
    from multi_agent_aac_amd import fused
    from multi_agent_aac_amd import uam_learner as L
    for i, p in enumerate(products):
        p.ar.inside_prob(p.prob, i)
    arr = (L.Gemm64Prob * len(products))(*[p.prob for p in products])
    L._ok(L._learn_lib().aac_gemm64_batch(arr, len(products), fused._stream()), "gemm64")
    torch.cuda.synchronize()
    for i, p in enumerate(products):
        p.verify(f"(product {i}: M {p.M} N {p.N} K {p.K})")
    arenas = {id(p.ar): p.ar for p in products}
    for ar in arenas.values():
        ar.check(writable=[r for p in products if p.ar is ar for r in p.writable()])


def kw_of(M, N, K, ones=0, ks=1):
    """The planner's waves per tile (aac_uam_learn.hip: g_kw4_steps = 16, g_kw4_tiles = 1024)."""
    steps = ((K + 3) // 4 + ks - 1) // ks
    tiles = ((M + 15) // 16) * ((N + ones + 15) // 16) * ks
    return 4 if steps >= 16 and tiles <= 1024 else 1


@pytest.mark.parametrize("pad", [0, 1, 3], ids=["natural", "pad1", "pad3"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm64_layout_sweep(native_lib, ta, tb, pad):
    """M, N in {1, 15, 17, 33} x K in {1, 3, 5, 65, 513} (K >= 61: four waves per tile with the LDS
    reduction); the epilogue rotates through bias / addend (ldadd = N + pad) / masks / tanh / the
    dual output (C2 at C's ldc) / the ones column, alone and with 3 or 8 split-K copies whose stride
    exceeds the copy; every other product has all its bases shifted by one double."""
    i = ta * 2 + tb + 4 * pad
    n = 0
    for M in (1, 15, 17, 33):
        for N in (1, 15, 17, 33):
            for K in (1, 3, 5, 65, 513):
                epi = dict(EPI[i % len(EPI)])
                if epi.get("ones"):
                    ks = (1, 3, 8)[(i // len(EPI)) % 3]
                    epi.update(ksplit=ks, stride_extra=5 if ks > 1 else 0)
                shift = ALL if (i // 2) % 2 else ()
                i += 1
                n += 1
                run64([P64(M, N, K, ta=ta, tb=tb, pad=pad, seed=i, shift=shift, **epi)])
    assert n == 80


@pytest.mark.parametrize("pad", [0, 3])
def test_gemm64_padding_waves_between_one_wave_and_four_wave_products(native_lib, pad):
    """One launch, one arena: a product of six one-wave tiles (17 x 33 x 5), then a four-wave
    product (17 x 33 x 65) whose waves start at the next multiple of four -- waves 6 and 7 belong to
    no tile and must write nothing -- then a one-wave product again and a split-K four-wave one.
    Nothing outside the outputs may change."""
    ar = Arena(60000, F64, DEV, max_ld=600)
    specs = [dict(M=17, N=33, K=5, tb=1, bias=True, act=1), dict(M=17, N=33, K=65, ta=1, addend=True),
             dict(M=15, N=1, K=3, mact=2), dict(M=33, N=15, K=513, ta=1, ones=1, ksplit=2, stride_extra=7),
             dict(M=1, N=17, K=65, tb=1, bias=True, act=1, dual=True)]
    assert [kw_of(s["M"], s["N"], s["K"], s.get("ones", 0), s.get("ksplit", 1)) for s in specs] == [1, 4, 1, 4, 4]
    run64([P64(pad=pad, seed=20 + i, ar=ar, **s) for i, s in enumerate(specs)])


@pytest.mark.parametrize("ns", [1, 3, 9, 17])
@pytest.mark.parametrize("shift", [0, 1])
def test_adam64_and_sum64_in_the_arena(native_lib, ns, shift):
    """aac_sum64_partials and aac_adam64_sum over buffers carved from the arena, n = 333 (no multiple
    of the 256-thread block): the sum is the copies added in copy order (exact in float64: the same
    IEEE additions), Adam from non-zero moments at step 3 against the formula of the header in
    float64; nothing but out / param / exp_avg / exp_avg_sq changes."""
    from multi_agent_aac_amd import fused
    from multi_agent_aac_amd import uam_learner as L
    n = 333
    g = torch.Generator().manual_seed(ns)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64) * 2 - 1   # noqa: E731
    ar = Arena((ns + 5) * (n + 48), F64, DEV, max_ld=16)
    parts = r(ns, n)
    gp = ar.take(1, ns * n, misalign=shift, name="gpart", data=parts.reshape(1, -1))
    out = ar.vec(n, misalign=shift, name="out")
    p0, m0, v0 = r(n), r(n) * 0.1, r(n).abs() * 0.01
    par = ar.vec(n, misalign=shift, name="param", data=p0)
    m = ar.vec(n, name="exp_avg", data=m0)
    v = ar.vec(n, misalign=shift, name="exp_avg_sq", data=v0)
    step = torch.full((1,), 2, dtype=torch.int32, device=DEV)
    for reg, span in ((gp, ns * n), (out, n), (par, n), (m, n), (v, n)):
        ar.inside(reg.ptr, span)
    vp = ctypes.c_void_p
    lib = L._learn_lib()
    L._ok(lib.aac_sum64_partials(vp(out.ptr), vp(gp.ptr), ns, n, fused._stream()), "sum64")
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    L._ok(lib.aac_adam64_sum(vp(par.ptr), vp(gp.ptr), ns, vp(m.ptr), vp(v.ptr), n, lr, b1, b2, eps,
                             vp(step.data_ptr()), 1, fused._stream()), "adam64")
    torch.cuda.synchronize()
    gsum = parts[0].clone()
    for s in range(1, ns):
        gsum = gsum + parts[s]
    assert torch.equal(out.get().reshape(-1), gsum)
    t = 3
    m_ref = b1 * m0 + (1 - b1) * gsum
    v_ref = b2 * v0 + (1 - b2) * gsum * gsum
    p_ref = p0 - (lr / (1 - b1 ** t)) * m_ref / (v_ref.sqrt() / np.sqrt(1 - b2 ** t) + eps)
    np.testing.assert_allclose(m.get().reshape(-1), m_ref, rtol=1e-13, atol=0)
    np.testing.assert_allclose(v.get().reshape(-1), v_ref, rtol=1e-13, atol=0)
    np.testing.assert_allclose(par.get().reshape(-1), p_ref, rtol=1e-12, atol=1e-14)
    assert int(step.item()) == 2
    ar.check(writable=[out, par, m, v])
