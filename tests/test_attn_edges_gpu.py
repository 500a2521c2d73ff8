"""The attention entry points at the edges of their template instances (tests/attn_cases.py), inside
the poisoned arena (tests/arena.py): K = 8 and 16 fill the last slot of <8> and <16>, K = 17 and 32
are the first and the last K of <32>, which no test had launched.  R = 1 and 19 (one row; two 16-row
blocks / five 4-row workgroups with a ragged last one).  Each case runs in the natural layout (16-B
aligned: the MFMA kernels at K = 8) and with bases moved off the 16-B grid (the per-row <8> instance
at K = 8).  Outputs start as canary and must be written in full; everything else in the arena keeps
its bits.  K = 0 and K = 33 are refused by every entry point with the outputs untouched.

The references are the fp64 torch forms of tests/test_learner_gpu.py and tests/test_fused_gpu.py at
their tolerances (2e-5 absolute, 1e-5 relative)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import attn_cases as C
from tests.arena import Arena
from tests.test_learner_gpu import _ref_attention
from tests.test_row_kernels_layouts_gpu import _attn_block_case, _attn_train_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
vp = ctypes.c_void_p

# the variant of tests/test_row_kernels_layouts_gpu.py that breaks a 16-B condition of the forward and of
# the backward dispatch at once (cat moved by one float)
LAYOUT_VARIANT = {"natural": "none", "misaligned": "cat"}


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("K", C.ARENA_K)
@pytest.mark.parametrize("R", C.ARENA_R)
def test_masked_attention_edges_in_the_arena(native_lib, R, K, layout):
    """aac_attn_fwd / aac_attn_bwd (what ops.masked_attention launches) with k | v as the two halves of
    rows of 128 and out / dout rows padded by 4 (natural) or every base off by one float and odd
    strides (misaligned); the gaps between the rows and the halves' neighbours keep the canary."""
    from multi_agent_aac_amd import ops
    mis = int(layout == "misaligned")
    g = torch.Generator().manual_seed(R * 100 + K)
    q_d, kv_d, dout_d = (torch.randn(*s, generator=g) for s in ((R, 64), (R, K, 128), (R, 64)))
    nei_d = C.nei_rows(R, K, seed=1)
    ar = Arena(R * (600 + 400 * K) + 4096, torch.float32, DEV, max_ld=136)
    q = ar.take(R, 64, misalign=mis, name="q", data=q_d)
    kv = ar.take(R * K, 128, ld=128 + 5 * mis, misalign=mis, name="kv", data=kv_d.reshape(R * K, 128))
    nei = ar.take(R * K, 6, misalign=mis, name="nei", data=nei_d.reshape(R * K, 6))
    out = ar.take(R, 64, ld=68 + mis, misalign=mis, name="out")
    alpha = ar.take(R, K, misalign=mis, name="alpha")
    dout = ar.take(R, 64, ld=68 + mis, misalign=mis, name="dout", data=dout_d)
    dq = ar.take(R, 64, misalign=mis, name="dq")
    dkv = ar.take(R * K, 128, ld=kv.ld, misalign=mis, name="dkv")
    for reg in ar.regions:
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    qr, kvr = q_d.double().requires_grad_(), kv_d.double().requires_grad_()
    ref = _ref_attention(qr, kvr[..., :64], kvr[..., 64:], nei_d.double())
    ref.backward(dout_d.double())
    tag = f"R {R} K {K} {layout}"
    L = ops.lib()
    ops._chk(L.aac_attn_fwd(vp(q.ptr), vp(kv.ptr), vp(kv.at(0, 64)), kv.ld, vp(nei.ptr), vp(out.ptr), out.ld,
                            vp(alpha.ptr), R, K, _stream()), "aac_attn_fwd")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.get().double(), ref.detach(), atol=2e-5, rtol=1e-5, err_msg="out " + tag)
    m = C.valid_mask(nei_d)
    a = alpha.get()
    assert float(a[~m].abs().max() if (~m).any() else 0.0) == 0.0, "alpha of a masked slot " + tag
    score = torch.einsum("rkc,rc->rk", kv_d[..., :64].double(), q_d.double()) / 8.0
    a_ref = torch.nan_to_num(torch.softmax(score.masked_fill(~m, float("-inf")), dim=1)).masked_fill(~m, 0.0)
    np.testing.assert_allclose(a.double(), a_ref, atol=1e-6, err_msg="alpha " + tag)     # the training kernels' alpha bound
    ar.check(writable=[out, alpha])
    ar.freeze([out, alpha])
    ops._chk(L.aac_attn_bwd(vp(q.ptr), vp(kv.ptr), vp(kv.at(0, 64)), kv.ld, vp(alpha.ptr), vp(dout.ptr), dout.ld,
                            vp(dq.ptr), vp(dkv.ptr), vp(dkv.at(0, 64)), R, K, _stream()), "aac_attn_bwd")
    torch.cuda.synchronize()
    np.testing.assert_allclose(dq.get().double(), qr.grad, atol=2e-5, rtol=1e-5, err_msg="dq " + tag)
    np.testing.assert_allclose(dkv.get().double().reshape(R, K, 128), kvr.grad, atol=2e-5, rtol=1e-5,
                               err_msg="dkv " + tag)
    ar.check(writable=[dq, dkv])


@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("K", C.ARENA_K)
@pytest.mark.parametrize("R", C.ARENA_R)
def test_attn_train_edges_in_the_arena(native_lib, R, K, layout):
    """aac_attn_train_fwd / _bwd (and _bwd_wn at K = 8: the partial rows in the natural layout, its
    refusal in the misaligned one) on the edge rows of attn_cases.nei_rows."""
    assert (C.kernel("attn_train_bwd", K, layout == "natural")[0] == "mfma") == (K == 8 and layout == "natural")
    _attn_train_case(R, K, LAYOUT_VARIANT[layout], nei_rows=C.nei_rows(R, K, seed=2))


@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("K", C.ARENA_K)
@pytest.mark.parametrize("R", C.ARENA_R)
def test_attn_block_edges_in_the_arena(native_lib, R, K, layout):
    """aac_attn_block: per-row instances <8>, <16>, <32> (its MFMA variant stops at K = 4)."""
    assert C.kernel("attn_block", K, layout == "natural") == ("row", C.instance(K))
    _attn_block_case(R, K, LAYOUT_VARIANT[layout], nei_rows=C.nei_rows(R, K, seed=3))


# ------------------------------------------------------------------ refusals
def _filled(*shape):
    return torch.full(shape, 7.0, device=DEV)


def _untouched(*tensors):
    torch.cuda.synchronize()
    for t in tensors:
        assert bool((t == 7.0).all())


@pytest.mark.parametrize("K", C.REFUSED_K)
def test_masked_attention_refuses_k_out_of_range(native_lib, K):
    from multi_agent_aac_amd import ops
    R, Kb = 19, max(K, 1)
    q, kv, nei = torch.randn(R, 64, device=DEV), torch.randn(R, Kb, 128, device=DEV), torch.randn(R, Kb, 6, device=DEV)
    with pytest.raises(RuntimeError, match="1 <= K <= 32"):
        ops.masked_attention(q, kv[:, :K].contiguous(), nei[:, :K].contiguous())
    out, alpha, dq, dkv = _filled(R, 64), _filled(R, Kb), _filled(R, 64), _filled(R, Kb, 128)
    dout = torch.randn(R, 64, device=DEV)
    P = lambda t, off=0: vp(t.data_ptr() + 4 * off)   # noqa: E731
    L = ops.lib()
    assert L.aac_attn_fwd(P(q), P(kv), P(kv, 64), 128, P(nei), P(out), 64, P(alpha), R, K, _stream()) != 0
    assert L.aac_attn_bwd(P(q), P(kv), P(kv, 64), 128, P(alpha), P(dout), 64, P(dq), P(dkv), P(dkv, 64), R, K,
                          _stream()) != 0
    with pytest.raises(RuntimeError, match="1 <= K <= 32"):
        ops._chk(L.aac_attn_fwd(P(q), P(kv), P(kv, 64), 128, P(nei), P(out), 64, P(alpha), R, K, _stream()), "aac_attn_fwd")
    _untouched(out, alpha, dq, dkv)


@pytest.mark.parametrize("K", C.REFUSED_K)
def test_attn_train_and_block_refuse_k_out_of_range(native_lib, K):
    from multi_agent_aac_amd import fused
    R, Kb = 19, max(K, 1)
    P = fused.ptr
    r = lambda *s: torch.randn(*s, device=DEV)   # noqa: E731
    cat, x, nei = r(R, 192), r(R * Kb, 64), r(R * Kb, 6)
    Wq, kv, Wn, bn, wqk = r(64, 64), r(128, 64), r(64, 6), r(64), r(64, 64)
    q, qk, alpha, xb, vout = _filled(R, 64), _filled(R, 64), _filled(R, Kb), _filled(R, 64), _filled(R, 64)
    with pytest.raises(RuntimeError, match="attn_train_fwd: 1 <= K <= 32"):
        fused.attn_train_fwd(P(cat), 192, P(x), P(nei), P(Wq), P(kv), P(kv, 64 * 64), P(q), P(qk), P(alpha), P(xb),
                             P(vout), 64, R, K)
    _untouched(q, qk, alpha, xb, vout)
    dv, dcat_o, a_in, qk_in = r(R, 64), r(R, 64), r(R, Kb), r(R, 64)
    dxn, dqk, dq, deo = _filled(R * Kb, 64), _filled(R, 64), _filled(R, 64), _filled(R, 64)
    with pytest.raises(RuntimeError, match="attn_train_bwd: 1 <= K <= 32"):
        fused.attn_train_bwd(P(dv), 64, P(x), P(a_in), P(qk_in), P(cat), 192, P(dcat_o), 64, P(Wq), P(kv),
                             P(kv, 64 * 64), P(dxn), P(dqk), P(dq), P(deo), R, K)
    pwn = _filled(fused.attn_bwd_partials(R), 448)
    with pytest.raises(RuntimeError, match="attn_train_bwd: 1 <= K <= 32"):
        fused.attn_train_bwd_wn(P(dv), 64, P(x), P(a_in), P(qk_in), P(cat), 192, P(dcat_o), 64, P(Wq), P(kv),
                                P(kv, 64 * 64), P(dqk), P(dq), P(deo), R, K, P(nei), P(pwn))
    _untouched(dxn, dqk, dq, deo, pwn)
    out = _filled(R, 64)
    with pytest.raises(RuntimeError, match="attn_block: 1 <= K <= 32"):
        fused.attn_block(P(cat), 192, P(nei), P(Wn), P(bn), P(wqk), P(kv, 64 * 64), P(out), 64, R, K)
    _untouched(out)
