"""The learner's row kernels that take a leading dimension (include/aac_fused.h) inside the poisoned
arena (tests/arena.py): the training attention forward / backward (MFMA and per-row paths), the
inference attention block, the critic heads and the actor output backward.  References and
tolerances are those of tests/test_fused_gpu.py (fp64 torch); every case ends in ``arena.check``:
only the kernel's documented outputs changed -- row gaps, neighbouring column blocks of ``cat`` and
the guards keep the canary -- and each output was written in full."""
import ctypes

import numpy as np
import pytest
import torch

from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
vp = ctypes.c_void_p


def _rnd(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def close(got, want, atol, rtol, what):
    np.testing.assert_allclose(got.double(), want, atol=atol, rtol=rtol, err_msg=what)


# ------------------------------------------------------------------ training attention
def attn_train_reference(eo, x, nei, Wq, Wk, Wv, dv, dcat_o):
    """fp64 autograd of the reference attention (ATT/nets:186-210) in the kernels' factored form
    (k_j . q = x_j . (Wk^T q)); the values test_attn_train_fwd_bwd_matches_autograd compares, plus
    qk, xb and dqk."""
    d = lambda t: t.double()   # noqa: E731
    eo_r, x_r = d(eo).requires_grad_(), d(x).requires_grad_()
    q = eo_r @ d(Wq).t()
    q.retain_grad()
    qk = q @ d(Wk)
    qk.retain_grad()
    score = torch.einsum("rkc,rc->rk", x_r, qk) / 8.0
    mask = d(nei).mean(-1) != 0
    a = torch.nan_to_num(torch.softmax(score.masked_fill(~mask, float("-inf")), dim=1)).masked_fill(~mask, 0.0)
    xb = torch.einsum("rk,rkc->rc", a, x_r)
    v = xb @ d(Wv).t()
    ((v * d(dv)).sum() + (eo_r * d(dcat_o)).sum()).backward()
    return dict(q=q.detach(), qk=qk.detach(), alpha=a.detach(), xb=xb.detach(), v=v.detach(),
                dxn=x_r.grad * (d(x) > 0), dqk=qk.grad, dq=q.grad, deo=eo_r.grad * (d(eo) > 0))


# which 16-B condition of the dispatch (aac_attn_train_fwd / attn_bwd_mfma_ok) a variant breaks
FWD_BREAKS = {"cat", "ldcat", "q", "qk", "nei"}
BWD_BREAKS = {"cat", "ldcat", "dv", "lddv", "dcat_o", "ldd", "dq", "deo"}
VARIANTS = ["none", "cat", "ldcat", "q", "qk", "nei", "dv", "lddv", "dcat_o", "ldd", "dq", "deo"]


def _attn_train_case(R, K, variant, nei_rows=None):
    """``nei_rows``: the neighbour rows (R, K, 6) to run with instead of the ones drawn here."""
    from multi_agent_aac_amd import fused
    r = _rnd(R * 100 + K)
    sh = lambda k: 1 if variant == k else 0   # noqa: E731
    ar = Arena(R * (1100 + 170 * K) + 3 * 64 * 64 + 448 * 8 + 8192, torch.float32, DEV, max_ld=448)
    eo_d, x_d = torch.relu(r(R, 64)), torch.relu(r(R, K, 64))
    nei_d = r(R, K, 6)
    nei_d[::4, 0] = 0.0                                   # masked neighbours
    if R > 7:
        nei_d[7] = 0.0                                    # an all-masked row
    if nei_rows is not None:
        nei_d = nei_rows.clone()
    Wq_d, Wk_d, Wv_d = (r(64, 64) * 0.125 for _ in range(3))
    dv_d, dcat_d = r(R, 64), r(R, 64)
    # cat: e_o in columns 0..63 (read), v_att into columns 128..191, columns 64..127 stay canary
    cat = ar.take(R, 192, ld=192 + sh("ldcat"), misalign=sh("cat"), name="cat", payload=False)
    eo = cat.sub(0, 0, R, 64, name="cat[:, :64]", data=eo_d)
    vout = cat.sub(0, 128, R, 64, name="cat[:, 128:]")
    x = ar.take(R * K, 64, name="xn", data=x_d.reshape(R * K, 64))
    nei = ar.take(R * K, 6, misalign=sh("nei"), name="nei", data=nei_d.reshape(R * K, 6))
    Wq = ar.take(64, 64, name="Wq", data=Wq_d)
    kv = ar.take(128, 64, name="Wkv", data=torch.cat([Wk_d, Wv_d]))
    q = ar.take(R, 64, misalign=sh("q"), name="q")
    qk = ar.take(R, 64, misalign=sh("qk"), name="qk")
    alpha, xb = ar.take(R, K, name="alpha"), ar.take(R, 64, name="xb")
    dv = ar.take(R, 64, ld=68 + sh("lddv"), misalign=sh("dv"), name="dv", data=dv_d)
    dcat = ar.take(R, 64, ld=68 + sh("ldd"), misalign=sh("dcat_o"), name="dcat_o", data=dcat_d)
    dxn, dqk = ar.take(R * K, 64, name="dxn"), ar.take(R, 64, name="dqk")
    dq, deo = ar.take(R, 64, misalign=sh("dq"), name="dq"), ar.take(R, 64, misalign=sh("deo"), name="deo")
    for reg in (cat, x, nei, Wq, kv, q, qk, alpha, xb, dv, dcat, dxn, dqk, dq, deo):
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    want = attn_train_reference(eo_d, x_d, nei_d, Wq_d, Wk_d, Wv_d, dv_d, dcat_d)
    tag = f"R {R} K {K} variant {variant}"
    fused.attn_train_fwd(eo.ptr, cat.ld, x.ptr, nei.ptr, Wq.ptr, kv.ptr, kv.at(64), q.ptr, qk.ptr, alpha.ptr, xb.ptr,
                         vout.ptr, cat.ld, R, K)
    torch.cuda.synchronize()
    close(vout.get(), want["v"], 2e-5, 1e-5, "v_att " + tag)
    close(alpha.get(), want["alpha"], 1e-6, 1e-7, "alpha " + tag)
    close(q.get(), want["q"], 2e-5, 1e-5, "q " + tag)
    close(qk.get(), want["qk"], 3e-5, 1e-5, "qk " + tag)
    close(xb.get(), want["xb"], 2e-5, 1e-5, "xb " + tag)
    ar.check(writable=[q, qk, alpha, xb, vout])
    ar.freeze([q, qk, alpha, xb, vout])                   # the backward only reads them
    fused.attn_train_bwd(dv.ptr, dv.ld, x.ptr, alpha.ptr, qk.ptr, eo.ptr, cat.ld, dcat.ptr, dcat.ld, Wq.ptr, kv.ptr,
                         kv.at(64), dxn.ptr, dqk.ptr, dq.ptr, deo.ptr, R, K)
    torch.cuda.synchronize()
    close(dxn.get().reshape(R, K, 64), want["dxn"], 2e-5, 1e-5, "dxn " + tag)
    close(dqk.get(), want["dqk"], 2e-5, 1e-5, "dqk " + tag)
    close(dq.get(), want["dq"], 2e-5, 1e-5, "dq " + tag)
    close(deo.get(), want["deo"], 2e-5, 1e-5, "deo " + tag)
    ar.check(writable=[dxn, dqk, dq, deo])
    if K > 8:
        return
    # the same backward with the neighbour encoder's weight-gradient partial rows (MFMA path only)
    npart = fused.attn_bwd_partials(R)
    pwn = ar.take(npart, 448, name="pwn")
    dqk2, dq2, deo2 = ar.take(R, 64, name="dqk2"), ar.take(R, 64, misalign=sh("dq"), name="dq2"), \
        ar.take(R, 64, misalign=sh("deo"), name="deo2")
    for reg in (pwn, dqk2, dq2, deo2):
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    ar.freeze([dxn, dqk, dq, deo])
    call = lambda: fused.attn_train_bwd_wn(dv.ptr, dv.ld, x.ptr, alpha.ptr, qk.ptr, eo.ptr, cat.ld, dcat.ptr, dcat.ld,  # noqa: E731
                                           Wq.ptr, kv.ptr, kv.at(64), dqk2.ptr, dq2.ptr, deo2.ptr, R, K, nei.ptr,
                                           pwn.ptr)
    if variant in BWD_BREAKS:
        with pytest.raises(RuntimeError, match="MFMA path"):
            call()
        ar.check()
        return
    call()
    torch.cuda.synchronize()
    assert torch.equal(dqk2.get(), dqk.get()) and torch.equal(dq2.get(), dq.get()) and torch.equal(deo2.get(), deo.get())
    g = want["dxn"].reshape(R * K, 64)
    tot = pwn.get().double().sum(0)
    close(tot[:384].reshape(64, 6), g.t() @ nei_d.double().reshape(R * K, 6), 2e-4, 1e-5, "dWn " + tag)
    close(tot[384:], g.sum(0), 2e-4, 1e-5, "dbn " + tag)
    ar.check(writable=[pwn, dqk2, dq2, deo2])


@pytest.mark.parametrize("K", [1, 4, 7, 12])
@pytest.mark.parametrize("R", [1, 15, 17, 65])
def test_attn_train_in_the_arena(native_lib, R, K):
    """aac_attn_train_fwd / _bwd / _bwd_wn with lde = ldv = 192 (v_att a column block of cat), lddv and
    ldd padded by 4; then each 16-B condition of the dispatch broken in turn (a base moved by one
    float, an ld of 4n + 1), so that the per-row kernels run on the same data.  K = 12 is the
    per-row path in any case.  Columns 64..127 of cat keep the canary throughout."""
    assert FWD_BREAKS | BWD_BREAKS | {"none"} == set(VARIANTS)
    for variant in (VARIANTS if K <= 8 else ["none", "cat", "lddv"]):
        _attn_train_case(R, K, variant)


@pytest.mark.parametrize("K", [1, 4, 7, 12])
@pytest.mark.parametrize("R", [1, 15, 17, 65])
def test_attn_block_in_the_arena(native_lib, R, K):
    """aac_attn_block (MFMA for K <= 4 on 16-B rows, per-row otherwise) reading e_o from cat and
    writing v_att into cat's last column block, reference of
    test_attn_block_matches_reference_attention; then with cat moved by one float and with ld 193."""
    for variant in ("none", "cat", "ldcat"):
        _attn_block_case(R, K, variant)


def _attn_block_case(R, K, variant, nei_rows=None):
    """One aac_attn_block launch in the arena; variant "cat": cat moved by one float, "ldcat": ld 193."""
    from multi_agent_aac_amd import fused
    r = _rnd(R * 100 + K + 1)
    ar = Arena(R * (200 + 8 * K) + 2 * 64 * 64 + 64 * 8 + 2048, torch.float32, DEV, max_ld=200)
    eo_d = torch.relu(r(R, 64))
    nei_d = r(R, K, 6)
    nei_d[::5, 0] = 0.0
    if R > 3:
        nei_d[3] = 0.0
    if nei_rows is not None:
        nei_d = nei_rows.clone()
    Wn_d, bn_d = r(64, 6) * 0.4, r(64) * 0.1
    Wq_d, Wk_d, Wv_d = (r(64, 64) * 0.125 for _ in range(3))
    cat = ar.take(R, 192, ld=192 + (variant == "ldcat"), misalign=int(variant == "cat"), name="cat", payload=False)
    eo = cat.sub(0, 0, R, 64, name="cat[:, :64]", data=eo_d)
    out = cat.sub(0, 128, R, 64, name="cat[:, 128:]")
    nei = ar.take(R * K, 6, name="nei", data=nei_d.reshape(R * K, 6))
    Wn, bn = ar.take(64, 6, name="Wn", data=Wn_d), ar.vec(64, name="bn", data=bn_d)
    wqk = ar.take(64, 64, name="Wqk", data=Wk_d.t() @ Wq_d)
    Wv = ar.take(64, 64, name="Wv", data=Wv_d)
    for reg in (cat, nei, Wn, bn, wqk, Wv):
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    fused.attn_block(eo.ptr, cat.ld, nei.ptr, Wn.ptr, bn.ptr, wqk.ptr, Wv.ptr, out.ptr, cat.ld, R, K)
    torch.cuda.synchronize()
    d = lambda t: t.double()   # noqa: E731
    x = torch.relu(d(nei_d) @ d(Wn_d).t() + d(bn_d))
    qv = d(eo_d) @ d(Wq_d).t()
    k, v = x @ d(Wk_d).t(), x @ d(Wv_d).t()
    score = torch.einsum("rkc,rc->rk", k, qv) / 8.0
    mask = d(nei_d).mean(-1) != 0
    score[~mask] = float("-inf")
    a = torch.softmax(score, dim=1)
    a[~mask] = 0.0
    a = torch.nan_to_num(a)
    close(out.get(), torch.einsum("rk,rkc->rc", a, v), 2e-5, 1e-5, f"R {R} K {K} {variant}")
    ar.check(writable=[out])


# ------------------------------------------------------------------ critic heads
def _head_case(M, mode, form, ldh=260):
    """One critic head over M rows of h at ldh = 260; form: "head" (aac_critic_head), "job"
    (aac_critic_head_job, mode 2 chained with the mse head), "gemm" (a job riding in a grouped GEMM
    launch beside a product).  include/aac_fused.h: "dha[r][c] ... ha / dha rows of 256" and for the
    head "rows of 256 features h[r*ldh + j]": dh is written as rows of 256 whatever ldh is."""
    from multi_agent_aac_amd import fused
    r = _rnd(M * 10 + mode)
    B, N = 2, 3                                           # mode 2: iteration = row // B
    ar = Arena(3 * M * (ldh + 256 + N * 2 + 8) + 4 * 256 + 12288, torch.float32, DEV, max_ld=ldh)
    h_d = torch.relu(r(M, 256))
    w_d, b_d, y_d = r(256), r(1), r(M)
    h = ar.take(M, 256, ld=ldh, name="h", data=h_d)
    w, b = ar.vec(256, name="w", data=w_d), ar.vec(1, name="b", data=b_d)
    y = ar.vec(M, misalign=1, name="y", data=y_d)
    rew_d, done_d = r(M, N), (torch.rand(M, N, generator=torch.Generator().manual_seed(M)) < 0.3).float()
    rew, done = ar.take(M, N, name="rew", data=rew_d), ar.take(M, N, misalign=1, name="done", data=done_d)
    q, dq = ar.vec(M, misalign=1, name="q"), ar.vec(M, name="dq")
    dh, yout = ar.take(M, 256, name="dh"), ar.vec(M, misalign=1, name="yout")
    chained = form == "job" and mode == 2
    if chained:                                           # the mse head of the first M2 rows of h2 on the TD target
        M2 = max(1, M - 1)
        h2_d, w2_d, b2_d = torch.relu(r(M2, 256)), r(256), r(1)
        h2 = ar.take(M2, 256, ld=ldh, name="h2", data=h2_d)
        w2, b2 = ar.vec(256, name="w2", data=w2_d), ar.vec(1, name="b2", data=b2_d)
        q2, dq2, dh2 = ar.vec(M2, name="q2"), ar.vec(M2, misalign=1, name="dq2"), ar.take(M2, 256, name="dh2")
    for reg in ar.regions:
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    job = fused.HeadJob(h.ptr, ldh, M, w.ptr, b.ptr, mode, y.ptr, rew.ptr, done.ptr, B, N, 0.95, q.ptr,
                        dq.ptr if mode < 2 else None, dh.ptr if mode < 2 else None, yout.ptr if mode == 2 else None,
                        *((h2.ptr, w2.ptr, b2.ptr, q2.ptr, dq2.ptr, dh2.ptr, M2) if chained else (None,) * 6 + (0,)))
    prod = None
    if form == "head":
        fused._chk(fused.lib().aac_critic_head(vp(h.ptr), ldh, M, vp(w.ptr), vp(b.ptr), mode, vp(y.ptr), vp(rew.ptr),
                                               vp(done.ptr), B, N, 0.95, vp(q.ptr), vp(job.dq), vp(job.dh), vp(job.yout),
                                               fused._stream()), "aac_critic_head")
    elif form == "job":
        fused.critic_head_job(job)
    else:
        from tests.test_gemm_layouts_gpu import P32
        prod = P32(33, 31, 40, tb=1, pad=4, bias=True, act=1, seed=M, ar=ar)
        ar.launch(fused.GemmLaunch([prod.prob], heads=[job]))
    torch.cuda.synchronize()
    tag = f"M {M} mode {mode} {form}"
    d = lambda t: t.double()   # noqa: E731
    close(q.get().reshape(-1), d(h_d) @ d(w_d) + d(b_d), 1e-4, 1e-5, "q " + tag)
    qg = q.get().reshape(-1)
    outs = [q]
    if mode == 2:
        it = torch.arange(M) // B
        want = rew_d[torch.arange(M), it] + 0.95 * qg * (1 - (done_d == 1).any(1).float())
        close(yout.get().reshape(-1), d(want), 1e-5, 1e-5, "yout " + tag)
        outs.append(yout)
        if chained:
            yv = yout.get().reshape(-1)[:M2]
            close(q2.get().reshape(-1), d(h2_d) @ d(w2_d) + d(b2_d), 1e-4, 1e-5, "q2 " + tag)
            g2 = (2.0 / M2) * (q2.get().reshape(-1) - yv)
            close(dq2.get().reshape(-1), d(g2), 1e-6, 1e-6, "dq2 " + tag)
            close(dh2.get(), d(g2[:, None] * w2_d[None] * (h2_d > 0)), 1e-6, 1e-6, "dh2 " + tag)
            outs += [q2, dq2, dh2]
    else:
        g = (2.0 / M) * (qg - y_d) if mode == 0 else torch.full_like(qg, -1.0 / M)
        close(dq.get().reshape(-1), d(g), 1e-6, 1e-6, "dq " + tag)
        close(dh.get(), d(g[:, None] * w_d[None] * (h_d > 0)), 1e-6, 1e-6, "dh " + tag)
        outs += [dq, dh]
    if prod is not None:
        prod.verify(tag)
        outs += prod.writable()
    ar.check(writable=outs)


@pytest.mark.parametrize("form", ["head", "job", "gemm"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M", [1, 3, 5])
def test_critic_head_in_the_arena(native_lib, M, mode, form):
    """ldh = 260, M in {1, 3, 5} (four rows per workgroup: a ragged last one); dh is exactly M rows
    of 256, q / dq / yout exactly M floats at bases off the 16-B grid."""
    _head_case(M, mode, form)


# ------------------------------------------------------------------ actor output backward
def _aob_reference(df, wenc, X, wa, ha, B, N, D0):
    R = B * N
    d = lambda t: t.double()   # noqa: E731
    da = torch.einsum("bnc,ncj->bnj", d(df).view(B, N, 128), d(wenc)[:, :, D0:D0 + 2]).reshape(R, 2)
    a_ = d(X)[:, :, D0:D0 + 2].reshape(R, 2)
    o = da * (1 - a_ * a_)
    return o, (o @ d(wa)) * (ha > 0)


@pytest.mark.parametrize("B", [1, 17])
def test_actor_out_bwd_in_the_arena(native_lib, B):
    """aac_actor_out_bwd with ldf = 128 N + 4 and aac_actor_dcomb_out_bwd (its operands have no ld of
    their own: ldw = 128 N is required; the bases it does not need aligned are moved by one float),
    N = 3, against the fp64 reference and tolerances of test_dcomb_out_bwd_matches_reference."""
    from multi_agent_aac_amd import fused
    N, D0 = 3, 14
    Din, R = D0 + 2, B * N
    r = _rnd(B)
    ar = Arena(B * (256 + 2 * 388 + N * Din + 8) + 256 * 384 + N * 128 * Din + 2 * 256 + 4 * R * 260 + 4096,
               torch.float32, DEV, max_ld=128 * N + 4)
    dh_d, Wc_d = r(B, 256) * 0.1, r(256, 128 * N) * 0.05
    f_d, wenc_d = torch.relu(r(B, 128 * N)), r(N, 128, Din) * 0.1
    X_d = torch.rand(B, N, Din, generator=torch.Generator().manual_seed(B)) * 2 - 1
    wa_d, ha_d = r(2, 256) * 0.1, torch.relu(r(R, 256))
    df_d = (dh_d.double() @ Wc_d.double() * (f_d > 0)).float()
    df = ar.take(B, 128 * N, ld=128 * N + 4, misalign=1, name="df", data=df_d)
    wenc = ar.take(N * 128, Din, misalign=1, name="wenc", data=wenc_d.reshape(N * 128, Din))
    X = ar.take(B, N * Din, misalign=1, name="X", data=X_d.reshape(B, N * Din))
    wa, ha = ar.take(2, 256, name="wa", data=wa_d), ar.take(R, 256, name="ha", data=ha_d)
    dout, dha = ar.take(R, 2, misalign=1, name="dout"), ar.take(R, 256, name="dha")
    dh, Wc = ar.take(B, 256, name="dh", data=dh_d), ar.take(256, 128 * N, name="Wc", data=Wc_d)
    f = ar.take(B, 128 * N, misalign=1, name="f", data=f_d)
    dout2, dha2 = ar.take(R, 2, misalign=1, name="dout2"), ar.take(R, 256, name="dha2")
    for reg in ar.regions:
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    fused.actor_out_bwd(df.ptr, df.ld, wenc.ptr, Din, D0, X.ptr, wa.ptr, ha.ptr, N, R, dout.ptr, dha.ptr)
    torch.cuda.synchronize()
    o, dh_ref = _aob_reference(df_d, wenc_d, X_d, wa_d, ha_d, B, N, D0)
    close(dout.get(), o, 1e-6, 1e-4, "dout")
    close(dha.get(), dh_ref, 1e-6, 1e-4, "dha")
    ar.check(writable=[dout, dha])
    ar.freeze([dout, dha])
    a = fused.DaobArgs(dh.ptr, Wc.ptr, f.ptr, wenc.ptr, X.ptr, wa.ptr, ha.ptr, dout2.ptr, dha2.ptr, 128 * N, Din, D0, N, B)
    fused.DcombAob(a)()
    torch.cuda.synchronize()
    df64 = dh_d.double() @ Wc_d.double() * (f_d > 0)
    o, dh_ref = _aob_reference(df64, wenc_d, X_d, wa_d, ha_d, B, N, D0)
    close(dout2.get(), o, 1e-6, 1e-4, "dcomb dout")
    close(dha2.get(), dh_ref, 1e-6, 1e-4, "dcomb dha")
    ar.check(writable=[dout2, dha2])
