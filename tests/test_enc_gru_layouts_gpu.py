"""aac_attn_enc_fwd (include/aac_fused.h) and the GRU row kernels aac_gru_cell / aac_pack_rows /
aac_gru_reset_hidden (include/aac_gru.h) inside the poisoned arena (tests/arena.py), with every
leading dimension above its natural width and the scalar-accessed bases off the 16-B grid.
References and tolerances are those of test_attn_enc_fwd_matches_reference,
test_out_layer_folded_into_critic_encoder_job and test_gru_cell_modes; every case ends in
``arena.check``."""
import numpy as np
import pytest
import torch

from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 64


def _rnd(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc


def close(got, want, atol, rtol, what):
    np.testing.assert_allclose(got.double(), want, atol=atol, rtol=rtol, err_msg=what)


def _inside_all(ar):
    for reg in ar.regions:
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)


# ------------------------------------------------------------------ aac_attn_enc_fwd
@pytest.mark.parametrize("two_sets", [False, True])
@pytest.mark.parametrize("K", [4, 7])
@pytest.mark.parametrize("R", [1, 17])
def test_attn_enc_fwd_in_the_arena(native_lib, R, K, two_sets):
    """One training set with the riding critic-encoder job and its folded output layer -- ld_own =
    d_own + 6, ld_radar = 20, ld_cat = 196, cx_ld = N Din + 4 -- alone, and beside an inference set
    (which writes its cat and nothing else).  The folded layer writes exactly the two action
    columns of each agent into the critic input (o_x); those columns and cf are the job's only
    writes.  The job stages whole input rows, action columns included, before it replaces them
    with the computed actions, so their canary is read and discarded, never folded."""
    from multi_agent_aac_amd import fused
    D0, Nc, Din, rows = 22, 3, 24, R
    Dc0 = Din - 2
    r = _rnd(R * 10 + K)
    ar = Arena(R * (28 + 20 + 6 * K + 2 * 196 + 64 * K + 4 * 64 + K + Nc * 256 + 76 + Nc * 128 + 400) + 64 * (D0 + 18 + 6 + 64 + 3)
               + 128 * 64 + Nc * 128 * (Din + 1) + 2 * 256 + 8192, torch.float32, DEV, max_ld=Nc * 128)
    d = lambda t: t.double()   # noqa: E731
    own_d, radar_d, nei_d = r(R, D0), torch.rand(R, 18, generator=torch.Generator().manual_seed(R)) * 15, r(R, K, 6)
    nei_d[::4, 0] = 0.0
    if R > 9:
        nei_d[9] = 0.0
    W = {k: r(*s, sc=sc) for k, s, sc in (("Wo", (64, D0), 0.3), ("bo", (64,), 0.1), ("Wg", (64, 18), 0.1),
                                             ("bg", (64,), 0.1), ("Wn", (64, 6), 0.4), ("bn", (64,), 0.1),
                                             ("Wq", (64, 64), 0.125))}
    kv_d = r(128, 64, sc=0.125)
    own = ar.take(R, D0, ld=D0 + 6, misalign=1, name="own", data=own_d)
    radar = ar.take(R, 18, ld=20, misalign=1, name="radar", data=radar_d)
    nei = ar.take(R * K, 6, name="nei", data=nei_d.reshape(R * K, 6))
    Wr = {k: ar.take(v.shape[0], v.shape[1], name=k, data=v) if v.dim() == 2 else ar.vec(64, name=k, data=v)
          for k, v in W.items()}
    kv = ar.take(128, 64, name="Wkv", data=kv_d)
    cat_t = ar.take(R, 192, ld=196, name="cat_t")
    cat_i = ar.take(R, 192, ld=196, name="cat_i") if two_sets else None
    xn, q, qk = ar.take(R * K, 64, name="xn"), ar.take(R, 64, name="q"), ar.take(R, 64, name="qk")
    alpha, xb = ar.take(R, K, misalign=1, name="alpha"), ar.take(R, 64, name="xb")
    # the riding job: critic input rows [own_n (Dc0) | a_n (2)] x Nc at cx_ld = Nc Din + 4
    X = ar.take(rows, Nc * Din, ld=Nc * Din + 4, misalign=1, name="X", payload=False)
    xo = [X.sub(0, n * Din, rows, Dc0, name=f"X.own{n}", data=r(rows, Dc0)) for n in range(Nc)]
    xa = [X.sub(0, n * Din + Dc0, rows, 2, name=f"X.act{n}") for n in range(Nc)]
    cw_d, cb_d = r(Nc, 128, Din, sc=0.2), r(Nc, 128, sc=0.1)
    cw = ar.take(Nc * 128, Din, misalign=1, name="cW", data=cw_d.reshape(Nc * 128, Din))
    cb = ar.vec(Nc * 128, misalign=1, name="cb", data=cb_d.reshape(-1))
    cf = ar.take(rows, Nc * 128, name="cf")
    ha_d, wa_d, ba_d = torch.relu(r(rows * Nc, 256)), r(2, 256, sc=0.1), r(2, sc=0.1)
    ha, wa = ar.take(rows * Nc, 256, name="ha", data=ha_d), ar.take(2, 256, name="Wa", data=wa_d)
    ba = ar.vec(2, misalign=1, name="ba", data=ba_d)
    _inside_all(ar)

    def args(cat, train, ride):
        a = fused.AttnEncArgs()
        a.own, a.ld_own, a.d_own, a.radar, a.ld_radar, a.nei = own.ptr, own.ld, D0, radar.ptr, radar.ld, nei.ptr
        for k in ("Wo", "bo", "Wg", "bg", "Wn", "bn", "Wq"):
            setattr(a, k, Wr[k].ptr)
        a.Wk, a.Wv = kv.ptr, kv.at(64)
        a.cat, a.ld_cat, a.R, a.K = cat.ptr, cat.ld, R, K
        if train:
            a.xn, a.q, a.qk, a.alpha, a.xb = xn.ptr, q.ptr, qk.ptr, alpha.ptr, xb.ptr
        if ride:
            a.cx, a.cx_ld, a.c_din, a.cW, a.cb, a.cf, a.c_rows, a.c_n = X.ptr, X.ld, Din, cw.ptr, cb.ptr, cf.ptr, rows, Nc
            a.o_h, a.o_w, a.o_b, a.o_x, a.o_d0 = ha.ptr, wa.ptr, ba.ptr, X.ptr, Dc0
        return a

    sets = [args(cat_t, True, True)] + ([args(cat_i, False, False)] if two_sets else [])
    fused.AttnEnc(*sets)()
    torch.cuda.synchronize()
    eo = torch.relu(d(own_d) @ d(W["Wo"]).t() + d(W["bo"]))
    eg = torch.relu(d(radar_d) @ d(W["Wg"]).t() + d(W["bg"]))
    x = torch.relu(d(nei_d) @ d(W["Wn"]).t() + d(W["bn"]))
    qr = eo @ d(W["Wq"]).t()
    k, v = x @ d(kv_d[:64]).t(), x @ d(kv_d[64:]).t()
    score = torch.einsum("rkc,rc->rk", k, qr) / 8.0
    mask = d(nei_d).mean(-1) != 0
    a = torch.nan_to_num(torch.softmax(score.masked_fill(~mask, float("-inf")), dim=1)).masked_fill(~mask, 0.0)
    want = torch.cat([eo, eg, torch.einsum("rk,rkc->rc", a, v)], 1)
    tag = f"R {R} K {K} sets {len(sets)}"
    for cat in [cat_t] + ([cat_i] if two_sets else []):
        close(cat.get(), want, 3e-5, 1e-5, cat.name + " " + tag)
    close(xn.get().reshape(R, K, 64), x, 2e-5, 1e-5, "xn " + tag)
    close(q.get(), qr, 2e-5, 1e-5, "q " + tag)
    close(qk.get(), qr @ d(kv_d[:64]), 3e-5, 1e-5, "qk " + tag)
    close(alpha.get(), a, 1e-6, 1e-7, "alpha " + tag)
    close(xb.get(), torch.einsum("rk,rkc->rc", a, x), 2e-5, 1e-5, "xb " + tag)
    a_ref = torch.tanh(d(ha_d) @ d(wa_d).t() + d(ba_d)).reshape(rows, Nc, 2)
    xin = torch.zeros(rows, Nc, Din, dtype=torch.float64)
    for n in range(Nc):
        close(xa[n].get(), a_ref[:, n], 2e-6, 1e-5, f"actions of agent {n} " + tag)
        xin[:, n, :Dc0], xin[:, n, Dc0:] = d(xo[n].get()), d(xa[n].get())
    fw = torch.relu(torch.einsum("bnd,ncd->bnc", xin, d(cw_d)) + d(cb_d)).reshape(rows, Nc * 128)
    close(cf.get(), fw, 2e-5, 1e-5, "cf " + tag)
    ar.check(writable=[cat_t, xn, q, qk, alpha, xb, cf] + xa + ([cat_i] if two_sets else []))


# ------------------------------------------------------------------ aac_gru_cell
@pytest.mark.parametrize("M,N", [(1, 1), (17, 1), (1, 17)])
@pytest.mark.parametrize("mode", ["fwd", "td", "critic", "actloss", "actbwd"])
def test_gru_cell_in_the_arena(native_lib, mode, M, N):
    """Every mode at M N in {1, 17} rows (four rows per workgroup: a ragged last one) with ldg = ldd =
    196, ldh = ldho = 68, ldy = O + 2, ldda = O + 1 and the packed destination rows of the fwd mode
    at ld_pack_dst = npack + O + 3 > npack + O; the fp64 autograd reference of test_gru_cell_modes."""
    from multi_agent_aac_amd import gru
    R = M * N
    O = 2 if mode in ("fwd", "actbwd") else 1
    act = gru.TANH if O == 2 else 0
    torch.manual_seed(5 + R)
    cells = [torch.nn.GRUCell(128, H).double() for _ in range(N)]
    outs = [torch.nn.Linear(H, O).double() for _ in range(N)]
    x = torch.randn(M, N, 128, dtype=torch.float64)
    h = torch.tanh(torch.randn(M, N, H, dtype=torch.float64))
    gi = torch.stack([x[:, i] @ cells[i].weight_ih.t() + cells[i].bias_ih for i in range(N)], 1).detach()
    gh = torch.stack([h[:, i] @ cells[i].weight_hh.t() + cells[i].bias_hh for i in range(N)], 1).detach()
    gi_r, gh_r = gi.clone().requires_grad_(True), gh.clone().requires_grad_(True)
    rr = torch.sigmoid(gi_r[..., :H] + gh_r[..., :H])
    zz = torch.sigmoid(gi_r[..., H:2 * H] + gh_r[..., H:2 * H])
    nn_ = torch.tanh(gi_r[..., 2 * H:] + rr * gh_r[..., 2 * H:])
    hp = (h - nn_) * zz + nn_
    W = torch.stack([o.weight.detach() for o in outs])          # (N, O, H)
    b = torch.stack([o.bias.detach() for o in outs])            # (N, O)
    y = torch.einsum("mnh,noh->mno", hp, W) + b
    if act:
        y = torch.tanh(y)
    tgt = torch.randn(M, N, dtype=torch.float64)
    rew, done = torch.randn(M, N, dtype=torch.float64), (torch.rand(M, N) < 0.3).double()
    da = torch.randn(M, N, O, dtype=torch.float64)
    if mode == "critic":
        loss = ((y[..., 0] - tgt) ** 2).mean(0).sum()
    elif mode == "actloss":
        loss = (3 - y[..., 0].mean(0)).sum()
    elif mode == "actbwd":
        loss = (y * da).sum()
    if mode in ("critic", "actloss", "actbwd"):
        loss.backward()
    f = lambda t: t.float()                                     # noqa: E731
    ar = Arena(R * (2 * 196 + 2 * 68 + 2 * 196 + 64) + N * 200 + 4096, torch.float32, DEV, max_ld=200)
    gi_a = ar.take(R, 192, ld=196, misalign=1, name="gi", data=f(gi).reshape(R, 192))
    gh_a = ar.take(R, 192, ld=196, name="gh", data=f(gh).reshape(R, 192))
    h_a = ar.take(R, H, ld=68, misalign=1, name="h", data=f(h).reshape(R, H))
    wpack = ar.take(N, 200, name="wpack", payload=False)        # agent stride 200 floats
    for i in range(N):
        wpack.sub(i, 0, 1, O * H, name=f"Wout{i}", data=f(W[i]).reshape(1, -1))
        wpack.sub(i, O * H, 1, O, name=f"bout{i}", data=f(b[i]).reshape(1, -1))
    hout = ar.take(R, H, ld=68, misalign=1, name="hout")
    kw = dict(gi=gi_a.ptr, gh=gh_a.ptr, ldg=196, h=h_a.ptr, ldh=68, wout=wpack.ptr, bout=wpack.at(0, O * H), wstride=200,
              bstride=200, O=O, act=act, R=R, N=N, hout=hout.ptr, ldho=68, ldy=O + 2, ldd=196, ldda=O + 1)
    outs_w = [hout]
    if mode == "fwd":
        src_d = torch.randn(R, 10)
        yo = ar.take(R, O, ld=O + 2, misalign=1, name="y")
        src = ar.take(R, 6, ld=12, misalign=1, name="pack_src", data=src_d[:, :6])
        pk = ar.take(R, 6 + O, ld=6 + O + 3, misalign=1, name="pack_dst")
        kw.update(mode=gru.FWD, y=yo.ptr, pack_src=src.ptr, ld_pack_src=12, npack=6, pack_dst=pk.ptr, ld_pack_dst=6 + O + 3)
        outs_w += [yo, pk]
    elif mode == "td":
        rew_a, done_a = ar.vec(R, misalign=1, name="rew", data=f(rew).reshape(-1)), ar.vec(R, name="done", data=f(done).reshape(-1))
        yo = ar.vec(R, misalign=1, name="yout")
        kw.update(mode=gru.TD, rew=rew_a.ptr, done=done_a.ptr, gamma=0.95, yout=yo.ptr)
        outs_w += [yo]
    else:
        dgi, dgh = ar.take(R, 192, ld=196, misalign=1, name="dgi"), ar.take(R, 192, ld=196, name="dgh")
        dq = ar.take(R, O, misalign=1, name="dq")
        kw.update(mode={"critic": gru.CRITIC, "actloss": gru.ACTLOSS, "actbwd": gru.ACTBWD}[mode], inv_m=1.0 / M,
                  dq=dq.ptr, dgi=dgi.ptr, dgh=dgh.ptr)
        outs_w += [dgi, dgh, dq]
        if mode == "actbwd":
            da_a = ar.take(R, O, ld=O + 1, misalign=1, name="da", data=f(da).reshape(R, O))
            kw.update(da=da_a.ptr)
        else:
            qv = ar.vec(R, misalign=1, name="q")
            kw.update(y=qv.ptr)
            outs_w += [qv]
            if mode == "critic":
                kw.update(target=ar.vec(R, misalign=1, name="target", data=f(tgt).reshape(-1)).ptr)
    _inside_all(ar)
    gru.GruCell(**kw)()
    torch.cuda.synchronize()
    tag = f"{mode} M {M} N {N}"
    close(hout.get().reshape(M, N, H), hp.detach(), 2e-6, 1e-7, "hout " + tag)
    if mode == "fwd":
        close(yo.get().reshape(M, N, O), y.detach(), 2e-6, 1e-7, "y " + tag)
        assert torch.equal(pk.get()[:, :6], src_d[:, :6]) and torch.equal(pk.get()[:, 6:], yo.get())
    elif mode == "td":
        close(yo.get().reshape(M, N), rew + 0.95 * y[..., 0].detach() * (1 - done), 5e-6, 1e-7, "yout " + tag)
    else:
        close(dgi.get().reshape(M, N, 192), gi_r.grad, 2e-6, 1e-4, "dgi " + tag)
        close(dgh.get().reshape(M, N, 192), gh_r.grad, 2e-6, 1e-4, "dgh " + tag)
        if mode == "critic":
            close(qv.get().reshape(M, N), y[..., 0].detach(), 2e-6, 1e-7, "q " + tag)
            close(dq.get().reshape(M, N), (2.0 / M) * (y[..., 0].detach() - tgt), 2e-6, 1e-4, "dq " + tag)
        elif mode == "actbwd":
            close(dq.get().reshape(M, N, O), da * (1 - y.detach() ** 2), 2e-6, 1e-4, "dout " + tag)
    ar.check(writable=outs_w)


@pytest.mark.parametrize("R", [1, 17])
def test_pack_rows_and_reset_hidden_in_the_arena(native_lib, R):
    """aac_pack_rows with ldd, lda and ldb above the packed widths; aac_gru_reset_hidden over R envs:
    the rows of the envs whose env_done is 0 stay bit-unchanged (they are checked as inputs), the
    others become zeros."""
    from multi_agent_aac_amd import gru
    r = _rnd(R)
    ar = Arena(R * (11 + 9 + 5 + 3 * 48 + 200) + 2048, torch.float32, DEV, max_ld=200)
    a_d, b_d = r(R, 6), r(R, 2)
    a = ar.take(R, 6, ld=9, misalign=1, name="a", data=a_d)
    b = ar.take(R, 2, ld=5, misalign=1, name="b", data=b_d)
    dst = ar.take(R, 8, ld=11, misalign=1, name="dst")
    width = 3 * 37                                               # N agents x an odd hidden width
    hc = ar.take(R, width, misalign=1, name="hidden", payload=False)
    h_d = r(R, width)
    done = torch.zeros(R, dtype=torch.uint8)
    done[::3] = 1
    if R > 5:
        done[5] = 255                                            # any non-zero byte counts
    rows = [hc.sub(e, 0, 1, width, name=f"hidden[{e}]", data=h_d[e:e + 1]) for e in range(R)]
    _inside_all(ar)
    gru.pack_rows(dst.ptr, dst.ld, a.ptr, a.ld, 6, b.ptr, b.ld, 2, R)
    done_dev = done.to(DEV)
    gru._chk(gru.glib().aac_gru_reset_hidden(gru.vp(hc.ptr), R, width, gru.vp(done_dev.data_ptr()),
                                             gru.fused._stream()), "aac_gru_reset_hidden")
    torch.cuda.synchronize()
    assert torch.equal(dst.get(), torch.cat([a_d, b_d], 1))
    cleared = [rows[e] for e in range(R) if done[e]]
    for reg in cleared:
        assert float(reg.get().abs().max()) == 0.0
    ar.check(writable=[dst] + cleared)
