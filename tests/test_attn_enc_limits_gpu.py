"""aac_attn_enc_fwd at its limits (tests/attn_cases.ENC_CASES): K = 8, d_own = 38 and a riding critic
job of nine agents with c_din = 40 and the folded output layer at o_d0 = 38 -- N = 9 as the fused plan
builds it, the edge of all three limits -- and the first cases on attn_enc_kernel<8, 10>, <4, 10> and
<8, 6>, which no test had launched.  The reference is the fp64 torch form of
test_attn_enc_fwd_matches_reference / test_out_layer_folded_into_critic_encoder_job at their tolerances.

Every operand lives in the poisoned arena (tests/arena.py).  The own rows are the critic-input rows of
the plan: ld_own = d_own + 2, so at d_own = 38 the stride is 40 exactly and the two columns between
the rows keep the canary NaN -- a kernel that staged them into a product would show it.  A two-set
launch (training set with the riding job + inference set) gives the bits of the sets launched alone.
K = 9, d_own = 41 and c_din = 41 are refused with the outputs untouched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import attn_cases as C
from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _d(t):
    return t.double()


def _reference(own, radar, nei, W, kv):
    eo = torch.relu(_d(own) @ _d(W["Wo"]).t() + _d(W["bo"]))
    eg = torch.relu(_d(radar) @ _d(W["Wg"]).t() + _d(W["bg"]))
    x = torch.relu(_d(nei) @ _d(W["Wn"]).t() + _d(W["bn"]))
    q = eo @ _d(W["Wq"]).t()
    k, v = x @ _d(kv[:64]).t(), x @ _d(kv[64:]).t()
    score = torch.einsum("rkc,rc->rk", k, q) / 8.0
    mask = _d(nei).mean(-1) != 0
    a = torch.nan_to_num(torch.softmax(score.masked_fill(~mask, float("-inf")), dim=1)).masked_fill(~mask, 0.0)
    return dict(cat=torch.cat([eo, eg, torch.einsum("rk,rkc->rc", a, v)], 1), xn=x, qa=q, qk=q @ _d(kv[:64]), alpha=a,
                xb=torch.einsum("rk,rkc->rc", a, x))


class _Acts:
    """The backward's activations of one training set as arena regions (what fused.ActorActs holds)."""
    NAMES = ("xn", "qa", "qk", "alpha", "xb")

    def __init__(self, ar, R, K, tag):
        self.reg = dict(xn=ar.take(R * K, 64, name="xn" + tag), qa=ar.take(R, 64, name="q" + tag),
                        qk=ar.take(R, 64, name="qk" + tag), alpha=ar.take(R, K, name="alpha" + tag),
                        xb=ar.take(R, 64, name="xb" + tag))
        for n, r in self.reg.items():
            setattr(self, n, r.view)

    def regions(self):
        return list(self.reg.values())


@pytest.mark.parametrize("K,d_own,Nc,Din,fold", C.ENC_CASES, ids=lambda v: str(int(v)))
def test_attn_enc_fwd_at_its_limits(native_lib, K, d_own, Nc, Din, fold):
    from multi_agent_aac_amd import fused
    R, rows = C.ENC_R, C.ENC_ROWS
    ld_own = d_own + 2
    g = torch.Generator().manual_seed(40 + K + d_own + Din)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc   # noqa: E731
    own_d, radar_d = r(R, d_own), torch.rand(R, 18, generator=g) * 15
    nei_d = C.nei_rows(R, K, seed=4)
    W = {k: r(*s, sc=sc) for k, s, sc in (("Wo", (64, d_own), 0.3), ("bo", (64,), 0.1), ("Wg", (64, 18), 0.1),
                                             ("bg", (64,), 0.1), ("Wn", (64, 6), 0.4), ("bn", (64,), 0.1),
                                             ("Wq", (64, 64), 0.125))}
    kv_d = r(128, 64, sc=0.125)
    d0 = Din - 2
    cx_d = r(rows, Nc, Din)
    cw_d, cb_d = r(Nc, 128, Din, sc=0.2), r(Nc, 128, sc=0.1)
    ha_d = torch.relu(r(rows * Nc, 256))
    wa_d, ba_d = r(2, 256, sc=0.1), r(2, sc=0.1)

    ar = Arena(R * (ld_own + 18 + 6 * K + 4 * 192 + 2 * (64 * K + 3 * 64 + K) + 64) + 64 * (d_own + 18 + 6 + 64 + 3)
               + 128 * 64 + rows * Nc * (Din + 2 * 128 + 256) + Nc * 128 * (Din + 1) + 1024 + 40 * 64, torch.float32, DEV,
               max_ld=max(192, Nc * 128))
    ownc = ar.take(R, ld_own, name="own rows", payload=False)
    own = ownc.sub(0, 0, R, d_own, name="own", data=own_d)
    radar = ar.take(R, 18, name="radar", data=radar_d)
    nei = ar.take(R * K, 6, name="nei", data=nei_d.reshape(R * K, 6))
    wr = {k: (ar.take(*v.shape, name=k, data=v) if v.dim() == 2 else ar.vec(v.numel(), name=k, data=v)) for k, v in W.items()}
    kv = ar.take(128, 64, name="Wkv", data=kv_d)
    ap = SimpleNamespace(**{k: v.ptr for k, v in wr.items()}, Wkv=kv.ptr)
    X = ar.take(rows, Nc * Din, name="X", payload=False)
    if fold:        # the action columns are outputs of the riding job (canary until written)
        for n in range(Nc):
            X.sub(0, n * Din, rows, d0, name=f"X own {n}", data=cx_d[:, n, :d0])
        xact = [X.sub(0, n * Din + d0, rows, 2, name=f"X act {n}") for n in range(Nc)]
        ha = ar.take(rows * Nc, 256, name="ha", data=ha_d)
        ap.Wa, ap.ba = ar.take(2, 256, name="Wa", data=wa_d).ptr, ar.vec(2, name="ba", data=ba_d).ptr
    else:
        X.sub(0, 0, rows, Nc * Din, name="X all", data=cx_d.reshape(rows, Nc * Din))
        xact = []
    cw = ar.take(Nc * 128, Din, name="enc_w", data=cw_d.reshape(Nc * 128, Din))
    cb = ar.vec(Nc * 128, name="enc_b", data=cb_d.reshape(-1))
    cp = SimpleNamespace(enc_w=[cw.at(n * 128) for n in range(Nc)], enc_b=[cb.at(0, n * 128) for n in range(Nc)])
    cats = [ar.take(R, 192, name=f"cat{i}") for i in range(4)]
    fs = [ar.take(rows, Nc * 128, name=f"f{i}") for i in range(2)]
    acts, acts2 = _Acts(ar, R, K, ""), _Acts(ar, R, K, "'")
    for reg in ar.regions:
        ar.inside_mat(reg.ptr, reg.rows, reg.cols, reg.ld, reg.name)
    assert C.enc_instance(K, max(d_own, Din)) in C.ENC_COMPILED

    def ride(f):
        return fused.critic_enc_ride(cp, X.ptr, rows, Nc, Din, f.view, fold=(ha.ptr, ap, d0) if fold else None)

    def aset(cat, a=None, rd=None):
        return fused.attn_set(ap, own.ptr, ld_own, d_own, radar.ptr, nei.ptr, R, K, cat.ptr, acts=a, ride=rd)
    fused.AttnEnc(aset(cats[0], acts, ride(fs[0])), aset(cats[1]))()
    torch.cuda.synchronize()
    want = _reference(own_d, radar_d, nei_d, W, kv_d)
    tag = f"K {K} d_own {d_own} c_n {Nc} c_din {Din}"
    for cat in cats[:2]:
        np.testing.assert_allclose(_d(cat.get()), want["cat"], atol=3e-5, rtol=1e-5, err_msg=cat.name + " " + tag)
    for n, (atol, rtol) in dict(xn=(2e-5, 1e-5), qa=(2e-5, 1e-5), qk=(3e-5, 1e-5), alpha=(1e-6, 1e-7), xb=(2e-5, 1e-5)).items():
        np.testing.assert_allclose(_d(acts.reg[n].get()).reshape(want[n].shape), want[n], atol=atol, rtol=rtol,
                                   err_msg=n + " " + tag)
    xin = _d(cx_d).clone()
    if fold:
        a_ref = torch.tanh(_d(ha_d) @ _d(wa_d).t() + _d(ba_d)).reshape(rows, Nc, 2)
        got = torch.stack([x.get() for x in xact], 1)
        np.testing.assert_allclose(_d(got), a_ref, atol=2e-6, rtol=1e-5, err_msg="folded actions " + tag)
        xin[:, :, d0:] = a_ref
    fw = torch.relu(torch.einsum("bnd,ncd->bnc", xin, _d(cw_d)) + _d(cb_d)).reshape(rows, Nc * 128)
    np.testing.assert_allclose(_d(fs[0].get()), fw, atol=2e-5, rtol=1e-5, err_msg="riding encoders " + tag)
    first = cats[:2] + [fs[0]] + acts.regions() + xact
    ar.check(writable=first)
    # the sets alone, and the riding job alone: the same bits, and nothing else touched
    ar.freeze(first)
    fused.AttnEnc(aset(cats[2], acts2))()
    fused.AttnEnc(aset(cats[3]))()
    fused.AttnEnc(fused.ride_only(ride(fs[1])))()
    torch.cuda.synchronize()
    assert torch.equal(cats[2].get(), cats[0].get()) and torch.equal(cats[3].get(), cats[1].get())
    assert torch.equal(fs[1].get(), fs[0].get())
    for n in _Acts.NAMES:
        assert torch.equal(acts2.reg[n].get(), acts.reg[n].get()), n
    ar.check(writable=cats[2:] + [fs[1]] + acts2.regions() + xact)      # the fold rewrites the same actions
    if fold:
        assert torch.equal(torch.stack([x.get() for x in xact], 1), got)


@pytest.mark.parametrize("what", C.ENC_REFUSED)
def test_attn_enc_fwd_refuses_past_its_limits(native_lib, what):
    """One past each limit of the N = 9 case: K = 9, d_own = 41, c_din = 41."""
    from multi_agent_aac_amd import fused
    K, d_own, Nc, Din = 8 + (what == "K"), 38 + 3 * (what == "d_own"), 9, 40 + (what == "c_din")
    assert not C.enc_accepts(K, d_own, Din) and C.enc_accepts(8, 38, 40)
    R, rows = C.ENC_R, C.ENC_ROWS
    P = fused.ptr
    r = lambda *s: torch.randn(*s, device=DEV)   # noqa: E731
    own, radar, nei = r(R, 48), r(R, 18), r(R, K, 6)
    Wt = dict(Wo=r(64, 48), bo=r(64), Wg=r(64, 18), bg=r(64), Wn=r(64, 6), bn=r(64), Wq=r(64, 64), Wkv=r(128, 64))
    ap = SimpleNamespace(**{k: P(v) for k, v in Wt.items()})
    cx, cw, cb = r(rows, Nc, Din), r(Nc, 128, Din), r(Nc, 128)
    cp = SimpleNamespace(enc_w=[P(cw, n * 128 * Din) for n in range(Nc)], enc_b=[P(cb, n * 128) for n in range(Nc)])
    full = lambda *s: torch.full(s, 7.0, device=DEV)   # noqa: E731
    acts = SimpleNamespace(xn=full(R * K, 64), qa=full(R, 64), qk=full(R, 64), alpha=full(R, K), xb=full(R, 64))
    cat_t, cat_i, f = full(R, 192), full(R, 192), full(rows, Nc * 128)
    tr = fused.attn_set(ap, P(own), 48, d_own, P(radar), P(nei), R, K, P(cat_t), acts=acts,
                        ride=fused.critic_enc_ride(cp, P(cx), rows, Nc, Din, f))
    inf = fused.attn_set(ap, P(own), 48, 38, P(radar), P(nei), R, 8, P(cat_i))      # a set that is fine by itself
    msg = {"K": "1 <= K <= 8", "d_own": "d_own <= 40", "c_din": "c_din <= 40"}[what]
    for launch in (fused.AttnEnc(tr), fused.AttnEnc(inf, tr)):
        with pytest.raises(RuntimeError, match=msg):
            launch()
    torch.cuda.synchronize()
    for t in (cat_t, cat_i, f, acts.xn, acts.qa, acts.qk, acts.alpha, acts.xb):
        assert bool((t == 7.0).all())
