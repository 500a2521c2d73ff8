"""The ATT learner over its whole agent range (tests/attn_cases.py).

Fused learner and act path, N = 2..9: every fused launch goes through aac_attn_enc_fwd, so N = 6..9
run attn_enc_kernel<8, 10> with the plan's own geometry (buffer offsets n * 128, ldw = 128 N,
Bt = N B), which no update had exercised; N = 9 is the edge of all its limits and N = 2 the shortest
merged schedule.  Autograd learner, N = 10 and 33: the first whole updates on the <16> and <32>
attention kernels of aac_learn.hip and the first critic with more than 16 encoders.  The grouped-GEMM
list is cut at 16 products only above nine agents, which a fused update never reaches: a direct case
runs the critic's encoder products at N = 17 and 33.

Seeds and Adam's eps per case are recorded in attn_cases.UPDATE_SEED with the CPU-only criterion they
were chosen by; the bounds are the project's (1e-5 for Q, targets, losses and parameters)."""
import functools

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import attn_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("s_own", "s_radar", "s_nei", "act", "rew", "done", "n_own", "n_radar", "n_nei")


def _case_id(c):
    return "N%d-B%d" % c[:2]


def _check(cls, case):
    N, B, E, iters = case
    seed, eps = C.UPDATE_SEED[case]
    return learner_ref.check_one_update(cls, device=DEV, N=N, B=B, E=E, tol=C.TOL, seed=seed, iters=iters, eps=eps)


@pytest.mark.parametrize("case", C.UPDATE_FUSED, ids=_case_id)
def test_fused_update_matches_cpu_restatement(native_lib, case):
    from multi_agent_aac_amd.maddpg import MADDPG
    assert C.fused_accepts(case[0])
    assert _check(MADDPG, case)


@pytest.mark.parametrize("form", C.FORMS_N9)
def test_fused_update_launch_forms_at_nine_agents(native_lib, monkeypatch, form):
    """N = 9 in the non-default launch forms: AAC_DAOB = 0 (the critic data gradient and the actor
    output backward as two launches) and AAC_ATTN_WN = 0 (the attention backward writes the dx_j rows
    and the neighbour encoder's weight gradient is a product over them: the ``dxn`` branch that the
    default takes only above K = 8, where the fused learner does not run)."""
    from multi_agent_aac_amd import fused
    from multi_agent_aac_amd.maddpg import MADDPG
    case = next(c for c in C.UPDATE_FUSED if c[0] == 9)
    if form == "daob_off":
        monkeypatch.setattr(fused.FusedUpdate, "DAOB", False)
    else:
        monkeypatch.setenv("AAC_ATTN_WN", "0")
    made = []

    def cls(*a, **k):
        made.append(MADDPG(*a, **k))
        return made[-1]
    assert _check(cls, case)
    plans = list(made[0]._fplans.values())
    assert plans and all(p.wn_part == (form != "wn_off") and p.DAOB == (form != "daob_off") for p in plans)


def _filled_model(N, B, E, **kw):
    from multi_agent_aac_amd.maddpg import MADDPG
    D0 = C.d0_of(N)
    m = MADDPG([D0, 18, 6], [D0, 18, 6], 2, n_agents=N, device=DEV, seed=4, batch_size=B, **kw)
    rep = m.attach_replay(4 * E, seed=2)
    for p in range(3):
        tr = learner_ref.random_transitions(E, N, 10 + p)
        rep.push_batch(*[tr[k].to(DEV).contiguous() for k in FIELDS])
    return m


@pytest.mark.parametrize("N", C.IDENTITY_N)
def test_graph_and_merged_schedule_identity(native_lib, monkeypatch, N):
    """Three updates at B = 64: the replayed graph gives the bits of the eager launch list, and the
    merged schedule the bits of the serial one (N = 2: ``i + 1 < N`` holds once; N = 9: eight zipped
    steps on attn_enc_kernel<8, 10>)."""
    from multi_agent_aac_amd import fused
    B, E = 64, 128
    runs = {}
    for name, merged, graph in (("graph", True, True), ("eager", True, False), ("serial", False, False)):
        monkeypatch.setattr(fused.FusedUpdate, "MERGED", merged)
        m = _filled_model(N, B, E)
        for _ in range(3):
            m.update(B, use_graph=graph)
        torch.cuda.synchronize()
        runs[name] = m
    for other in ("graph", "serial"):
        for name in ("fa", "fc", "fa_t", "fc_t"):
            assert torch.equal(getattr(runs["eager"], name).data, getattr(runs[other], name).data), (other, name)
        for opt in ("actor_optimizer", "critic_optimizer"):
            a, b = getattr(runs["eager"], opt), getattr(runs[other], opt)
            assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq), (other, opt)
            assert int(a.step_t) == int(b.step_t) == 3 * N
    assert runs["eager"]._fused_plan(B).n_launches < runs["serial"]._fused_plan(B).n_launches


@pytest.mark.parametrize("case", C.UPDATE_AUTOGRAD, ids=_case_id)
def test_autograd_update_past_the_fused_range(native_lib, case):
    """fused=False at N = 10 (K = 9: the first K of attn_fwd / attn_bwd <16>) and N = 33 (K = 32, the last
    K of <32>; 33 critic encoders).  N = 33 runs one iteration: the CPU restatement alone takes 1.5 s
    per iteration."""
    from multi_agent_aac_amd.maddpg import MADDPG
    assert not C.fused_accepts(case[0]) and C.instance(case[0] - 1) == (16 if case[0] == 10 else 32)
    assert _check(functools.partial(MADDPG, fused=False), case)


@pytest.mark.parametrize("N", C.SPLIT_N)
def test_critic_encoder_products_are_split_past_16(native_lib, N):
    """The critic's forward encoder products and encoder weight-gradient products (``encw`` of
    FusedUpdate._critic_stages: dW_n | db_n = df_n^T [X_n | 1] in SPLIT_CRITIC partial copies) as the
    plan would list them for N agents, through ``gemm_launches``: more than GEMM_MAX products become
    several launches, each product lands in its own block, fp64 torch as the reference (tolerance of
    test_gemm_batch_grouped: 9e-6 sqrt(K))."""
    from types import SimpleNamespace

    from multi_agent_aac_amd import fused
    rows, D0 = C.SPLIT_ROWS, C.d0_of(N)
    Din, SC = D0 + 2, fused.FusedUpdate.SPLIT_CRITIC
    g = torch.Generator(device=DEV).manual_seed(N)
    r = lambda *s, sc=1.0: torch.randn(*s, device=DEV, generator=g) * sc   # noqa: E731
    P = fused.ptr
    X, W, b = r(rows, N, Din), r(N, 128, Din, sc=0.2), r(N, 128, sc=0.1)
    f, h = torch.full((rows, 128 * N), 7.0, device=DEV), torch.empty(rows, 256, device=DEV)
    cp = SimpleNamespace(enc_w=[P(W, n * 128 * Din) for n in range(N)], enc_b=[P(b, n * 128) for n in range(N)],
                         Wc=None, bc=None)
    enc, _ = fused.critic_forward_stages(cp, P(X), rows, N, Din, f, h)
    fwd = fused.gemm_launches(enc)
    assert len(enc) == N and len(fwd) == (N + fused.GEMM_MAX - 1) // fused.GEMM_MAX > 1
    assert [L.n for L in fwd] == [fused.GEMM_MAX] * (N // fused.GEMM_MAX) + [N % fused.GEMM_MAX]
    for L in fwd:
        L()
    d = lambda t: t.double().cpu()   # noqa: E731
    want = torch.relu(torch.einsum("bnd,ncd->bnc", d(X), d(W)) + d(b)).reshape(rows, N * 128)
    np.testing.assert_allclose(d(f), want, atol=9e-6 * np.sqrt(Din), rtol=1e-5)
    # weight gradients: the flat layout [enc_w (N, 128, Din) | enc_b (N, 128)] per partial copy
    df = r(rows, 128 * N, sc=0.1)
    nC = fused.padded(N * 128 * (Din + 1))
    gc = torch.zeros(SC, nC, device=DEV)
    ow, ob = (lambda n: n * 128 * Din), (lambda n: N * 128 * Din + n * 128)
    encw = [fused.prob(P(df, n * 128), P(X, n * Din), P(gc, ow(n)), 128, Din, rows, 128 * N, N * Din, Din, ta=1, ones=1,
                       cextra=P(gc, ob(n)), ksplit=SC, split_stride=nC) for n in range(N)]
    bwd = fused.gemm_launches(encw)
    assert len(bwd) == len(fwd)
    for L in bwd:
        L()
    torch.cuda.synchronize()
    tot = d(gc).sum(0)
    dW = torch.einsum("bnc,bnd->ncd", d(df).view(rows, N, 128), d(X))
    np.testing.assert_allclose(tot[:N * 128 * Din].reshape(N, 128, Din), dW, atol=9e-6 * np.sqrt(rows), rtol=1e-5)
    np.testing.assert_allclose(tot[N * 128 * Din:N * 128 * (Din + 1)].reshape(N, 128),
                               d(df).view(rows, N, 128).sum(0), atol=9e-6 * np.sqrt(rows), rtol=1e-5)
    assert float(tot[N * 128 * (Din + 1):].abs().max() if nC > N * 128 * (Din + 1) else 0.0) == 0.0     # the padding


@pytest.mark.parametrize("O", [64 * 64, 64 * 64 + 1, 33 * 128])
def test_act_bgrad_takes_layers_wider_than_4096_columns(native_lib, O):
    """ops.act_bgrad hands aac_act_bgrad one ticket per block of 64 columns.  Its cached ticket buffer
    held 64, which covers O <= 4096: the critic's stacked encoders at N = 33 are 33 * 128 = 4224 columns
    (66 blocks), so the bias gradient of the last encoder went through tickets past the buffer -- the
    defect the N = 33 update exposed.  db and gm against the column sums in fp64 (error of an M-term
    fp32 sum: M 2^-24 sum |g|), twice on the same tickets, M = 16 and 35 (one and two row blocks)."""
    from multi_agent_aac_amd import ops
    for M in (16, 35):
        g = torch.Generator().manual_seed(O + M)
        gy, y = torch.randn(M, O, generator=g), torch.randn(M, O, generator=g)
        want = gy.double() * (y > 0)
        bound = M * 2.0 ** -24 * want.abs().sum(0) + 1e-30
        for _ in range(2):
            gm, db = torch.full((M, O), 7.0, device=DEV), torch.full((O,), 7.0, device=DEV)
            ops.act_bgrad(gy.to(DEV), y.to(DEV), gm, db, 1)
            torch.cuda.synchronize()
            assert torch.equal(gm.cpu().double(), want)
            assert bool(((db.cpu().double() - want.sum(0)).abs() <= bound).all())
        tk = ops._ticket_buf(torch.device(DEV, torch.cuda.current_device()))
        assert tk.numel() >= (O + 63) // 64 and int(tk.abs().sum()) == 0
