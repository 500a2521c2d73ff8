"""Gradient clipping inside the ATT and GRU learners (``grad_clip`` / ``set_grad_clip``) against the oracle
restatements driven by ``ClippedAdam`` (tests/clip_ref.py): ``clip_grad_norm_`` ahead of every optimiser
step, as the reference's ``update()`` has it.

The bounds are never taken from the code under test: an unclipped run of the restatement on the model's
initial weights gives each network's norms, ``clip_ref.split_bounds`` puts the bound between the smallest
and the largest, and the tests assert that both outcomes (a clipped and an unclipped step) then occur per
network, in the restatement and on the device alike.
"""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from oracle import gru_ref, learner_ref
from tests import clip_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, B, E, UPDATES = 3, 64, 32, 3
D0 = 6 + 4 * (N - 1)
KEYS = clip_ref.ATT_KEYS
GRU_KEYS = KEYS + ("h_cur", "h_next")
TOL = 1e-5


def _att_model(pushes, seed=0, n=N, b=B, e=E, rep_seed=0, **kw):
    from multi_agent_aac_amd.maddpg import MADDPG
    d0 = 6 + 4 * (n - 1)
    m = MADDPG([d0, 18, 6], [d0, 18, 6], 2, n_agents=n, device=DEV, seed=seed, memory_length=4 * e, batch_size=b, **kw)
    rep = m.attach_replay(4 * e, seed=rep_seed)
    for tr in pushes:
        rep.push_batch(*[tr[k].to(DEV).contiguous() for k in KEYS])
    return m


def _ref_nets(m):
    actor, critic = learner_ref.RefActor([D0, 18, 6], 2), learner_ref.RefCritic([D0, 18, 6], N, 2)
    actor.load_state_dict({k: v.cpu() for k, v in m.actors.reference_state_dict().items()})
    critic.load_state_dict({k: v.cpu() for k, v in m.critics.reference_state_dict().items()})
    return actor, critic


@functools.lru_cache(maxsize=None)
def _att_reference():
    """The problem, the bounds from the unclipped restatement and the clipped restatement's results."""
    pushes, host, idx = clip_ref.att_problem(N, B, E, 0, UPDATES)
    m = _att_model(pushes)
    actor, critic = _ref_nets(m)
    init = (m.fa.data.cpu().clone(), m.fc.data.cpu().clone())
    _, _, free = clip_ref.att_ref_run(copy.deepcopy(actor), copy.deepcopy(critic), host, idx, None)
    bounds = clip_ref.split_bounds(free)
    stats, targets, norms = clip_ref.att_ref_run(actor, critic, host, idx, bounds)
    print("unclipped norms", free, "bounds", bounds, "clipped-run norms", norms)
    return dict(pushes=pushes, idx=idx, init=init, bounds=bounds, stats=stats, norms=norms,
                nets=(actor, critic) + targets)


@functools.lru_cache(maxsize=None)
def _att_device(fz):
    ref = _att_reference()
    m = _att_model(ref["pushes"], fused=fz)
    assert torch.equal(m.fa.data.cpu(), ref["init"][0]) and torch.equal(m.fc.data.cpu(), ref["init"][1])
    m.set_grad_clip(ref["bounds"])
    stats, recs = [], []
    for it in ref["idx"]:
        s = m.update(B, use_graph=False, idx_list=[i.to(DEV) for i in it])
        stats.append([(float(lq), float(la), q.cpu().reshape(-1), y.cpu().reshape(-1)) for lq, la, q, y in s])
        recs.append(m.clip_record())
    return dict(model=m, stats=stats, recs=recs)


@pytest.mark.parametrize("fz", [True, False], ids=["fused", "autograd"])
def test_att_matches_clipped_restatement(native_lib, fz):
    ref, dev = _att_reference(), _att_device(fz)
    m = dev["model"]
    for u in range(UPDATES):
        for (lq, la, q, y), (rlq, rla, rq, ry) in zip(dev["stats"][u], ref["stats"][u]):
            torch.testing.assert_close(q, rq.reshape(-1), rtol=TOL, atol=TOL)
            torch.testing.assert_close(y, ry.reshape(-1), rtol=TOL, atol=TOL)
            assert abs(lq - rlq) <= TOL * max(1.0, abs(rlq)) and abs(la - rla) <= TOL * max(1.0, abs(rla)), (u, lq, rlq, la, rla)
    for mine, r in zip((m.actors, m.critics, m.actors_target, m.critics_target), ref["nets"]):
        sd = mine.reference_state_dict()
        for k, v in r.state_dict().items():
            d = float((sd[k].cpu() - v).abs().max())
            assert d <= TOL, (k, d)
    # both outcomes per network, and the device and the restatement agree on how many steps clipped in
    # every update and on the norm of its last iteration
    for net, bound in zip(("critic", "actor"), ref["bounds"]):
        norms = ref["norms"][net]
        hit = [bool(clip_ref.coef_of(x, bound) < 1.0) for x in norms]
        print(net, "bound", bound, "restatement norms", norms, "device record", [r["clipped"][net] for r in dev["recs"]])
        assert any(hit) and not all(hit), (net, bound, norms)
        for u, rec in enumerate(dev["recs"]):
            assert rec["steps"][net][0] == N * (u + 1) and rec["nonfinite"][net][0] == 0
            assert rec["clipped"][net][0] == sum(hit[:N * (u + 1)]), (net, u, rec["clipped"][net], hit)
            np.testing.assert_allclose(rec["last_norm"][net][0], norms[N * (u + 1) - 1], rtol=1e-4)
            assert rec["last_coef"][net][0] == clip_ref.coef_of(rec["last_norm"][net][0], bound)
        last = dev["recs"][-1]
        assert 0 < last["clipped"][net][0] < last["steps"][net][0]
        np.testing.assert_allclose(last["max_norm_seen"][net][0], max(norms), rtol=1e-4)


def test_fused_equals_autograd_with_clipping(native_lib):
    """As test_fused_equals_autograd_learner: Q, targets and the actor loss at 1e-5, the parameters after
    the 9 Adam steps at 1e-4 (a near-zero gradient moves by ~lr whichever way it rounds)."""
    a, b = _att_device(True), _att_device(False)
    for sa, sb in zip(a["stats"], b["stats"]):
        for (lqa, laa, qa, ya), (lqb, lab, qb, yb) in zip(sa, sb):
            np.testing.assert_allclose(qa, qb, atol=1e-5, rtol=1e-5)
            np.testing.assert_allclose(ya, yb, atol=1e-5, rtol=1e-5)
            np.testing.assert_allclose(laa, lab, atol=1e-5, rtol=1e-5)
    ma, mb = a["model"], b["model"]
    for x, y in ((ma.fa.data, mb.fa.data), (ma.fc.data, mb.fc.data), (ma.fa_t.data, mb.fa_t.data)):
        np.testing.assert_allclose(x.cpu(), y.cpu(), atol=1e-4, rtol=1e-5)
    for ra, rb in zip(a["recs"], b["recs"]):
        for net in ("critic", "actor"):
            assert ra["clipped"][net][0] == rb["clipped"][net][0]
            np.testing.assert_allclose(ra["last_norm"][net], rb["last_norm"][net], rtol=1e-4)


def _state(m):
    return [m.fa.data, m.fc.data, m.fa_t.data, m.fc_t.data] + m.actor_optimizer.state() + m.critic_optimizer.state()


def _same(a, b):
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)


def _pushes(n, e, seed=7):
    return [learner_ref.random_transitions(e, n, seed + p) for p in range(3)]


def test_att_inf_bound_is_bit_equal_to_off(native_lib):
    pushes = _pushes(N, 2 * E)
    off, inf = _att_model(pushes, seed=2, rep_seed=5), _att_model(pushes, seed=2, rep_seed=5, grad_clip=math.inf)
    assert off.clip is None and inf.clip is not None
    for _ in range(2):
        off.update(B, use_graph=False, want_stats=False)
        inf.update(B, use_graph=False, want_stats=False)
    torch.cuda.synchronize()
    _same(off, inf)
    assert torch.equal(off.fc.grad, inf.fc.grad) and torch.equal(off.fa.grad, inf.fa.grad)
    rec = inf.clip_record()
    for net in ("critic", "actor"):
        assert rec["steps"][net][0] == 2 * N and rec["clipped"][net][0] == 0 and rec["last_coef"][net][0] == 1.0
    with pytest.raises(ValueError):
        off.clip_record()


def test_att_launch_counts_and_mixed_bounds(native_lib):
    """With clipping on the plan has at most one launch more per Adam boundary (N + 1 of them); off, the
    list is today's; a (None, bound) pair clips the actor only."""
    pushes = _pushes(N, 2 * E)
    m = _att_model(pushes, seed=2)
    n_off = m._fused_plan(B).n_launches
    m.set_grad_clip(1.0)
    n_on = m._fused_plan(B).n_launches
    assert n_off < n_on <= n_off + N + 1, (n_off, n_on)
    m.set_grad_clip((None, 1e-3))
    assert m.critic_optimizer.clip_step is None and m.actor_optimizer.clip_step is not None
    m.update(B, use_graph=False, want_stats=False)
    rec = m.clip_record()
    assert rec["steps"]["critic"][0] == 0 and rec["steps"]["actor"][0] == N and rec["clipped"]["actor"][0] > 0
    m.set_grad_clip(None)
    assert m.clip is None and m._fused_plan(B).n_launches == n_off


def test_att_graph_replay_equals_eager_and_set_grad_clip_drops_the_graph(native_lib):
    pushes = _pushes(N, 2 * E)
    ms = [_att_model(pushes, seed=1, rep_seed=9, grad_clip=(2.0, 0.05)) for _ in range(2)]
    for _ in range(3):
        ms[0].update(B, use_graph=True, want_stats=False)
        ms[1].update(B, use_graph=False, want_stats=False)
    torch.cuda.synchronize()
    _same(ms[0], ms[1])
    ra, rb = ms[0].clip_record(), ms[1].clip_record()
    for f in clip_ref.FIELDS:
        for net in ("critic", "actor"):
            assert np.array_equal(ra[f][net], rb[f][net]), (f, net)
    assert ra["steps"]["critic"][0] == 3 * N       # the capture's warm-up updates left no record
    # a new bound drops the captured graph; the next (captured) update uses it
    assert ms[0].has_graph()
    for m in ms:
        m.set_grad_clip(1e-4)
    assert not ms[0].has_graph()
    ms[0].update(B, use_graph=True, want_stats=False)
    ms[1].update(B, use_graph=False, want_stats=False)
    torch.cuda.synchronize()
    _same(ms[0], ms[1])
    rec = ms[0].clip_record()
    for net in ("critic", "actor"):
        assert rec["steps"][net][0] == N and rec["clipped"][net][0] == N      # the record restarted; 1e-4 clips all
        assert rec["last_coef"][net][0] == clip_ref.coef_of(rec["last_norm"][net][0], 1e-4)


def test_att_monitor_shows_the_pre_clip_norm(native_lib):
    from multi_agent_aac_amd.monitor import LearnerMonitor
    pushes = _pushes(N, 2 * E)
    m = _att_model(pushes, seed=3, grad_clip=(2.0, 0.05))
    m.attach_monitor(LearnerMonitor(N, ring=4, device=DEV))
    m.update(B, use_graph=False, want_stats=False)
    rec, mon = m.clip_record(), m.monitor.read()
    for net in ("critic", "actor"):
        # column N - 1 = the last gradient iteration, the one last_norm describes
        np.testing.assert_allclose(mon[f"grad_norm_{net}"][-1, N - 1], rec["last_norm"][net][0], rtol=1e-6)
    assert rec["clipped"]["critic"][0] + rec["clipped"]["actor"][0] > 0


def test_att_world2_schedule_equals_one_rank(native_lib):
    """The world = 2 schedule on one GPU (partial sums, collective, aac_clip_sumsq with nsplit = 1 and
    gscale = 1 / 2, aac_adam_flat_clip), the collective standing in for two ranks with identical shards
    (SUM = 2 g): the mean gradient is g exactly, so the update is bit-equal to the world = 1 clipped update."""
    pushes = _pushes(N, 2 * E)
    one = _att_model(pushes, seed=4, rep_seed=3, grad_clip=(2.0, 0.05))
    two = _att_model(pushes, seed=4, rep_seed=3)
    two.world = 2
    two._share_grads()
    calls = []

    def allreduce(critic, actor):
        nc = two.fc.numel
        t = two.grads if (critic and actor) else (two.grads[:nc] if critic else two.grads[nc:])
        t.mul_(2.0)
        calls.append((critic, actor))
    two._allreduce_grads = allreduce
    two.set_grad_clip((2.0, 0.05))
    for _ in range(2):
        one.update(B, use_graph=False, want_stats=False)
        two.update(B, use_graph=False, want_stats=False)
    torch.cuda.synchronize()
    assert len(calls) == 2 * (N + 1)
    _same(one, two)
    ra, rb = one.clip_record(), two.clip_record()
    for f in clip_ref.FIELDS:
        for net in ("critic", "actor"):
            assert np.array_equal(ra[f][net], rb[f][net]), (f, net)
    assert 0 < ra["clipped"]["critic"][0] + ra["clipped"]["actor"][0]


# ------------------------------------------------------------------------------------------- GRU
def _gru_model(seed=3, n=N, b=B, e=96, **kw):
    from multi_agent_aac_amd.gru import MADDPG
    m = MADDPG([6, 18, 6], [6, 18, 6], 2, 64, 10, n_agents=n, device=DEV, seed=seed, batch_size=b, **kw)
    rep = m.attach_replay(4 * e, seed=seed + 3)
    host = {k: [] for k in GRU_KEYS}
    for p in range(3):
        tr = gru_ref.random_gru_transitions(e, n, 10 * n + p)
        rep.push_batch(*[tr[k].to(DEV).contiguous() for k in GRU_KEYS])
        for k in GRU_KEYS:
            host[k].append(tr[k])
    return m, rep, {k: torch.cat(v) for k, v in host.items()}


def _gru_ref_nets(m):
    n, d = m.n_agents, m.d_own
    actors = [gru_ref.RefGRUActor([d, 18, 6], 2) for _ in range(n)]
    critics = [gru_ref.RefGRUCritic([d, 18, 6], 2) for _ in range(n)]
    for i in range(n):
        actors[i].load_state_dict({k: v.cpu() for k, v in m.actors[i].state_dict().items()})
        critics[i].load_state_dict({k: v.cpu() for k, v in m.critics[i].state_dict().items()})
    return actors, critics


def _gru_ref_run(actors, critics, batches, d_own, bounds, eps):
    actors_t, critics_t = copy.deepcopy(actors), copy.deepcopy(critics)
    bc, ba = bounds if bounds is not None else (None, None)
    opts = ([clip_ref.ClippedAdam(a.parameters(), ba, lr=1e-3, eps=eps) for a in actors],
            [clip_ref.ClippedAdam(c.parameters(), bc, lr=1e-3, eps=eps) for c in critics])
    stats = []
    for b in batches:
        s, opts = gru_ref.ref_gru_update(actors, critics, actors_t, critics_t, b, d_own, opts=opts)
        stats.append(s)
    norms = {"actor": [o.norms for o in opts[0]], "critic": [o.norms for o in opts[1]]}
    return stats, (actors_t, critics_t), norms


def test_gru_matches_clipped_restatement(native_lib):
    """One ClippedAdam per agent network; tolerances and eps = 1e-3 of test_gru_update_matches_cpu_restatement.
    The unit is the agent: per-agent last_norm and clipped counts against the restatement's."""
    eps = 1e-3
    m, rep, host = _gru_model()
    m.actor_optimizer.eps = m.critic_optimizer.eps = eps
    actors, critics = _gru_ref_nets(m)
    gen = np.random.default_rng(N)
    idx = [torch.from_numpy(gen.choice(len(rep), size=B, replace=False).astype(np.int32)) for _ in range(UPDATES)]
    batches = []
    for i in idx:
        b = {k: v[i.long()].clone() for k, v in host.items()}
        b["done"] = b["done"].float()
        batches.append(b)
    _, _, free = _gru_ref_run(copy.deepcopy(actors), copy.deepcopy(critics), batches, m.d_own, None, eps)
    flat = {k: [x for agent in v for x in agent] for k, v in free.items()}
    bounds = clip_ref.split_bounds(flat)
    rstats, (actors_t, critics_t), norms = _gru_ref_run(actors, critics, batches, m.d_own, bounds, eps)
    print("unclipped norms", free, "bounds", bounds, "clipped-run norms", norms)
    m.set_grad_clip(bounds)
    for u, i in enumerate(idx):
        stats = m.update(B, use_graph=False, idx=i.to(DEV))
        for ag, ((lq, la, q, tg), (rlq, rla, rq, rtg)) in enumerate(zip(stats, rstats[u])):
            dt, dqv = float((tg.cpu() - rtg).abs().max()), float((q.cpu() - rq).abs().max())
            assert dt < 2e-5 * max(1.0, float(rtg.abs().max())), ("target", u, ag, dt)
            assert dqv < 2e-5 * max(1.0, float(rq.abs().max())), ("q", u, ag, dqv)
            assert abs(float(lq) - rlq) <= 1e-4 * max(1.0, abs(rlq)), ("loss_q", u, ag, float(lq), rlq)
            assert abs(float(la) - rla) <= 1e-4 * max(1.0, abs(rla)), ("loss_a", u, ag, float(la), rla)
        rec = m.clip_record()
        for net, bound in zip(("critic", "actor"), bounds):
            want = [norms[net][ag][u] for ag in range(N)]
            np.testing.assert_allclose(rec["last_norm"][net], want, rtol=1e-4)
            assert list(rec["steps"][net]) == [u + 1] * N and not rec["nonfinite"][net].any()
            assert list(rec["clipped"][net]) == [sum(bool(clip_ref.coef_of(x, bound) < 1.0) for x in norms[net][ag][:u + 1])
                                                 for ag in range(N)], (net, u)
    for i in range(N):
        for mine, ref in ((m.actors[i], actors[i]), (m.critics[i], critics[i]),
                          (m.actors_target[i], actors_t[i]), (m.critics_target[i], critics_t[i])):
            for (k, v), (_, rv) in zip(mine.state_dict().items(), ref.state_dict().items()):
                d = float((v.cpu() - rv).abs().max())
                assert d < 2e-5, (i, k, d)
    rec = m.clip_record()
    for net in ("critic", "actor"):
        total = int(rec["clipped"][net].sum())
        assert 0 < total < N * UPDATES, (net, rec["clipped"][net])


def test_gru_inf_graph_and_monitor(native_lib):
    """GRU: grad_clip = inf is bit-equal to off; with a bound the graph replay is bit-equal to eager; the
    monitor's per-agent gradient norm is the record's last_norm (the pre-clip gradient in both)."""
    from multi_agent_aac_amd.monitor import LearnerMonitor
    off, inf = _gru_model(seed=1)[0], _gru_model(seed=1, grad_clip=math.inf)[0]
    for _ in range(2):
        off.update(B, use_graph=False, want_stats=False)
        inf.update(B, use_graph=False, want_stats=False)
    torch.cuda.synchronize()
    _same(off, inf)
    assert list(inf.clip_record()["steps"]["critic"]) == [2] * N
    ga, gb = _gru_model(seed=2, grad_clip=(1.0, 0.05))[0], _gru_model(seed=2, grad_clip=(1.0, 0.05))[0]
    for g in (ga, gb):
        g.attach_monitor(LearnerMonitor(N, ring=4, device=DEV))
    for _ in range(3):
        ga.update(B, use_graph=True, want_stats=False)
        gb.update(B, use_graph=False, want_stats=False)
    torch.cuda.synchronize()
    _same(ga, gb)
    ra, rb = ga.clip_record(), gb.clip_record()
    mon = gb.monitor.read()
    for net in ("critic", "actor"):
        for f in clip_ref.FIELDS:
            assert np.array_equal(ra[f][net], rb[f][net]), (f, net)
        assert list(ra["steps"][net]) == [3] * N
        np.testing.assert_allclose(mon[f"grad_norm_{net}"][-1], rb["last_norm"][net], rtol=1e-6)
    assert ga.has_graph()
    ga.set_grad_clip(None)
    assert not ga.has_graph() and ga.clip is None
