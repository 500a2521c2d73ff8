"""The learner monitor in the training loops (``Trainer(..., monitor=True)``, ``UamTrainer``): off by
default with unchanged launch lists; observe-only; records equal to tests/monitor_ref.py of the buffers
the launches read; eager steps, whole-step graphs and a resumed run give bit-equal records; the sticky
non-finite word; the refusals."""
import math

import numpy as np
import pytest
import torch

import monitor_ref

pytestmark = pytest.mark.gpu

MODELS = ["att", "gru", "uam"]
U24, U53 = 2.0 ** -24, 2.0 ** -53


def _trainer(model, monitor=False, seed=1, **kw):
    from multi_agent_aac_amd import trainer
    if model == "uam":
        return trainer.UamTrainer(8, 5, 8, 4096, seed=seed, monitor=monitor, **kw)
    return trainer.Trainer(64, 3, 32, 4096, "combined", seed=seed, model=model, monitor=monitor, **kw)


def _plan(tr, model):
    """(the update plan, its op list)."""
    if model == "att":
        p = tr.model._fused_plan(tr.B)
        return p, p.ops()
    if model == "gru":
        p = tr.model._plan(tr.B)
        return p, p.ops()
    p = tr.model.fused(tr.B, tr.replay)
    return p, list(p._launches)


def _snapshot(tr):
    """Learner, replay, env state and loop rows -- everything but the monitor itself."""
    from multi_agent_aac_amd import checkpoint
    torch.cuda.synchronize()
    out = {"L." + k: v.clone() for k, v in checkpoint.learner_tensors(tr.model).items()}
    out.update({"R." + k: v.clone() for k, v in checkpoint.replay_tensors(tr.replay).items()})
    out.update({"E." + k: v.clone() for k, v in checkpoint.env_tensors(tr.env).items()})
    out.update({"X." + k: v.clone() for k, v in tr.checkpoint_parts()["extra"].items() if not k.startswith("monitor.")})
    return out


def _mon_raw(tr):
    """The monitor's tensors as bit patterns (records hold NaN where a field does not apply)."""
    torch.cuda.synchronize()
    return {k: v.clone().view(torch.int64) for k, v in tr.monitor.tensors().items()}


def _same(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad


# ------------------------------------------------------------------------------------ default off
@pytest.mark.parametrize("model", MODELS)
def test_off_by_default_with_the_same_launch_list(native_lib, model):
    from multi_agent_aac_amd import monitor
    plain, off, on = _trainer(model), _trainer(model, monitor=False), _trainer(model, monitor=True)
    for t in (plain, off):
        assert t.monitor is None and t.model.monitor is None
        assert not any(k.startswith("monitor.") for k in t.checkpoint_parts()["extra"])
    assert sorted(k for k in on.checkpoint_parts()["extra"] if k.startswith("monitor.")) == [
        "monitor.agg", "monitor.ring", "monitor.ring_update", "monitor.state"]
    n = [len(_plan(t, model)[1]) for t in (plain, off, on)]
    assert n[0] == n[1]
    if model == "att":
        assert _plan(plain, model)[0].n_launches == _plan(off, model)[0].n_launches == n[0]
        assert _plan(on, model)[0].n_launches == n[2]
    ops_on = _plan(on, model)[1]
    nvec = sum(isinstance(o, monitor.VecLaunch) for o in ops_on)
    ncommit = sum(isinstance(o, monitor.CommitLaunch) for o in ops_on)
    assert not any(isinstance(o, (monitor.VecLaunch, monitor.CommitLaunch)) for o in _plan(off, model)[1])
    assert nvec == (on.N + 1 if model == "att" else 2) and ncommit == 1 and n[2] == n[0] + nvec + ncommit
    assert isinstance(ops_on[-1], monitor.CommitLaunch)
    assert on.monitor.R == 64 and _trainer(model, monitor=7).monitor.R == 7


# ------------------------------------------------------------------------------------ observe only
@pytest.mark.parametrize("model", MODELS)
def test_observe_only(native_lib, model):
    a, b = _trainer(model, monitor=True), _trainer(model, monitor=False)
    for t in (a, b):
        for _ in range(8):
            t.step(update=True)
    _same(_snapshot(a), _snapshot(b))
    out = a.monitor.read()
    assert out["updates"] == 8 and list(out["update"]) == list(range(8)) and a.monitor.bad_update() == -1
    assert a.finish() is None
    assert np.isfinite(out["loss_q"]).all() and (out["grad_norm_critic"] > 0).all()


# ------------------------------------------------------------------------------------ records are right
def _job_arrays(g, p, j):
    """Per segment: (copies [nsplit][n], parameters [n]) of a vec job's snapshot."""
    gf, pf = g.reshape(-1)[j.get("g_off", 0):], p.reshape(-1)[j.get("p_off", 0):]
    n, ns, gs = j["n"], j.get("nsplit", 1), j.get("gstride", j["n"])
    ss = j.get("seg_stride", n)
    return [(np.stack([gf[c * gs + s * ss:c * gs + s * ss + n] for c in range(ns)]), pf[s * ss:s * ss + n])
            for s in range(j.get("nseg", 1))]


def _rows_of(model, tr, plan):
    """The row fields [A][B] the update left, downloaded from the plan's own buffers."""
    N, B = tr.N, tr.B
    c = lambda t: t.detach().cpu().numpy()      # noqa: E731
    if model == "att":
        rew, done = c(plan.rew).reshape(N, B, N), c(plan.done).reshape(N, B, N)
        return dict(q=c(plan.q_c).reshape(N, B), y=c(plan.y).reshape(N, B), q_a=c(plan.q_a).reshape(N, B),
                    reward=np.stack([rew[i, :, i] for i in range(N)]), qn=c(plan.qn).reshape(N, B), done=done,
                    a_off=0.0, gamma=tr.model.GAMMA)
    if model == "gru":
        return dict(q=c(plan.q_c).T, y=c(plan.y).T, q_a=c(plan.q_a).T, reward=c(plan.batch["rew"]).reshape(B, N).T,
                    qn=None, done=None, a_off=3.0, gamma=0.0)
    return dict(q=c(plan.q)[None], y=c(plan.y)[None], q_a=c(plan.la)[None], reward=c(plan.rows)[:, 27][None], qn=None,
                done=None, a_off=0.0, gamma=0.0)


@pytest.mark.parametrize("model", MODELS)
def test_records_equal_the_restatement(native_lib, model):
    from multi_agent_aac_amd import monitor
    tr = _trainer(model, monitor=True)
    for _ in range(3):
        tr.step(update=False)                    # fill the replay; no update yet
    plan, ops = _plan(tr, model)
    A = tr.monitor.A
    assert A == (1 if model == "uam" else tr.N)
    nets = [dict() for _ in range(A)]
    seen = {0: 0, 1: 0}
    for op in ops:
        if isinstance(op, monitor.VecLaunch):
            torch.cuda.synchronize()
            for g, p, j in op.reads:
                net = j["net"]
                # columns: ATT the k-th launch of a network is gradient iteration k; GRU one launch of N
                # per-agent segments; UAM the single column
                col0 = seen[net] if model == "att" else 0
                seen[net] += 1
                assert j.get("col0", 0) == col0
                # ATT's 16-byte aligned padded copies take the copy-parallel Adam's four-group order
                order = 1 if model == "att" else 0
                assert j.get("order", 0) == order
                segs = _job_arrays(g.detach().cpu().numpy(), p.detach().cpu().numpy(), j)
                assert len(segs) == (tr.N if model == "gru" else 1)
                for s, (copies, par) in enumerate(segs):
                    nets[col0 + s][monitor.NETS[net]] = monitor_ref.vec(copies, par, 1.0, order)
                if model == "att":
                    # the Adam launch stored the gradient it formed: the restatement's sum is that, bit for bit
                    flat = tr.model.fc if net == 0 else tr.model.fa
                    want = monitor_ref.sum_copies(segs[0][0], order)
                    np.testing.assert_array_equal(want.view(np.uint32), flat.grad.cpu().numpy().view(np.uint32))
        op()
    torch.cuda.synchronize()
    assert all(set(n) == {"critic", "actor"} for n in nets)
    if model == "att":
        assert seen == {0: tr.N, 1: tr.N}
    f = _rows_of(model, tr, plan)
    want, tol = np.zeros((A, monitor.FIELDS)), np.zeros((A, monitor.FIELDS))
    for c in range(A):
        rf, rt = monitor_ref.rows(f["q"][c], f["y"][c], f["q_a"][c], f["reward"][c], f["a_off"],
                                  None if f["qn"] is None else f["qn"][c], None if f["done"] is None else f["done"][c],
                                  f["gamma"])
        want[c], tol[c] = monitor_ref.record_row(rf, rt, nets[c])
    got = tr.monitor.ring.cpu().numpy()[0]
    print(model, "record", got, "want", want)
    ok = monitor_ref.close(got, want, tol)
    assert ok.all(), (np.argwhere(~ok), got[~ok], want[~ok])
    out = tr.monitor.read()
    assert out["updates"] == 1 and out["bad_update"] == -1
    assert (got[:, monitor_ref.F["critic_grad_sumsq"]] > 0).all() and (got[:, monitor_ref.F["actor_grad_sumsq"]] > 0).all()
    # the independent cross-check: the learners' own loss values (fp32 means: B * 2^-24 relative to the
    # mean magnitude of the terms; UAM's float64 means: the double bound)
    B = tr.B
    if model == "uam":
        lq, la = float(plan.loss[0]), float(plan.loss[1])
        e2, qa = (f["q"][0] - f["y"][0]) ** 2, f["q_a"][0]
        assert abs(got[0, 0] - lq) <= 2 * (B + 2) * U53 * float(np.mean(e2))
        assert abs(got[0, 1] - la) <= 2 * (B + 2) * U53 * float(np.mean(np.abs(qa)))
    else:
        for c, (lq, la, _, _) in enumerate(plan.stats()):
            e2 = (f["q"][c].astype(np.float64) - f["y"][c]) ** 2
            assert abs(got[c, 0] - float(lq)) <= (B + 4) * U24 * float(np.mean(e2)), (c, got[c, 0], float(lq))
            assert abs(got[c, 1] - float(la)) <= (B + 4) * U24 * (float(np.mean(np.abs(f["q_a"][c]))) + f["a_off"]), c


# ------------------------------------------------------------------------------------ eager = graph = resumed
@pytest.mark.parametrize("model", MODELS)
def test_eager_graph_and_resume_agree(native_lib, monkeypatch, tmp_path, model):
    from multi_agent_aac_amd import trainer
    monkeypatch.setattr(trainer, "STEP_GRAPH", True)
    monkeypatch.setattr(trainer, "STEP_GRAPH_GRU", True)
    a = _trainer(model, monitor=4)
    for _ in range(5):
        a.step(update=True)
    path = str(tmp_path / f"{model}.ckpt")
    a.save_checkpoint(path)
    mid = _mon_raw(a)
    for _ in range(6):
        a.step(update=True)
    want, snap = _mon_raw(a), _snapshot(a)
    assert int(want["state"][0]) == 11 and int(want["state"][1]) == -1 and a.monitor.read()["updates"] == 11
    assert sorted(want["ring_update"].tolist()) == [7, 8, 9, 10]
    g = _trainer(model, monitor=4)
    for _ in range(2):
        g.step(update=True)
    g.load_checkpoint(path)
    _same(_mon_raw(g), mid)
    g.step_graph()
    g.step_graph()
    g.step_graph_pair()
    g.step_graph_pair()
    _same(_mon_raw(g), want)
    _same(_snapshot(g), snap)
    assert g.finish() is None


def test_checkpoint_without_monitor_is_refused(native_lib, tmp_path):
    a, b = _trainer("att"), _trainer("att", monitor=True)
    for t in (a, b):
        t.step(update=True)
    path = str(tmp_path / "plain.ckpt")
    a.save_checkpoint(path)
    before, raw = _snapshot(b), _mon_raw(b)
    with pytest.raises(KeyError, match="monitor."):
        b.load_checkpoint(path)
    _same(_snapshot(b), before)
    _same(_mon_raw(b), raw)


# ------------------------------------------------------------------------------------ watchdog
@pytest.mark.parametrize("model", MODELS)
def test_watchdog_names_the_first_nonfinite_update(native_lib, model):
    from multi_agent_aac_amd import checkpoint
    tr = _trainer(model, monitor=True)
    k = 3
    for _ in range(k):
        tr.step(update=True)
    assert tr.monitor.bad_update() == -1 and tr.finish() is None
    # NaN arithmetic is ordinary data: one critic parameter becomes NaN before update k
    lt = checkpoint.learner_tensors(tr.model)
    (lt["flat"] if model == "uam" else lt["fc"])[0] = math.nan
    tr.step(update=True)      # one step only: its update turns the actor NaN, which no env step should see
    assert tr.monitor.bad_update() == k
    out = tr.monitor.read()
    assert out["critic_param_nonfinite"][k].sum() >= 1 and out["critic_param_nonfinite"][k - 1].sum() == 0
    with pytest.raises(FloatingPointError, match=f"update {k}"):
        tr.finish()


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("model", MODELS)
def test_refusals(native_lib, model):
    from multi_agent_aac_amd import monitor
    tr = _trainer(model)
    A, dt = (1, torch.float64) if model == "uam" else (tr.N, torch.float32)
    mon = monitor.LearnerMonitor(A, dtype=dt)
    # more than one rank (the model's own world size; no second process is needed to refuse)
    tr.model.world = 2
    with pytest.raises(ValueError, match="world"):
        tr.model.attach_monitor(mon)
    tr.model.world = 1
    # the autograd learners
    if model == "att":
        tr.model.fused = False
        with pytest.raises(ValueError, match="fused"):
            tr.model.attach_monitor(mon)
        tr.model.fused = True
        tr.model.attach_monitor(mon)
        for _ in range(2):
            tr.step(update=False)
        with pytest.raises(ValueError, match="fused learner only"):
            tr.model.update(tr.B, freeze_actor=True)
    elif model == "uam":
        tr.model.fused_learner = False
        with pytest.raises(ValueError, match="fused"):
            tr.model.attach_monitor(mon)
        tr.model.fused_learner = True
    # a monitor of another shape
    with pytest.raises(ValueError):
        tr.model.attach_monitor(monitor.LearnerMonitor(A + 1, dtype=dt))
    assert tr.model.monitor is None or model == "att"
    # attaching and detaching drop the cached plans
    tr.model.attach_monitor(mon)
    p1 = _plan(tr, model)[0]
    tr.model.attach_monitor(None)
    p2 = _plan(tr, model)[0]
    assert p1 is not p2 and p2.mon is None and p1.mon is mon
