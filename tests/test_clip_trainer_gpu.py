"""Gradient clipping in the training loops: ``Trainer(..., grad_clip=...)`` passes the bound to the model,
the whole-step graphs pick the two launches up through the update's launch list (replays bit-equal to
eager steps), ``finish()`` returns the record under ``"clip"``, and ``UamTrainer`` refuses."""
import numpy as np
import pytest
import torch

from tests import clip_ref

pytestmark = pytest.mark.gpu
E, N, B = 64, 3, 32


def _trainer(model, **kw):
    from multi_agent_aac_amd import trainer
    return trainer.Trainer(E, N, B, 4096, "combined", seed=1, model=model, **kw)


def _snapshot(tr):
    from multi_agent_aac_amd import checkpoint
    torch.cuda.synchronize()
    out = {"L." + k: v.clone() for k, v in checkpoint.learner_tensors(tr.model).items()}
    out.update({"R." + k: v.clone() for k, v in checkpoint.replay_tensors(tr.replay).items()})
    out.update({"E." + k: v.clone() for k, v in checkpoint.env_tensors(tr.env).items()})
    out.update({"M." + k: v.clone().view(torch.int64) for k, v in tr.monitor.tensors().items()})
    out["clip"] = tr.model.clip.record.clone().view(torch.int64)
    return out


@pytest.mark.parametrize("model", ["att", "gru"])
def test_graph_steps_equal_eager_steps(native_lib, model):
    g, e = (_trainer(model, grad_clip=1.0, monitor=True) for _ in range(2))
    for t in (g, e):
        for _ in range(2):
            t.step(update=True)
    assert g.graph_ok()
    for _ in range(2):
        g.step_graph_pair()
    for _ in range(4):
        e.step(update=True)
    a, b = _snapshot(g), _snapshot(e)
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad
    updates = 6
    out = g.finish()
    rec = out["clip"]
    assert set(rec) == set(clip_ref.FIELDS)
    for net in ("critic", "actor"):
        units = 1 if model == "att" else N
        per_update = N if model == "att" else 1       # Adam boundaries per unit and update
        assert list(rec["steps"][net]) == [updates * per_update] * units
        assert not rec["nonfinite"][net].any() and np.isfinite(rec["last_norm"][net]).all()
        assert (rec["clipped"][net] <= rec["steps"][net]).all()
        # the monitor shows the same (pre-clip) gradient: its last record's norm is last_norm
        mon = g.monitor.read()[f"grad_norm_{net}"][-1]
        # (ATT: column N - 1 is the last gradient iteration; GRU: column i is agent i, the unit)
        np.testing.assert_allclose(mon[-1:] if model == "att" else mon, rec["last_norm"][net], rtol=1e-6)
    assert int(rec["clipped"]["critic"].sum()) + int(rec["clipped"]["actor"].sum()) > 0
    assert "clip" not in g.checkpoint_parts()["extra"] and not any("clip" in k for k in g.checkpoint_parts()["extra"])


def test_off_by_default_and_set_grad_clip_recaptures(native_lib):
    plain, on = _trainer("att"), _trainer("att", grad_clip=0.5)
    assert plain.model.clip is None and plain.finish() is None
    n_off, n_on = plain.model._fused_plan(B).n_launches, on.model._fused_plan(B).n_launches
    assert n_off < n_on <= n_off + N + 1
    for _ in range(2):
        on.step(update=True)
    on.step_graph()
    assert on._sg
    on.model.set_grad_clip(1e-4)           # new plans: the whole-step graphs are captured again
    on.step_graph()
    rec = on.finish()["clip"]
    assert rec["steps"]["critic"][0] == N and rec["clipped"]["critic"][0] == N and rec["clipped"]["actor"][0] == N


def test_uam_trainer_refuses(native_lib):
    from multi_agent_aac_amd import trainer
    with pytest.raises(NotImplementedError, match="UAM"):
        trainer.UamTrainer(8, 5, 8, 4096, seed=1, grad_clip=1.0)
