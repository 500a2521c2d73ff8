"""Exploration maps in the training loops (``Trainer(..., visits=True)``, ``UamTrainer``) and the
evaluator: off by default; when on they change nothing they observe; eager steps, whole-step graphs
and a resumed run give bit-equal tables; ``finish()`` returns them.  Shapes as
tests/test_stats_trainer_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODELS = ["att", "gru", "uam"]
VIS = dict(explore_until=1)       # the first episode of an env is "explore", later ones "exploit"


def _trainer(model, visits, seed=1):
    from multi_agent_aac_amd import trainer
    if model == "uam":
        return trainer.UamTrainer(8, 5, 8, 4096, seed=seed, visits=visits)
    return trainer.Trainer(64, 3, 32, 4096, "combined", seed=seed, model=model, visits=visits)


def _snapshot(tr):
    """Learner, replay (the whole ring), env state and loop rows -- everything but the maps themselves."""
    from multi_agent_aac_amd import checkpoint
    torch.cuda.synchronize()
    out = {"L." + k: v.clone() for k, v in checkpoint.learner_tensors(tr.model).items()}
    out.update({"R." + k: v.clone() for k, v in checkpoint.replay_tensors(tr.replay).items()})
    out.update({"E." + k: v.clone() for k, v in checkpoint.env_tensors(tr.env).items()})
    out.update({"X." + k: v.clone() for k, v in tr.checkpoint_parts()["extra"].items() if not k.startswith("visits.")})
    return out


def _raw(tr):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in tr.visits.tensors().items()}


def _same(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else np.array_equal(a[k], b[k]))]
    assert not bad, bad


@pytest.mark.parametrize("model", MODELS)
def test_visits_off_by_default_and_observe_only(native_lib, model):
    a, b = _trainer(model, visits=VIS), _trainer(model, visits=False)
    assert b.visits is None and b.finish() is None
    assert not any(k.startswith("visits.") for k in b.checkpoint_parts()["extra"])
    assert a.visits is not None and (a.visits.E, a.visits.N, a.visits.explore_until) == (a.E, a.N, 1)
    k = 8
    for t in (a, b):
        for _ in range(k):
            t.step(update=True)
    _same(_snapshot(a), _snapshot(b))
    out = a.finish()["visits"]
    assert out["samples"].sum() == k * a.E * a.N == out["pos"].sum() + out["pos_outside"].sum()
    assert out["act"].sum() + out["act_outside"].sum() == k * a.E * a.N and out["act_outside"].sum() == 0
    assert out["bad_map"] == 0 and out["pos"].shape == (1, 2, 50, 50) and out["act"].shape == (2, 20, 20)
    # the default geometry and period
    d = _trainer(model, visits=True).visits
    assert (d.GX, d.GY, d.A, d.explore_until) == (50, 50, 20, 10000 if model == "uam" else 8000)


@pytest.mark.parametrize("model", MODELS)
def test_eager_graph_and_resume_agree(native_lib, monkeypatch, tmp_path, model):
    from multi_agent_aac_amd import trainer
    monkeypatch.setattr(trainer, "STEP_GRAPH", True)
    monkeypatch.setattr(trainer, "STEP_GRAPH_GRU", True)
    a = _trainer(model, visits=VIS)
    for _ in range(5):
        a.step(update=True)
    path = str(tmp_path / f"{model}.ckpt")
    a.save_checkpoint(path)
    mid = _raw(a)
    assert mid["counters"][:, 0].sum() == 5 * a.E * a.N
    for _ in range(6):
        a.step(update=True)
    want, snap = _raw(a), _snapshot(a)
    assert want["counters"][:, 0].sum() == 11 * a.E * a.N
    # whole-step graphs from the same checkpoint: one step per replay, then two per replay (the fresh
    # loops below take steps of their own first, so the load has something to overwrite)
    g = _trainer(model, visits=VIS)
    for _ in range(2):
        g.step(update=True)
    g.load_checkpoint(path)
    _same(_raw(g), mid)
    g.step_graph()
    g.step_graph()
    g.step_graph_pair()
    g.step_graph_pair()
    _same(_raw(g), want)
    _same(_snapshot(g), snap)
    out = g.finish()["visits"]
    assert np.array_equal(out["pos"].reshape(want["pos_hist"].shape), want["pos_hist"])
    # a resumed eager run
    r = _trainer(model, visits=VIS)
    for _ in range(3):
        r.step(update=False)
    r.load_checkpoint(path)
    for _ in range(6):
        r.step(update=True)
    _same(_raw(r), want)


def test_unfused_tail_counts_the_same(native_lib):
    a, b = _trainer("att", visits=VIS), _trainer("att", visits=VIS)
    b.fused_tail = False
    for t in (a, b):
        for _ in range(6):
            t.step(update=True)
    _same(_raw(a), _raw(b))


def test_checkpoint_without_visits_is_refused(native_lib, tmp_path):
    """A file saved by a trainer without the maps names the missing tensor and changes nothing."""
    a, b = _trainer("att", visits=False), _trainer("att", visits=VIS)
    for t in (a, b):
        t.step(update=True)
    path = str(tmp_path / "plain.ckpt")
    a.save_checkpoint(path)
    before, raw = _snapshot(b), _raw(b)
    with pytest.raises(KeyError, match="visits."):
        b.load_checkpoint(path)
    _same(_snapshot(b), before)
    _same(_raw(b), raw)
    b.save_checkpoint(path)
    a.load_checkpoint(path)       # the other direction loads: the plain trainer asks for no visits tensor


@pytest.mark.parametrize("model", MODELS)
def test_evaluator_keeps_a_map(native_lib, model):
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = _trainer(model, visits=False)
    for _ in range(3):
        tr.step(update=True)
    before = _snapshot_plain(tr)
    ev = Evaluator(tr, E=32 if model == "uam" else 16, visits=dict(explore_until=1000))
    st = ev.evaluate(1)
    out = ev.visits.read()
    # the map holds the episodes the statistics count: one action per step of every counted episode
    assert st["episodes"] == ev.E and out["samples"].sum() == st["steps"] * ev.N
    # the training env's counters are at most a few episodes: every sample is "explore"
    assert int(tr.episode.min()) <= 1000 and out["samples"][:, 1].sum() == 0 and out["act"][1].sum() == 0
    assert out["pos"].sum() + out["pos_outside"].sum() == out["samples"].sum() and out["act_outside"].sum() == 0
    # a second call replays the same episode set into an emptied map
    st2 = ev.evaluate(1)
    out2 = ev.visits.read()
    assert st2["steps"] == st["steps"] and np.array_equal(out2["pos"], out["pos"]) and np.array_equal(out2["act"], out["act"])
    # past the training loop's noise schedule the same rollout lands in "exploit"
    ev.visits.explore_until = 0
    ev.evaluate(1)
    out3 = ev.visits.read()
    assert np.array_equal(out3["pos"][:, 1], out["pos"][:, 0]) and out3["samples"][:, 0].sum() == 0
    assert np.array_equal(out3["act"][1], out["act"][0])
    _same(_snapshot_plain(tr), before)       # the training loop is untouched
    assert Evaluator(tr, E=8).visits is None


def _snapshot_plain(tr):
    from multi_agent_aac_amd import checkpoint
    torch.cuda.synchronize()
    out = {"L." + k: v.clone() for k, v in checkpoint.learner_tensors(tr.model).items()}
    out.update({"E." + k: v.clone() for k, v in checkpoint.env_tensors(tr.env).items()})
    return out
