"""Episode statistics in the training loops (``Trainer(..., stats=True)``, ``UamTrainer``):
off by default; when on they change nothing they observe; eager steps, whole-step graphs and a
resumed run give bit-equal tallies; ``finish()`` returns them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODELS = ["att", "gru", "uam"]


def _trainer(model, stats, seed=1):
    from multi_agent_aac_amd import trainer
    if model == "uam":
        # 8 envs x 5 aircraft (tests/test_uam_gpu.py runs 6 x 5 and 8 x 3, tests/test_uam_learner_gpu.py
        # learners of 5 and 3).  Not 3 aircraft: the evaluator test rolls 32 envs, and the UAM step
        # kernel finishes only the first 16 envs of a workgroup, which holds 64 // N of them -- more
        # than 16 for N < 4 (envs 16.. of each workgroup then never end an episode)
        return trainer.UamTrainer(8, 5, 8, 4096, seed=seed, stats=stats)
    return trainer.Trainer(64, 3, 32, 4096, "combined", seed=seed, model=model, stats=stats)


def _snapshot(tr):
    """Learner, replay, env state and loop rows -- everything but the statistics themselves."""
    from multi_agent_aac_amd import checkpoint
    torch.cuda.synchronize()
    out = {"L." + k: v.clone() for k, v in checkpoint.learner_tensors(tr.model).items()}
    out.update({"R." + k: v.clone() for k, v in checkpoint.replay_tensors(tr.replay).items()})
    out.update({"E." + k: v.clone() for k, v in checkpoint.env_tensors(tr.env).items()})
    out.update({"X." + k: v.clone() for k, v in tr.checkpoint_parts()["extra"].items() if not k.startswith("stats.")})
    return out


def _stats_raw(tr):
    torch.cuda.synchronize()
    d = {k: v.cpu().numpy() for k, v in tr.stats.tensors().items()}
    d["totals"] = tr.stats._reduce().copy()
    return d


def _same(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else np.array_equal(a[k], b[k]))]
    assert not bad, bad


@pytest.mark.parametrize("model", MODELS)
def test_stats_off_by_default_and_observe_only(native_lib, model):
    a, b = _trainer(model, stats=True), _trainer(model, stats=False)
    assert b.stats is None and b.finish() is None
    assert not any(k.startswith("stats.") for k in b.checkpoint_parts()["extra"])
    assert a.stats is not None and (a.stats.E, a.stats.N) == (a.E, a.N)
    for t in (a, b):
        for _ in range(8):
            t.step(update=True)
    _same(_snapshot(a), _snapshot(b))
    tot = a.finish()
    assert tot["steps"] + int(a.stats.run_len.sum()) == 8 * a.E       # every env step counted once
    assert tot["episodes"] == int(a.stats.ep_count.sum())


@pytest.mark.parametrize("model", MODELS)
def test_eager_graph_and_resume_agree(native_lib, monkeypatch, tmp_path, model):
    from multi_agent_aac_amd import trainer
    monkeypatch.setattr(trainer, "STEP_GRAPH", True)
    monkeypatch.setattr(trainer, "STEP_GRAPH_GRU", True)
    a = _trainer(model, stats=True)
    for _ in range(5):
        a.step(update=True)
    path = str(tmp_path / f"{model}.ckpt")
    a.save_checkpoint(path)
    mid = a.stats.read()
    for _ in range(6):
        a.step(update=True)
    want, want_raw, snap = a.finish(), _stats_raw(a), _snapshot(a)
    assert want["steps"] + int(a.stats.run_len.sum()) == 11 * a.E
    # whole-step graphs from the same checkpoint: one step per replay, then two per replay (the fresh
    # loops below take steps of their own first, so the load has something to overwrite)
    g = _trainer(model, stats=True)
    for _ in range(2):
        g.step(update=True)
    g.load_checkpoint(path)
    np.testing.assert_equal(g.stats.read(), mid)      # (nan fields compare equal)
    g.step_graph()
    g.step_graph()
    g.step_graph_pair()
    g.step_graph_pair()
    np.testing.assert_equal(g.finish(), want)
    _same(_stats_raw(g), want_raw)
    _same(_snapshot(g), snap)
    # a resumed eager run
    r = _trainer(model, stats=True)
    for _ in range(3):
        r.step(update=False)
    r.load_checkpoint(path)
    for _ in range(6):
        r.step(update=True)
    np.testing.assert_equal(r.finish(), want)
    _same(_stats_raw(r), want_raw)


def test_checkpoint_without_stats_is_refused(native_lib, tmp_path):
    """A file saved by a trainer without statistics names the missing tensor and changes nothing."""
    a, b = _trainer("att", stats=False), _trainer("att", stats=True)
    for t in (a, b):
        t.step(update=True)
    path = str(tmp_path / "plain.ckpt")
    a.save_checkpoint(path)
    before, raw = _snapshot(b), _stats_raw(b)
    with pytest.raises(KeyError, match="stats.run_return"):
        b.load_checkpoint(path)
    _same(_snapshot(b), before)
    _same(_stats_raw(b), raw)
    # the other direction loads: the plain trainer asks for no stats tensor
    b.save_checkpoint(path)
    a.load_checkpoint(path)
