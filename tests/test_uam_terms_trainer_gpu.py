"""The reward ledger in the UAM loops: ``UamTrainer(terms=True)`` changes nothing it observes and gives
the same ledger from whole-step graph replays as from eager steps; ``Evaluator(uam_trainer, terms=True)``
holds exactly the statistics' episode set; ``record()`` returns the terms of every recorded step."""
import os

import numpy as np
import pytest
import torch

from tests import uam_terms_ref as R

pytestmark = pytest.mark.gpu
E, N, B = 64, 5, 64


def _trainer(terms, seed=1):
    from multi_agent_aac_amd import trainer
    return trainer.UamTrainer(E, N, B, 4096, seed=seed, terms=terms)


def _snapshot(tr):
    """Learner, replay ring, env state and the loop's rows (rewards among them)."""
    from multi_agent_aac_amd import checkpoint
    torch.cuda.synchronize()
    out = {"L." + k: v.clone() for k, v in checkpoint.learner_tensors(tr.model).items()}
    out.update({"R." + k: v.clone() for k, v in checkpoint.replay_tensors(tr.replay).items()})
    out.update({"E." + k: v.clone() for k, v in checkpoint.env_tensors(tr.env).items()})
    out.update({"X." + k: v.clone() for k, v in tr.checkpoint_parts()["extra"].items()})
    return out


def _same(a, b):
    assert set(a) == set(b)
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, bad


def test_terms_change_nothing_and_graph_equals_eager(native_lib):
    eager, graph, off = _trainer(True), _trainer(True), _trainer(False)
    assert off.ledger is None and off.env.terms is None and off.terms() is None
    assert eager.ledger is not None and eager.env.terms is not None
    for _ in range(6):
        eager.step(update=True)
        off.step(update=True)
    for _ in range(2):
        graph.step(update=True)
    for _ in range(4):
        graph.step_graph()
    torch.cuda.synchronize()
    _same(_snapshot(eager), _snapshot(off))          # rewards, ring rows, parameters, env state
    assert torch.equal(eager.cur.reward, off.cur.reward) and torch.equal(eager.cur.own, off.cur.own)
    assert eager.ledger.raw().tobytes() == graph.ledger.raw().tobytes()
    assert torch.equal(eager.ledger.run, graph.ledger.run) and bool((eager.ledger.run != 0).any())
    assert torch.equal(eager.ledger.ep_count, graph.ledger.ep_count)
    assert torch.equal(eager.env.terms, graph.env.terms)
    _same(_snapshot(eager), _snapshot(graph))
    assert np.array_equal(R.slot_sum(eager.env.terms.cpu().numpy()), eager.cur.reward.cpu().numpy())
    out = eager.terms()
    assert out["episodes"] == int(eager.ledger.ep_count.sum()) > 0
    assert eager.finish()["terms"]["episodes"] == out["episodes"] and off.finish() is None


def test_evaluator_ledger_and_recorded_terms(native_lib, tmp_path):
    from multi_agent_aac_amd.evaluate import Evaluator
    from multi_agent_aac_amd.record import Trajectories
    tr = _trainer(False)
    plain = Evaluator(tr, seed=3)
    ev = Evaluator(tr, seed=3, terms=True)
    assert tr.env.terms is None and plain.env.terms is None and ev.env.terms is not None
    base = plain.evaluate(1)
    stats, led = ev.evaluate(1)
    assert isinstance(base, dict) and stats == base        # the same rollout with the ledger on
    assert stats["episodes"] == E == led["episodes"]
    assert set(led["terms"]) == set(R.NAMES[:R.SLOTS])
    # float64 rewards: the two means differ by the order of the additions only
    assert abs(led["return_mean"] - stats["return_mean"]) <= 1e-9 * max(1.0, abs(stats["return_mean"]))
    stats2, traj, led2 = ev.record(1, env_ids=[0, 5, E - 1])
    assert stats2 == stats and led2 == led
    t = traj.terms
    assert t is not None and t.shape == (3, traj.S, N, R.WIDTH) and plain.record(1, env_ids=[0])[1].terms is None
    checked = 0
    for k in range(3):
        c = int(traj.cursor[k])
        assert c >= 2
        assert np.array_equal(R.slot_sum(t[k, :c]), traj.rows["reward"][k, :c]), k
        reset = (traj.rows["header"][k, :c, 2] & 2) != 0
        assert np.all(t[k, :c][reset] == 0) and np.any(t[k, :c][~reset][..., 9] != 0)
        checked += int((~reset).sum())
    assert checked >= 3
    p = os.path.join(str(tmp_path), "t.npz")
    traj.save(p)
    back = Trajectories.load(p)
    assert back == traj and np.array_equal(back.terms, t)
    back.rows["terms"] = t + 1.0
    assert not (back == traj)
