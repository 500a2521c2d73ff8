"""Noise-free evaluation rollouts (multi_agent_aac_amd/evaluate.py) for the three models, 32 eval
envs: ``evaluate(2)`` against a slow loop written here (act without noise, env.step, host tallies by
tests/stats_ref.py, auto_reset) on a second env built the same way; repeatability; and the trainer --
learner, noise counter, replay, env, captured whole-step graphs -- left exactly as it was."""
import numpy as np
import pytest
import torch

import stats_ref
from test_stats_trainer_gpu import _same, _snapshot, _trainer

pytestmark = pytest.mark.gpu

E_EVAL = 32


def _warm(tr):
    for _ in range(4):
        tr.step(update=True)
    return tr


def _slow_loop(tr, model, k):
    """k episodes per eval env, one launch and one download at a time."""
    from multi_agent_aac_amd import gru
    from multi_agent_aac_amd.evaluate import Evaluator
    ev = Evaluator(tr, E=E_EVAL, seed=0)          # only its env, buffers and episode counters are used
    env, N, m = ev.env, ev.N, tr.model
    ref = stats_ref.StatsRef(E_EVAL, N, ev.episode_length, ev.stats.goal_bit, ev.stats.return_mode)
    quota = np.full(E_EVAL, k, dtype=np.int32)
    ev._start()
    # GRU hidden states: a fixed ping-pong pair, so the learner builds two act plans and no more
    hp = [torch.zeros(E_EVAL, N, 64, device="cuda") for _ in range(2)]
    for s in range(k * (ev.episode_length + 1)):
        c, n = ev.bufs[s & 1], ev.bufs[1 - (s & 1)]
        if model == "uam":
            act = m.act(c.own, c.radar, ev.episode, noisy=False)
        elif model == "gru":
            act, h = m.act(c.own, c.radar, hp[s & 1], ev.episode, noisy=False, h_out=hp[1 - (s & 1)])
        else:
            act = m.act(c.own, c.radar, c.nei, ev.episode, noisy=False)
        env.step(act, out=n)
        ref.accumulate(*[getattr(n, f).cpu().numpy() for f in ("reward", "done", "mask", "env_done", "bbc")],
                       quota=quota)
        if model == "gru":
            gru.reset_hidden(h, n.env_done)
        env.auto_reset(n.env_done, out=n)
        if ref.under_quota == 0:
            break
    return ref


@pytest.mark.parametrize("model", ["att", "gru", "uam"])
def test_evaluate_matches_slow_loop_and_leaves_trainer_alone(native_lib, model):
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = _warm(_trainer(model, stats=False))
    before = _snapshot(tr)
    ev = Evaluator(tr, E=E_EVAL, seed=0)
    got = ev.evaluate(2)
    assert got["episodes"] == 2 * E_EVAL and got["under_quota"] == 0
    assert (ev.stats.ep_count == 2).all()
    again = ev.evaluate(2)
    np.testing.assert_equal(again, got)           # the same episode set every call
    _same(_snapshot(tr), before)
    ref = _slow_loop(tr, model, 2)
    print(model, {k: got[k] for k in stats_ref.COUNTERS}, got["reach_hist"], got["return_mean"])
    stats_ref.check_totals(got, ref)
    _same(_snapshot(tr), before)
    one = ev.evaluate(1)                          # another quota: the first episode of every env
    assert one["episodes"] == E_EVAL


@pytest.mark.parametrize("model", ["att", "gru", "uam"])
def test_training_continues_as_if_never_evaluated(native_lib, monkeypatch, model):
    """A whole-step graph captured before ``evaluate`` still replays afterwards, and the next steps are
    bit-equal to a run that never evaluated."""
    from multi_agent_aac_amd import trainer
    from multi_agent_aac_amd.evaluate import Evaluator
    monkeypatch.setattr(trainer, "STEP_GRAPH", True)
    monkeypatch.setattr(trainer, "STEP_GRAPH_GRU", True)
    a, b = _warm(_trainer(model, stats=True)), _warm(_trainer(model, stats=True))
    for t in (a, b):
        t.step_graph()
        t.step_graph()
    graphs = dict(a._sg)
    Evaluator(a, E=E_EVAL, seed=0).evaluate(1)
    for t in (a, b):
        for _ in range(4):
            t.step_graph()
    assert a._sg == graphs                        # not re-captured
    _same(_snapshot(a), _snapshot(b))
    np.testing.assert_equal(a.finish(), b.finish())
