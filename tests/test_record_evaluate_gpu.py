"""``Evaluator.record`` for the three models, 32 eval envs: the recorded rollout (the split launch
sequence from its own pair of graphs) covers exactly the episode set of ``evaluate`` -- equal
statistics before and after each other, the statistics log's 64 episodes equal to the recorder's
summaries per (env, episode order) bit for bit --, repeats itself, leaves the trainer alone, gives
well-formed episodes, and a subset of tracks records what the same envs gave among all of them."""
import numpy as np
import pytest

import record_ref
from test_evaluate_gpu import E_EVAL, _warm
from test_stats_trainer_gpu import _same, _snapshot, _trainer

pytestmark = pytest.mark.gpu

SUBSET = [31, 0, 7]


def _same_episode(a, b):
    assert set(a) == set(b)
    for k in a:
        if k != "track":
            assert record_ref.same_bits(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("model", ["att", "gru", "uam"])
def test_record_covers_the_evaluated_episodes(native_lib, model):
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = _warm(_trainer(model, stats=False))
    before = _snapshot(tr)
    ev = Evaluator(tr, E=E_EVAL, seed=0, log=2 * E_EVAL)
    want = ev.evaluate(2)
    assert ev._rec is None and ev._rec_graphs is None        # an evaluator that never recorded
    assert want["episodes"] == 2 * E_EVAL
    stats, tj = ev.record(2)
    np.testing.assert_equal(stats, want)
    # the statistics log of that rollout: per env, its episodes in order
    log = ev.stats.log_rows()
    assert len(log) == 2 * E_EVAL
    assert list(tj.tracks) == list(range(E_EVAL)) and (tj.ep_seen == 2).all() and not tj.dropped.any()
    for e in range(E_EVAL):
        mine = log[log["env"] == e]
        eps = tj.episodes(track=e)
        assert len(mine) == len(eps) == 2
        for row, ep in zip(mine, eps):
            assert ep["env"] == e and int(row["len"]) == ep["len"]
            assert np.float64(row["ret"]).tobytes() == np.float64(ep["ret"]).tobytes(), (e, row["ret"], ep["ret"])
    np.testing.assert_equal(ev.evaluate(2), want)            # and evaluate after record
    stats2, tj2 = ev.record(2)
    np.testing.assert_equal(stats2, want)
    assert tj2 == tj
    _same(_snapshot(tr), before)
    eps = tj.episodes()
    assert len(eps) == 2 * E_EVAL
    for ep in eps:
        assert not ep["truncated"] and ep["rows"] == ep["len"] + 1 <= ev.episode_length + 2
        assert ep["t"][0] == 0 and ep["row_flags"][0] == 2           # a reset row first
        assert ep["row_flags"][-1] == 1 and not ep["row_flags"][1:-1].any()      # env_done on the last row only
        assert list(ep["t"]) == list(range(ep["rows"]))
        assert ep["min_sep"] == ep["min_sep_row"].min() and ep["min_sep_t"] == int(np.argmin(ep["min_sep_row"]))
        assert ep["any_done"] == bool(ep["done"].any())
    assert [ep["episode"] for ep in tj.episodes(track=5)] == [1, 2]
    ms = tj.min_separation()
    print(model, "return_mean", want["return_mean"], "closest approach: min", ms.min(), "median", np.median(ms))
    # a subset of tracks, in another order
    stats3, sub = ev.record(2, env_ids=SUBSET)
    np.testing.assert_equal(stats3, want)
    assert list(sub.tracks) == SUBSET
    for k, e in enumerate(SUBSET):
        a, b = sub.episodes(track=k), tj.episodes(track=e)
        assert len(a) == len(b) == 2
        for x, y in zip(a, b):
            _same_episode(x, y)
    _same(_snapshot(tr), before)
