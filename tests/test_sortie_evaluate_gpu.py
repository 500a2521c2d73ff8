"""Sortie statistics in the evaluator (``Evaluator(..., sorties=True)``) for the ATT, GRU and UAM trainers
at E = 16: the split launch sequence the ATT / GRU rollouts take with sorties on gives the same
``EpisodeStats`` as the fused tail; the sortie totals agree with the episode tallies over the same episode
set; every logged sortie's flown length equals the one recomputed on the host from the flight recorder's
positions, bit for bit; graph and NO_GRAPH rollouts agree bit for bit."""
import math

import numpy as np
import pytest
import torch

import sortie_ref

pytestmark = pytest.mark.gpu

MODELS = ["att", "gru", "uam"]
E_EVAL, K = 16, 2


def _trainer(model, seed=1):
    from multi_agent_aac_amd import trainer
    if model == "uam":
        tr = trainer.UamTrainer(8, 5, 8, 4096, seed=seed)
    else:
        tr = trainer.Trainer(64, 3, 32, 4096, "combined", seed=seed, model=model)
    for _ in range(3):
        tr.step(update=True)
    return tr


def _same_stats(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, float) and math.isnan(x):
            assert isinstance(y, float) and math.isnan(y), k
        else:
            assert x == y, (k, x, y)


def _raw(ss):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in ss.tensors().items()}


@pytest.mark.parametrize("model", MODELS)
def test_sorties_count_the_evaluated_episode_set(native_lib, model):
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = _trainer(model)
    plain = Evaluator(tr, E=E_EVAL)
    assert plain.sorties is None
    want = plain.evaluate(K)
    ev = Evaluator(tr, E=E_EVAL, sorties=dict(log=4096))
    st = ev.evaluate(K)
    _same_stats(st, want)           # the split sequence equals the fused tail; the return value is unchanged
    so = ev.sorties.read()
    rows = ev.sorties.log_rows()
    print(model, {k: so[k] for k in sortie_ref.COUNTERS}, "ratio", so["ratio_mean"], so["ratio_std"])
    assert st["episodes"] == E_EVAL * K == so["episodes"]
    assert so["sorties"] == ev.N * st["episodes"] == len(rows) == sum(so[k] for k in sortie_ref.CLASSES)
    # an aircraft whose goal bit was ever set: the episode tallies' reach count
    assert int((rows["reach_step"] > 0).sum()) == sum(k * n for k, n in enumerate(st["reach_hist"]))
    assert so["reached"] == sum(k * n for k, n in enumerate(st["reach_hist"]))
    assert int(so["collide_hist"].sum()) == st["collision_count"]
    assert ev.sorties.reach_margin == (5.0 if model == "uam" else 0.0)
    assert np.array_equal(ev.sorties.ep_count.cpu().numpy(), ev.stats.ep_count.cpu().numpy())
    # a second call replays the same episode set into an emptied accumulator
    first = _raw(ev.sorties)
    _same_stats(ev.evaluate(K), want)
    again = _raw(ev.sorties)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    # keywords reach the accumulator
    assert Evaluator(tr, E=8, sorties=dict(reach_margin=1.5)).sorties.reach_margin == 1.5


@pytest.mark.parametrize("model", MODELS)
def test_logged_flown_equals_the_recorded_path(native_lib, model):
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = _trainer(model)
    ev = Evaluator(tr, E=E_EVAL, sorties=dict(log=4096))
    out = ev.record(K)
    assert len(out) == 2            # (stats, Trajectories): unchanged
    st, traj = out
    rows = ev.sorties.log_rows()
    assert len(rows) == ev.N * st["episodes"]
    eps = {(ep["env"], ep["episode"]): ep for ep in traj.episodes()}
    assert len(eps) == st["episodes"]
    margin, checked = ev.sorties.reach_margin, 0
    for r in rows:
        ep = eps[(int(r["env"]), int(r["episode"]))]
        assert not ep["truncated"] and ep["len"] == r["len"]
        p = ep["pos"][:, int(r["agent"])]          # the reset row (the start), then one row per step
        dist = 0.0
        for k in range(2, len(p)):
            dist = dist + sortie_ref.norm(float(p[k][0]) - float(p[k - 1][0]), float(p[k][1]) - float(p[k - 1][1]))
        first = sortie_ref.norm(float(p[1][0]) - float(p[0][0]), float(p[1][1]) - float(p[0][1]))
        flown = (dist + first) + margin
        assert flown.hex() == float(r["flown"]).hex(), (r, flown)
        g = ep["goal"][0, int(r["agent"])]
        straight = sortie_ref.norm(float(g[0]) - float(p[0][0]), float(g[1]) - float(p[0][1]))
        assert straight.hex() == float(r["straight"]).hex(), (r, straight)
        m = np.bitwise_or.reduce(ep["mask"][1:, int(r["agent"])])
        bits = sortie_ref.BITS_UAM if model == "uam" else sortie_ref.BITS_ENV
        assert sortie_ref.classify(int(m), bits["bound_bit"], bits["obstacle_bit"], bits["drone_bit"],
                                   bits["goal_bit"]) == r["cls"]
        checked += 1
    assert checked == len(rows) > 0
    so = ev.sorties.read()
    assert so["sorties"] == len(rows) and int(so["collide_hist"].sum()) == st["collision_count"]


@pytest.mark.parametrize("model", MODELS)
def test_graph_and_eager_rollouts_agree(native_lib, monkeypatch, model):
    from multi_agent_aac_amd import trainer
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = _trainer(model)
    ev = Evaluator(tr, E=E_EVAL, sorties=dict(log=4096))
    st = ev.evaluate(K)
    want, so = _raw(ev.sorties), ev.sorties.read()
    monkeypatch.setattr(trainer, "NO_GRAPH", True)
    eager = Evaluator(tr, E=E_EVAL, sorties=dict(log=4096))
    _same_stats(eager.evaluate(K), st)
    got, so2 = _raw(eager.sorties), eager.sorties.read()
    for k in want:
        assert want[k].tobytes() == got[k].tobytes(), k
    for k in so:
        assert np.array_equal(so[k], so2[k], equal_nan=True), k
    assert so["sorties"] == ev.N * E_EVAL * K
