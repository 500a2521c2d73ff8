"""The gradient-clipping references agree with each other on the CPU: the float64 numpy restatement of
aac_clip_sumsq + aac_adam_flat_clip (tests/clip_ref.py) against torch's ``clip_grad_norm_`` + Adam
(``ClippedAdam``), the edge cases of the coefficient, the ``grad_clip`` argument's forms, and that the
bounds the learner tests derive give both outcomes (a clipped and an unclipped step) per network."""
import copy
import math

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import clip_ref

LR, EPS = 1e-3, 1e-8


def _torch_steps(p0, grads, max_norm):
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = clip_ref.ClippedAdam([p], max_norm, lr=LR, eps=EPS)
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    s = opt.state[p]
    return p.detach().numpy(), s["exp_avg"].numpy(), s["exp_avg_sq"].numpy(), opt.norms


def _np_steps(p0, grads, max_norm, order=0, gscale=1.0):
    p, m, v = np.array(p0, dtype=np.float64), np.zeros(len(p0)), np.zeros(len(p0))
    rec, norms, coefs = clip_ref.new_record(), [], []
    for t, g in enumerate(grads, 1):
        _, norm, coef, p, m, v = clip_ref.clip_adam(np.asarray(g, dtype=np.float64)[None], order, gscale, max_norm, p, m, v,
                                                    t, lr=LR, eps=EPS, record=rec)
        norms.append(norm)
        coefs.append(coef)
    return p, m, v, norms, coefs, rec


@pytest.mark.parametrize("n", [1, 7, 1000])
@pytest.mark.parametrize("max_norm", [0.05, 1.0, 1e3])
def test_restatement_matches_clipped_adam(n, max_norm):
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * s for s in (1.0, 0.01, 3.0)]
    want = _torch_steps(p0, grads, max_norm)
    got = _np_steps(p0, grads, max_norm)
    # 1e-12 relative to each vector's scale: exp_avg = b1 m + (1 - b1) g cancels in single elements, where
    # torch's lerp and the restatement's order differ by an ulp of the operands, not of the result
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * np.abs(b).max())
    np.testing.assert_allclose(got[3], want[3], rtol=1e-12, atol=0)


def test_copy_orders():
    """The two copy orders on float32 copies: the definitions, and the split of a sum across copies and
    gscale (what a world > 1 update does) leaves the norm of the mean."""
    rng = np.random.default_rng(3)
    c = rng.standard_normal((6, 50)).astype(np.float32)
    want0 = ((((c[0] + c[1]) + c[2]) + c[3]) + c[4]) + c[5]
    want1 = ((c[0] + c[4]) + (c[1] + c[5])) + (c[2] + c[3])
    assert np.array_equal(clip_ref.sum_copies(c, 0), want0) and np.array_equal(clip_ref.sum_copies(c, 1), want1)
    assert clip_ref.sum_copies(c, 1).dtype == np.float32
    z = np.zeros(50)
    one = clip_ref.clip_adam(c, 1, 1.0, 0.5, z, z, z, 1)
    two = clip_ref.clip_adam((2 * want1)[None], 0, 0.5, 0.5, z, z, z, 1)       # SUM over two equal ranks x 1 / 2
    assert one[1] == two[1] and one[2] == two[2] and np.array_equal(one[3], two[3])


def test_edge_cases():
    g = np.array([3.0, 4.0, 0.0])                   # norm exactly 5
    p0 = np.array([0.5, -1.0, 2.0])
    plain = _torch_steps(p0, [g], None)
    for max_norm, clipped in ((10.0, 0), (5.0, 1), (1.0, 1), (math.inf, 0)):      # below, equal, above, inf
        p, m, v, norms, coefs, rec = _np_steps(p0, [g], max_norm)
        want = _torch_steps(p0, [g], max_norm)
        np.testing.assert_allclose(p, want[0], rtol=1e-12, atol=0)
        assert norms == [5.0] and rec["clipped"] == clipped and rec["steps"] == 1 and rec["nonfinite"] == 0
        assert (coefs[0] < 1.0) == bool(clipped)
        if not clipped:
            assert coefs[0] == 1.0
            np.testing.assert_allclose(p, plain[0], rtol=1e-12, atol=0)
    assert _np_steps(p0, [g], 5.0)[4][0] == 5.0 / (5.0 + 1e-6)
    # a zero gradient: norm 0, coef = min(1, max_norm / 1e-6) = 1, nothing moves
    p, m, v, norms, coefs, rec = _np_steps(p0, [np.zeros(3)], 1.0)
    assert norms == [0.0] and coefs == [1.0] and rec["clipped"] == 0 and np.array_equal(p, p0)
    np.testing.assert_array_equal(p, _torch_steps(p0, [np.zeros(3)], 1.0)[0])
    # one NaN element: the norm, coef and every parameter go NaN, as in torch (error_if_nonfinite=False)
    bad = np.array([1.0, np.nan, 2.0])
    p, m, v, norms, coefs, rec = _np_steps(p0, [bad], 1.0)
    want = _torch_steps(p0, [bad], 1.0)
    assert np.isnan(p).all() and np.isnan(want[0]).all() and np.isnan(norms[0]) and np.isnan(coefs[0])
    assert rec["nonfinite"] == 1 and rec["clipped"] == 0 and rec["max_norm_seen"] == 0.0
    # an infinite element: coef 0, inf * 0 = NaN at that element only in the gradient; torch agrees
    inf = np.array([1.0, np.inf, 2.0])
    p, m, v, norms, coefs, rec = _np_steps(p0, [inf], 1.0)
    want = _torch_steps(p0, [inf], 1.0)
    assert np.array_equal(np.isnan(p), np.isnan(want[0])) and coefs == [0.0] and rec["nonfinite"] == 1
    assert rec["clipped"] == 1


def test_grad_clip_argument_forms():
    from multi_agent_aac_amd import clip
    assert clip.parse(None) is None and clip.parse((None, None)) is None
    assert clip.parse(1) == (1.0, 1.0) and clip.parse((5.0, None)) == (5.0, None)
    assert clip.parse([None, math.inf]) == (None, math.inf)
    for bad in (-1.0, math.nan, (1.0,), (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            clip.parse(bad)
    assert clip.partials(1) == 1 and clip.partials(clip.CHUNK) == 1 and clip.partials(clip.CHUNK + 1) == 2
    assert (clip.CHUNK, clip.THREADS, clip.FIELDS) == (clip_ref.CHUNK, clip_ref.THREADS, clip_ref.FIELDS)


def test_uam_learner_refuses():
    from multi_agent_aac_amd import uam_learner
    with pytest.raises(NotImplementedError, match="FusedUamUpdate"):
        uam_learner.MADDPG.set_grad_clip(None, 1.0)


def test_learner_bounds_give_both_outcomes():
    """At the learner test's shape (N = 3, B = 64, E = 32, three updates) on torch-seed-0 default weights:
    the bounds ``split_bounds`` derives from an unclipped reference run clip at least one and leave at
    least one step unclipped per network, and a scalar ``grad_clip=1.0`` would not (it clips every critic
    step and no actor step), which is why the learner tests use the derived pair."""
    N, B, E = 3, 64, 32
    D0 = 6 + 4 * (N - 1)
    torch.manual_seed(0)
    actor, critic = learner_ref.RefActor([D0, 18, 6], 2), learner_ref.RefCritic([D0, 18, 6], N, 2)
    _, host, idx = clip_ref.att_problem(N, B, E, 0, 3)
    _, _, free = clip_ref.att_ref_run(copy.deepcopy(actor), copy.deepcopy(critic), host, idx, None)
    assert len(free["critic"]) == len(free["actor"]) == 3 * N
    bounds = clip_ref.split_bounds(free)
    _, _, norms = clip_ref.att_ref_run(actor, critic, host, idx, bounds)
    for k, b in zip(("critic", "actor"), bounds):
        hit = [clip_ref.coef_of(x, b) < 1.0 for x in norms[k]]
        assert any(hit) and not all(hit), (k, b, norms[k])
    assert all(x > 1.0 for x in free["critic"]) and all(x < 1.0 for x in free["actor"]), free
