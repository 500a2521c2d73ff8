"""The UAM step kernel's reward terms (aac_uam_set_terms_buffer, include/aac_terms.h).

  * the left-to-right sum of every row's slots 0..6 equals the stored reward with ``==``, on the
    exact-threshold batches at N = 3, 5, 16 (the 16-lane ballot rows) and N = 17 (the sequential per-env
    walk), with more than 16 envs per workgroup (N = 2, 3 at E = 44) and on a 40-step free run with
    auto-reset, where a reset never changes a row;
  * every slot against tests/uam_terms_ref.py from the identical injected pre-step state: slots 0-4 and
    6-10 within 1e-12, slots 5 and 11 within 1e-9 (the UAM radar bar: the two sides locate ray hits by
    different formulas);
  * with no buffer, with one attached and with one attached then detached the outputs and the state are
    bit-equal."""
import functools

import numpy as np
import pytest
import torch

from tests import uam_terms_ref as R
from tests import uam_thresholds as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT, RADAR = 1e-12, 1e-9
RADAR_SLOTS = (5, 11)


def _np_state(env):
    return {k: v.cpu().numpy() for k, v in env.get_state().items()}


def _nan_terms(env):
    """A terms buffer full of NaN: a slot the step leaves unwritten shows."""
    return env.use_terms_buffer(torch.full((env.E, env.N, 12), float("nan"), dtype=torch.float64, device=DEV))


@functools.lru_cache(maxsize=None)
def _threshold_step(N):
    """One zero-action step of the threshold batch with a terms buffer: (batch, pre-step state, reward,
    mask, radar, terms)."""
    from multi_agent_aac_amd import uam
    B = T.build(N)
    st = B.state()
    E = len(B)
    env = uam.BatchedUAM(E, N)
    env.reset(st["pos"], st["goal"], st["cloud_kind"])
    env.set_state(**st)
    pre = _np_state(env)
    terms = _nan_terms(env)
    env.step(torch.zeros(E, N, 2, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    b = env.bufs
    return B, pre, b.reward.cpu().numpy(), b.mask.cpu().numpy(), b.radar.cpu().numpy(), terms.cpu().numpy()


def _kinds(mask):
    """The reward branch of every aircraft from its mask: 0 bound, 1 cloud, 2 drone, 3 goal, 4 normal."""
    k = np.full(mask.shape, 4)
    k[(mask & 16) != 0] = 3
    k[(mask & 4) != 0] = 2
    k[(mask & 2) != 0] = 1
    k[(mask & 1) != 0] = 0
    return k


def _check_rows(terms, reward, mask, radar=None):
    """What holds for every row with no reference: the sum identity, the branch's slots, the gauges."""
    assert not np.isnan(terms).any(), np.argwhere(np.isnan(terms))[:5]
    assert np.array_equal(R.slot_sum(terms), reward)
    k = _kinds(mask)
    crash = k < 3
    assert (terms[..., 0][crash] <= -50.0).all() and (terms[..., 0][k == 3] == 50.0).all()
    assert (terms[..., 0][k == 4] == 0.0).all()
    assert (terms[..., (1, 2, 4, 7)] == 0.0).all()
    assert (terms[..., (3, 5, 6)][k != 4] == 0.0).all()
    assert (terms[..., 8:] >= 0.0).all()
    if radar is not None:
        assert np.array_equal(terms[..., 11], radar.min(axis=-1))
    return k


@pytest.mark.parametrize("N", [3, 5, 16, 17])
def test_sum_identity_on_thresholds(native_lib, N):
    B, pre, reward, mask, radar, terms = _threshold_step(N)
    k = _check_rows(terms, reward, mask, radar)
    assert set(np.unique(k)) == {0, 1, 2, 3, 4}
    assert (reward == -100.0).any()          # the crash doubling


def test_n17_sequential_walk_against_oracle(native_lib):
    """N > 16 takes the per-env walk of phase 6: reward against the oracle and the rows against the
    restatement, one env per family."""
    N = 17
    B, pre, reward, mask, radar, terms = _threshold_step(N)
    picks = T.one_per_family(B)
    ref = R.batch_terms(pre, N, picks)
    for e in picks:
        t, r, _ = ref[e]
        tag = (B.fam[e], B.var[e], e)
        np.testing.assert_allclose(reward[e], r, rtol=0, atol=RADAR, err_msg=str(tag))
        _cmp_terms(terms[e], t, tag)


def _cmp_terms(got, want, tag):
    for s in range(R.WIDTH):
        np.testing.assert_allclose(got[:, s], want[:, s], rtol=0, atol=RADAR if s in RADAR_SLOTS else TIGHT,
                                   err_msg=f"{tag} slot {s} ({R.NAMES[s]})")


@pytest.mark.parametrize("N", [3, 5, 16])
def test_values_against_restatement(native_lib, N):
    B, pre, reward, mask, radar, terms = _threshold_step(N)
    envs = list(range(len(B))) if N < 16 else T.one_per_family(B)
    ref = R.batch_terms(pre, N, envs)
    used = np.zeros(R.WIDTH, bool)
    band_dbl = crash_dbl = 0
    for e in envs:
        t, r, ev = ref[e]
        _cmp_terms(terms[e], t, (B.fam[e], B.var[e], e))
        used |= (terms[e] != 0).any(axis=0)
        # a doubling that shows in the row itself: the normal-branch aircraft whose own bearing doubled
        # the coefficient, the collided aircraft whose own bearing doubled the crash penalty
        band_dbl += sum(1 for i in range(N) if ev["band_dbl"][i] and t[i, 6] != 0)
        crash_dbl += sum(1 for i in range(N) if ev["crash_dbl"][i] and t[i, 0] <= -100.0)
    if N < 16:
        assert set(np.flatnonzero(used)) == set(R.USED), np.flatnonzero(used)
        assert band_dbl > 0 and crash_dbl > 0, (band_dbl, crash_dbl)
        assert (terms[..., 0] == -100.0).any()


@pytest.mark.parametrize("N", [2, 3])
def test_more_than_16_envs_per_workgroup(native_lib, N):
    """floor(64 / N) > 16 envs per workgroup: the ballot rows take them 16 at a time, and the envs past
    the 16th get their rows like the others (a buffer of NaN shows a row that is left alone)."""
    from multi_agent_aac_amd import uam
    E = 44
    env = uam.BatchedUAM(E, N)
    env.set_bank(uam.build_bank(256, N, seed=40 + N), seed=2)
    env.auto_reset()
    rng = np.random.default_rng(N)
    for k in range(2):
        terms = _nan_terms(env)
        env.step(torch.from_numpy(rng.uniform(-1, 1, (E, N, 2))).to(DEV))
        torch.cuda.synchronize()
        b = env.bufs
        _check_rows(terms.cpu().numpy(), b.reward.cpu().numpy(), b.mask.cpu().numpy(), b.radar.cpu().numpy())


def test_free_run_with_auto_reset(native_lib):
    """40 steps at E = 2048, N = 8 with the steering of test_uam_event_coverage: the identity on every
    step, all five branches, and rows that an auto-reset leaves as the terminal step wrote them."""
    from multi_agent_aac_amd import uam
    E, N = 2048, 8
    env = uam.BatchedUAM(E, N)
    env.set_bank(uam.build_bank(4096, N, seed=3), seed=5)
    env.auto_reset()
    terms = _nan_terms(env)
    rng = np.random.default_rng(0)
    seen = set()
    resets = 0
    for k in range(40):
        pre = _np_state(env)
        d = pre["goal"] - pre["pos"]
        act = np.clip(d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9) + rng.normal(0, 0.7, d.shape),
                      -1, 1)
        out = np.where(pre["start"][..., :1] < 20, -1.0, 1.0)
        act[::4] = np.concatenate([out, np.zeros_like(out)], -1)[::4]
        env.step(torch.from_numpy(act).to(DEV))
        b = env.bufs
        t = terms.clone()
        kinds = _check_rows(t.cpu().numpy(), b.reward.cpu().numpy(), b.mask.cpu().numpy(), b.radar.cpu().numpy())
        seen |= set(np.unique(kinds))
        resets += int(b.env_done.sum())
        env.auto_reset(b.env_done)
        assert torch.equal(terms, t)
    assert seen == {0, 1, 2, 3, 4}, seen
    assert resets > 0


def test_detached_is_the_plain_step(native_lib):
    """Three envs from one bank and one action sequence: no buffer, a buffer, a buffer for the first
    step only.  Outputs and state are bit-equal on every step; a detached buffer is written no more."""
    from multi_agent_aac_amd import uam
    E, N = 300, 5
    bank = uam.build_bank(512, N, seed=9)
    envs = []
    for _ in range(3):
        env = uam.BatchedUAM(E, N, p3=True, tdcpa=True)
        env.set_bank(bank, seed=77)
        env.auto_reset()
        envs.append(env)
    assert all(env.terms is None for env in envs)
    with pytest.raises(ValueError):
        envs[1].use_terms_buffer(torch.zeros(E, N, 12, dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        envs[1].use_terms_buffer(torch.zeros(E, N, 13, dtype=torch.float64, device=DEV)[..., :12])
    with pytest.raises(ValueError):
        envs[1].use_terms_buffer(torch.zeros(E, N, 12, dtype=torch.float64))
    assert envs[1].terms is None
    t1, t2 = _nan_terms(envs[1]), _nan_terms(envs[2])
    assert envs[1].terms is t1
    rng = np.random.default_rng(4)
    kept = None
    for k in range(4):
        act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 2))).to(DEV)
        for env in envs:
            env.step(act)
        if k == 0:
            assert torch.equal(t1, t2)
            assert envs[2].use_terms_buffer(detach=True) is None and envs[2].terms is None
            kept = t2.clone()
        b0, s0 = envs[0].bufs, envs[0].get_state()
        for env in envs[1:]:
            for f in b0.__dataclass_fields__:
                assert torch.equal(getattr(env.bufs, f), getattr(b0, f)), (k, f)
            for name, v in env.get_state().items():
                assert torch.equal(v, s0[name]), (k, name)
        assert np.array_equal(R.slot_sum(t1.cpu().numpy()), b0.reward.cpu().numpy())
        assert torch.equal(t2, kept)
        for env in envs:
            env.auto_reset(env.bufs.env_done)
