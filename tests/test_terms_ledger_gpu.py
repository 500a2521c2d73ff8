"""The reward ledger's kernels (aac_terms_accumulate / aac_terms_reduce, csrc/aac_terms.hip) against the
numpy fold of tests/terms_ref.py on synthetic terms, env_done and quota sequences -- counts exact, sums
bit-equal (the fixed tree), twice and eager against a captured graph -- and, on a real rollout, against
the episode statistics."""
import types

import numpy as np
import pytest
import torch

from tests import terms_ref as R

pytestmark = pytest.mark.gpu
STEPS = 6


class _Env:
    """What RewardLedger reads of an env: E, N, device and the attached terms buffer."""

    def __init__(self, E, N):
        self.E, self.N, self.device = E, N, torch.device("cuda", torch.cuda.current_device())
        self.terms = torch.zeros(E, N, R.WIDTH, dtype=torch.float64, device=self.device)


def _sequence(E, N, seed):
    rng = np.random.default_rng(seed)
    terms = rng.normal(size=(STEPS, E, N, R.WIDTH)) * rng.choice([1e-3, 1.0, 1e3], size=(STEPS, E, N, 1))
    done = (rng.random((STEPS, E)) < 0.4).astype(np.uint8)
    done[-1, : max(1, E // 2)] = 1
    quota = rng.integers(1, 4, size=E).astype(np.int32)
    return terms, done, quota


def _device(E, N, terms, done, quota, graph=False):
    from multi_agent_aac_amd.terms import RewardLedger
    env = _Env(E, N)
    led = RewardLedger(env)
    bufs = types.SimpleNamespace(env_done=torch.zeros(E, dtype=torch.uint8, device=env.device))
    q = None if quota is None else torch.from_numpy(quota).cuda()
    t_dev, d_dev = torch.from_numpy(terms).cuda(), torch.from_numpy(done).cuda()
    g = None
    if graph:
        led.accumulate(bufs, quota=q)           # argument struct built outside the capture
        torch.cuda.synchronize()
        led.reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            led.accumulate(bufs, quota=q)
    for s in range(STEPS):
        env.terms.copy_(t_dev[s])
        bufs.env_done.copy_(d_dev[s])
        if g is not None:
            g.replay()
        else:
            led.accumulate(bufs, quota=q)
    raw = led.raw().copy()
    return raw, led.ep_count.cpu().numpy(), led.run.cpu().numpy(), led


@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("E", [1, 255, 256, 257, 600])
def test_ledger_against_numpy_fold(native_lib, E, N):
    terms, done, quota = _sequence(E, N, 1000 * E + N)
    for use_quota in (False, True):
        q = quota if use_quota else None
        ref = R.LedgerRef(E, N)
        for s in range(STEPS):
            ref.accumulate(terms[s], done[s], q)
        n, sm, sq, lo, hi = ref.reduce()
        raw, epc, run, led = _device(E, N, terms, done, q)
        d = raw.view(np.float64)
        assert int(raw[0]) == n and n > 0
        assert np.array_equal(epc, ref.ep_count)
        for name, got, want in (("sum", d[1:9], sm), ("sqsum", d[9:17], sq), ("min", d[17:25], lo), ("max", d[25:33], hi)):
            assert got.tobytes() == np.asarray(want, np.float64).tobytes(), (name, got, want)
        assert run.tobytes() == ref.run.tobytes()
        # again, and from a captured graph: bit-identical totals
        raw2 = _device(E, N, terms, done, q)[0]
        raw3 = _device(E, N, terms, done, q, graph=True)[0]
        assert raw.tobytes() == raw2.tobytes() == raw3.tobytes()
    out = led.read(clear=True)
    assert out["episodes"] == n and set(out["terms"]) == set(R.NAMES[:R.SLOTS])
    assert abs(sum(v["share"] for v in out["terms"].values()) - 1.0) < 1e-9
    assert led.read()["episodes"] == 0 and np.array_equal(led.ep_count.cpu().numpy(), ref.ep_count)


def test_ledger_refuses_other_envs(native_lib):
    from multi_agent_aac_amd.terms import RewardLedger, names
    from multi_agent_aac_amd.uam import BatchedUAM
    assert names() == R.NAMES
    with pytest.raises(NotImplementedError, match="UAM"):
        RewardLedger.for_env(BatchedUAM(4, 3))


@pytest.mark.parametrize("variant", ["att", "wgru"])
def test_ledger_against_episode_stats_on_a_rollout(native_lib, occ, variant):
    """40 steps of random actions with auto-reset, E = 96.  Per finished episode the ledger's terms add up
    to the statistics' return within the float32 rounding of the stored rewards, sum over the episode's
    steps and agents of |reward| * 2^-24 (computed from the run's own rewards); the device totals are the
    numpy fold of the downloaded terms, bit for bit."""
    from multi_agent_aac_amd import world
    from multi_agent_aac_amd.env import BatchedEnv
    from multi_agent_aac_amd.stats import EpisodeStats
    from multi_agent_aac_amd.terms import RewardLedger
    E, N, T = 96, 3, 40
    env = BatchedEnv(E, N, occ, max_wp=32, variant=variant, episode_length=15)
    env.set_od_bank(world.ODBank(occ, n_pairs=1024, seed=3, max_wp=32), seed=9)
    stats = EpisodeStats.for_env(env, log=4096)
    led = RewardLedger.for_env(env)
    ref = R.LedgerRef(E, N)
    b = env.bufs
    env.auto_reset(None, out=b)
    rng = np.random.default_rng(7)
    run_t, run_abs = np.zeros(E), np.zeros(E)
    eps = []                     # (env, sum of the terms, bound) in (step, env) order
    for s in range(T):
        act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)).cuda()
        env.step(act, out=b)
        stats.accumulate(b)
        led.accumulate(b)
        terms, rew, done = env.terms.cpu().numpy(), b.reward.cpu().numpy().astype(np.float64), b.env_done.cpu().numpy()
        ref.accumulate(terms, done)
        run_t += terms[:, :, :R.SLOTS].sum(axis=(1, 2))
        run_abs += np.abs(rew).sum(axis=1)
        for e in np.flatnonzero(done):
            eps.append((int(e), run_t[e], run_abs[e] * 2.0 ** -24))
            run_t[e] = run_abs[e] = 0.0
        env.auto_reset(b.env_done, out=b)
    rows = stats.log_rows()
    assert len(rows) == len(eps) >= E
    worst = max(abs(tot - float(row["ret"])) / bound for row, (e, tot, bound) in zip(rows, eps) if bound > 0)
    print(f"{variant}: {len(eps)} episodes, largest |sum of terms - return| / bound = {worst:.3f}")
    for row, (e, tot, bound) in zip(rows, eps):
        assert int(row["env"]) == e
        assert abs(tot - float(row["ret"])) <= bound, (e, tot, float(row["ret"]), bound)
    n, sm, sq, lo, hi = ref.reduce()
    raw = led.raw()
    assert int(raw[0]) == n == len(eps) == stats.read()["episodes"]
    assert raw.view(np.float64)[1:9].tobytes() == sm.tobytes()
    out = led.read()
    assert abs(out["return_mean"] - stats.read()["return_mean"]) <= sum(x[2] for x in eps) / n + 1e-9
