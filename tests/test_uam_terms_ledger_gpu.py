"""``RewardLedger.for_uam(BatchedUAM)`` on a rollout: E = 300, N = 5 (two ledger slots, the second ragged),
40 steps of steered actions with auto-reset and a quota.  Totals and running state are the numpy fold
(tests/terms_ref.LedgerRef) of the downloaded rows bit for bit, and every finished episode's terms add up
to the statistics' return within the reordering bound of a double sum, n * 2^-52 * sum |addend| with n
the number of (non-zero) addends."""
import numpy as np
import pytest
import torch

from tests import uam_terms_ref as R

pytestmark = pytest.mark.gpu


def test_uam_ledger_against_fold_and_episode_stats(native_lib):
    from multi_agent_aac_amd import uam
    from multi_agent_aac_amd.stats import EpisodeStats
    from multi_agent_aac_amd.terms import RewardLedger
    E, N, T, QUOTA = 300, 5, 40, 2
    env = uam.BatchedUAM(E, N, episode_length=12)
    env.set_bank(uam.build_bank(1024, N, seed=3), seed=9)
    stats = EpisodeStats.for_env(env, log=4096)
    assert env.terms is None
    led = RewardLedger.for_uam(env)
    assert env.terms is not None and tuple(env.terms.shape) == (E, N, 12) and led.slots.shape[0] == 2
    ref = R.LedgerRef(E, N)
    quota = np.full(E, QUOTA, np.int32)
    q_dev = torch.from_numpy(quota).cuda()
    b = env.bufs
    env.auto_reset(None)
    rng = np.random.default_rng(7)
    run_t, run_abs, run_n = np.zeros(E), np.zeros(E), np.zeros(E)
    count = np.zeros(E, int)
    eps = []                     # (env, sum of the terms, bound) in (step, env) order
    for s in range(T):
        st = env.get_state()
        d = (st["goal"] - st["pos"]).cpu().numpy()
        act = np.clip(d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9) + rng.normal(0, 0.7, d.shape),
                      -1, 1)
        env.step(torch.from_numpy(act).cuda())
        stats.accumulate(b, quota=q_dev)
        led.accumulate(b, quota=q_dev)
        terms, done = env.terms.cpu().numpy(), b.env_done.cpu().numpy()
        assert np.array_equal(R.slot_sum(terms), b.reward.cpu().numpy())
        ref.accumulate(terms, done, quota)
        c = terms[:, :, :R.SLOTS]
        run_t += c.sum(axis=(1, 2))
        run_abs += np.abs(c).sum(axis=(1, 2))
        run_n += (c != 0).sum(axis=(1, 2))
        for e in np.flatnonzero(done):
            if count[e] < QUOTA:
                eps.append((int(e), run_t[e], run_n[e] * 2.0 ** -52 * run_abs[e]))
                count[e] += 1
            run_t[e] = run_abs[e] = run_n[e] = 0.0
        env.auto_reset(b.env_done)
    rows = stats.log_rows()
    assert len(rows) == len(eps) >= E
    assert count.max() == QUOTA            # the quota bit: some env finished more than it may count
    worst = max(abs(tot - float(row["ret"])) / bound for row, (e, tot, bound) in zip(rows, eps) if bound > 0)
    print(f"uam: {len(eps)} episodes, largest |sum of terms - return| / bound = {worst:.3f}")
    for row, (e, tot, bound) in zip(rows, eps):
        assert int(row["env"]) == e
        assert abs(tot - float(row["ret"])) <= bound, (e, tot, float(row["ret"]), bound)
    n, sm, sq, lo, hi = ref.reduce()
    raw = led.raw()
    d = raw.view(np.float64)
    assert int(raw[0]) == n == len(eps) == stats.read()["episodes"]
    for name, got, want in (("sum", d[1:9], sm), ("sqsum", d[9:17], sq), ("min", d[17:25], lo), ("max", d[25:33], hi)):
        assert got.tobytes() == np.asarray(want, np.float64).tobytes(), (name, got, want)
    assert led.run.cpu().numpy().tobytes() == ref.run.tobytes()
    assert np.array_equal(led.ep_count.cpu().numpy(), ref.ep_count)
    out = led.read()
    for k in ("event", "progress", "building", "drone"):
        assert out["terms"][k]["min"] != out["terms"][k]["max"], k
    for k in ("waypoint", "path", "speed", "reserved"):
        assert out["terms"][k]["min"] == out["terms"][k]["max"] == 0.0, k


def test_for_uam_takes_the_uam_env_only(native_lib, occ):
    """``for_env`` stays the ``BatchedEnv`` entry (tests/test_terms_ledger_gpu.py holds its refusal of a
    ``BatchedUAM``); ``for_uam`` refuses the other envs."""
    from multi_agent_aac_amd.env import BatchedEnv
    from multi_agent_aac_amd.mpe import BatchedSpread
    from multi_agent_aac_amd.terms import RewardLedger
    for env in (BatchedEnv(4, 3, occ), BatchedSpread(4, 3)):
        with pytest.raises(NotImplementedError, match="BatchedUAM"):
            RewardLedger.for_uam(env)
    with pytest.raises(NotImplementedError, match="MPE"):
        RewardLedger.for_env(BatchedSpread(4, 3))

