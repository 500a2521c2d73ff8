"""``env_simulator(reward_terms=True)``: ``ss_reward`` hands out the reference's per-step pieces
(``step_reward_record`` ATT/env:2590, ``eps_status_holder`` rows ATT/env:2596-2624) from the kernel's
reward terms; five steps against tests/terms_ref.py.  With the default flag the stub is unchanged."""
import json
import os

import numpy as np
import pytest

from tests import terms_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATOL = 1e-12


def _world(occ, **kw):
    from multi_agent_aac_amd.env import env_simulator
    fixed = json.load(open(os.path.join(GOLDEN, "fixed_od.json")))["fixedDrone_5_adj.xlsx"]["agents"]
    starts = [tuple(a["start"]) for a in fixed]
    goals = [a["goals"] for a in fixed]
    N = len(fixed)
    env = env_simulator(occ, radar_mode="drones", seed=1, **kw)
    env.create_world(N, 2, 0.95, 0.01, 1, 0.5, 0.15, 0.5, None, 5, [-8, 8])
    env.reset_world(N, [16, 18, 6], show=0, starts=starts, goals=goals)
    return env, N, starts, goals


def test_facade_reward_terms(native_lib, occ):
    env, N, starts, goals = _world(occ, reward_terms=True)
    ref = R.AttTerms(N, occ, radar_mode=0)
    ref.reset(starts, goals)
    rng = np.random.default_rng(4)
    record, holder = [[] for _ in range(N)], [None] * N
    want_rows = [[] for _ in range(N)]
    for step in range(5):
        act = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
        env.step([list(a) for a in act], step, 8, [16, 18, 6])
        rew, done, cg, record, holder, _, bbc = env.ss_reward(step, record, holder, [[] for _ in range(N)],
                                                              (None, None), True, None)
        ref.step(act)
        terms, own, _, _ = ref.ss_reward_terms()
        assert np.float32(np.sum([np.array(x) for x in own])) == np.float32(rew[0])
        for i in range(N):
            assert record[i][0] == 0.0 and abs(record[i][1] - terms[i, 3]) <= ATOL
            want_rows[i].append([terms[i, 10], terms[i, 3], 0.0, 0.0, 0.0, 0.0, terms[i, 9], 0.0, 0.0])
    for i in range(N):
        assert isinstance(holder[i], list) and len(holder[i]) == 5 and all(len(r) == 9 for r in holder[i])
        np.testing.assert_allclose(np.array(holder[i]), np.array(want_rows[i]), rtol=0, atol=ATOL)
    assert any(abs(r[1]) > 0 for rows in holder for r in rows) and all(r[0] > 0 for rows in holder for r in rows)


def test_facade_default_keeps_the_stub(native_lib, occ):
    env, N, _, _ = _world(occ)
    assert env._env.terms is None
    env.step([[0.1, -0.2]] * N, 0, 8, [16, 18, 6])
    record, holder = [[] for _ in range(N)], [None] * N
    out = env.ss_reward(0, record, holder, [[] for _ in range(N)], (None, None), True, None)
    assert out[3] == [[0.0, None]] * N and out[4] is holder and holder == [None] * N
