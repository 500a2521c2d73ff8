"""``uam.env_simulator(reward_terms=True)``: ``ss_reward_Mar_changeskin`` fills ``eps_status_holder`` with
the reference's per-step pieces (UAM/env:4651-4665) from the kernel's reward terms; the E = 1 loop of
tests/test_uam_gpu.py::test_uam_facade_loop against tests/uam_terms_ref.py.  With the default flag the
holders stay empty."""
import random

import numpy as np
import pytest

from oracle import uam_ref as U
from tests import uam_terms_ref as R

pytestmark = pytest.mark.gpu
TIGHT, RADAR = 1e-12, 1e-9
# holder key -> (slot, sign, tolerance): the reference lists penalties unsigned
KEYS = {"goal_leading_reward": (3, 1.0, TIGHT), "near_building_penalty": (5, -1.0, RADAR),
        "near_drone_penalty": (6, -1.0, TIGHT), "current_drone_speed": (9, 1.0, TIGHT),
        "Euclidean_dist_to_goal": (10, 1.0, TIGHT), "deviation_to_ref_line": (8, 1.0, TIGHT)}


def _world(N, **kw):
    from multi_agent_aac_amd import uam
    s, g, c0, c1 = U.sample_episode(N, random.Random(21), np.random.RandomState(21))
    st, go, cl = np.array(s), np.array(g), np.array((c0, c1), dtype=np.int32)
    env = uam.env_simulator(seed=1, **kw)
    env.create_world(N, 2, 0.95, 0.01, 1, 0.5, 0.15, 0.5, None, 1, [-0.5, 0.5])
    env.reset_world_change_skin(N, starts=st, goals=go, clouds=cl)
    return env, st, go, cl


def _state_of(env):
    return {k: v.cpu().numpy() for k, v in env._env.get_state().items()}


def test_facade_reward_terms(native_lib):
    N = 5
    env, st, go, cl = _world(N, reward_terms=True)
    rng = np.random.default_rng(2)
    seen = set()
    for step in range(1, 30):
        act = rng.uniform(-0.5, 0.5, (N, 2))
        pre = _state_of(env)
        env.step(act, step, 0.5)
        r, d, cg, rec, holder, _, bbc = env.ss_reward_Mar_changeskin(step, [None] * N, [[] for _ in range(N)])
        t, r2, d2, cg2, bbc2, _, over = R.uam_env(pre, 0, N).full_step_terms(act)
        np.testing.assert_allclose(np.array(r, dtype=float), r2, rtol=0, atol=RADAR)
        assert list(d) == list(d2) and list(cg) == list(cg2) and bbc == list(bbc2)
        for i in range(N):
            assert set(holder[i]) == set(KEYS)
            for key, (slot, sign, tol) in KEYS.items():
                assert isinstance(holder[i][key], float)
                np.testing.assert_allclose(holder[i][key], sign * t[i, slot], rtol=0, atol=tol, err_msg=f"{step} {i} {key}")
                if holder[i][key] != 0:
                    seen.add(key)
            assert rec[i] == [0, float(r[i])]
        if env.episode_over(step):
            assert over
            break
    assert {"goal_leading_reward", "current_drone_speed", "Euclidean_dist_to_goal", "deviation_to_ref_line"} <= seen


def test_facade_default_is_unchanged(native_lib):
    N = 5
    env, *_ = _world(N)
    assert env._env.terms is None
    env.step(np.zeros((N, 2)), 1, 0.5)
    r, d, cg, rec, holder, coll, bbc = env.ss_reward_Mar_changeskin(1, [None] * N, [[] for _ in range(N)])
    assert holder == [{} for _ in range(N)]
    assert all(rec[i] == [0, float(r[i])] for i in range(N))
