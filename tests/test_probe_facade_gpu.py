"""``env_simulator(radar_probes=True)``: ``step`` returns the reference's six probe lists (ATT/env:1051-1170,
:2720) from a radar probe of the step's state; with the default flag the six empty lists, and the state,
normalised state and ``ss_reward`` outputs are the same either way."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _world(occ, mode, **kw):
    from multi_agent_aac_amd.env import env_simulator
    fixed = json.load(open(os.path.join(GOLDEN, "fixed_od.json")))["fixedDrone_3drones.xlsx"]["agents"]
    starts = [tuple(a["start"]) for a in fixed]
    goals = [a["goals"] for a in fixed]
    N = len(fixed)
    assert N == 3
    env = env_simulator(occ, radar_mode=mode, seed=1, **kw)
    env.create_world(N, 2, 0.95, 0.01, 1, 0.5, 0.15, 0.5, None, 5, [-8, 8])
    env.reset_world(N, [16, 18, 6], show=0, starts=starts, goals=goals)
    return env, N


def _flat(x):
    """Nested lists / tuples / dicts / arrays -> one float64 vector (bit comparison of whole results)."""
    if isinstance(x, dict):
        return np.concatenate([_flat(v) for v in x.values()]) if x else np.zeros(0)
    if isinstance(x, (list, tuple)):
        return np.concatenate([_flat(v) for v in x]) if len(x) else np.zeros(0)
    return np.zeros(0) if x is None else np.asarray(x, dtype=np.float64).reshape(-1)


@pytest.mark.parametrize("mode", ["drones", "combined"])
def test_facade_probe_lists(native_lib, occ, mode):
    on, N = _world(occ, mode, radar_probes=True)
    off, _ = _world(occ, mode)
    assert off._probe is None and off.last_probes is None
    cells = int(np.count_nonzero(occ))
    rng = np.random.default_rng(6)
    hit_total = 0
    for step in range(3):
        act = [list(a) for a in rng.uniform(-1, 1, (N, 2)).astype(np.float32)]
        res = on.step(act, step, 8, [16, 18, 6])
        base = off.step(act, step, 8, [16, 18, 6])
        assert len(res) == len(base) == 8 and list(base[2:]) == [[], [], [], [], [], []]
        state, norm, polys, st, ed, hits, lines, mini = res
        assert np.array_equal(_flat(state).view(np.uint64), _flat(base[0]).view(np.uint64))
        assert np.array_equal(_flat(norm).view(np.uint64), _flat(base[1]).view(np.uint64))
        pr = on.last_probes
        assert set(pr) == {"dist", "point", "end", "kind", "id"} and pr["dist"].shape == (1, N, 18)
        # the occupied cells, x-major, as (4, 2) corner arrays
        assert len(polys) == cells and all(isinstance(p, np.ndarray) and p.shape == (4, 2) for p in polys)
        ij = np.argwhere(np.asarray(occ))
        for p, (i, j) in zip(polys, ij):
            assert p.min(0).tolist() == [455.0 + 10 * i, 255.0 + 10 * j] and p.max(0).tolist() == [465.0 + 10 * i, 265.0 + 10 * j]
        assert len(st) == len(ed) == len(hits) == len(lines) == len(mini) == N
        for i in range(N):
            c = tuple(on.all_agents[i].pos)
            assert list(st[i]) == list(ed[i]) == list(range(0, 360, 20))
            assert all(st[i][d] == c for d in st[i])
            assert [ed[i][20 * r] for r in range(18)] == [tuple(x) for x in pr["end"][0, i]]
            assert lines[i] == [(c, ed[i][20 * r]) for r in range(18)]
            want = [tuple(x) for x in pr["point"][0, i][pr["kind"][0, i] != 0]]
            assert hits[i] == want and mini[i] == want and all(isinstance(h, tuple) for h in hits[i])
            hit_total += len(want)
        # state[1]: the radar rows the facade hands out are the probe's distances, rounded to fp32
        assert np.array_equal(np.stack(state[1]).astype(np.float32).view(np.uint32),
                              pr["dist"][0].astype(np.float32).view(np.uint32))
        rec = lambda: ([[] for _ in range(N)], [None] * N, [[] for _ in range(N)])      # noqa: E731
        a = on.ss_reward(step, *rec(), (None, None), True, None)
        b = off.ss_reward(step, *rec(), (None, None), True, None)
        assert np.array_equal(_flat(a).view(np.uint64), _flat(b).view(np.uint64)) and len(a) == len(b) == 7
    assert mode == "drones" or hit_total > 0


def test_facade_default_is_the_stub(native_lib, occ):
    env, N = _world(occ, "drones")
    out = env.step([[0.1, -0.2]] * N, 0, 8, [16, 18, 6])
    assert list(out[2:]) == [[], [], [], [], [], []] and env.last_probes is None
