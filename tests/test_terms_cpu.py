"""The reward-terms restatement (tests/terms_ref.py) against the oracles it copies, and the ledger's
fold rule in numpy.  No GPU.

The restatement's left-to-right slot sum must equal the oracle's own per-agent reward as a double, with
no tolerance (== on float64: -0.0 equals 0.0, nothing else differs), on the golden rollouts and on the
exact-threshold states; its state changes (waypoint pops, reach flags, wall counts) must be the oracle's."""
import copy
import os

import numpy as np
import pytest

from tests import terms_ref as R
from tests import thresholds as T
from tests import wgru_thresholds as WT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _same_state(a, b):
    for i in a.all_agents:
        x, y = a.all_agents[i], b.all_agents[i]
        assert x.goal == y.goal and x.waypoints == y.waypoints and x.reach_target == y.reach_target
        assert x.collide_wall_count == y.collide_wall_count


@pytest.mark.parametrize("name", ["rand5_drones", "rand8_obstacles", "ctrl5_combined", "headon2"])
def test_att_slot_sum_is_the_oracle_reward_on_goldens(name):
    g = np.load(os.path.join(GOLDEN, f"env_{name}.npz"))
    E, N = g["start"].shape[:2]
    seen = set()
    for e in range(E):
        env = R.AttTerms(N, g["occ"], radar_mode=int(g["radar_mode"]))
        env.reset([tuple(x) for x in g["start"][e]],
                  [[tuple(g["wps"][e, i, k]) for k in range(g["cnt"][e, i])] for i in range(N)])
        for t in range(g["act"].shape[0]):
            env.step(g["act"][t, e])
            twin = copy.deepcopy(env)
            team, done, _, _, masks = twin.ss_reward()
            terms, own, done2, masks2 = env.ss_reward_terms()
            _same_state(env, twin)
            assert done == done2 and masks == masks2
            assert np.array_equal(R.slot_sum(terms), own), (name, e, t)
            assert np.all(terms[:, 7] == 0) and np.all(terms[:, [1, 2, 4, 5, 8, 11]] == 0)
            # np.sum over the N per-agent values, as the oracle forms the team reward
            assert float(team[0]) == float(np.sum([np.array(x) for x in R.slot_sum(terms)])), (name, e, t)
            assert np.float32(team[0]) == g["reward"][t, e, 0], (name, e, t)
            seen |= {m & 7 for m in masks}
    assert 0 in seen          # the normal branch; crash / goal branches are asserted on the threshold states


def test_att_slot_sum_on_threshold_states():
    N, mode = 3, 0          # (the radar feeds no ATT reward term: AttTerms skips it)
    fam, var, st, occ = T.build(N, seed=3)
    near = T.build_near(N)
    keep = [e for e, f in enumerate(fam) if f not in T.RADAR_FAMILIES]      # the reward's own thresholds
    st = {k: np.concatenate([st[k][keep], near[2][k]]) for k in st}
    E = st["pos"].shape[0]
    branches = set()
    nonzero = np.zeros(R.WIDTH, bool)
    for e in range(E):
        env = R.att_env(st, e, occ, mode)
        env.step(np.zeros((N, 2), np.float32))
        twin = copy.deepcopy(env)
        team, done, cg, bbc, masks = twin.ss_reward()
        terms, own, _, masks2 = env.ss_reward_terms()
        _same_state(env, twin)
        assert masks == masks2
        assert np.array_equal(R.slot_sum(terms), own)
        assert float(team[0]) == float(np.sum([np.array(x) for x in own]))
        for i, m in enumerate(masks):
            branches.add("bound" if m & 1 else "drone" if m & 2 else "goal" if m & 4 else "normal")
        nonzero |= np.any(terms != 0, axis=0)
    assert branches == {"bound", "drone", "goal", "normal"}
    assert nonzero[0] and nonzero[6]


@pytest.mark.parametrize("W", [4, 9])
def test_wgru_slot_sum_on_threshold_states(W):
    N = 3
    occ = T.threshold_map()
    fam, var, st = WT.select(*WT.build(N, W), [f for f in set(WT.build(N, W)[0]) if f != "xt_random"])
    E = len(fam)
    branches = set()
    nonzero = np.zeros(R.WIDTH, bool)
    for e in range(E):
        env = R.wgru_env(st, e, occ)
        env.step(np.zeros((N, 2), np.float32))
        twin = copy.deepcopy(env)
        rew, done, cg, bbc, masks = twin.ss_reward()
        terms, own, done2, masks2 = env.ss_reward_terms()
        _same_state(env, twin)
        assert done == done2 and masks == masks2
        assert np.array_equal(R.slot_sum(terms), np.array([float(x) for x in rew])), (fam[e], var[e])
        assert np.array_equal(own, np.array([float(x) for x in rew]))
        assert np.all(terms[:, 6:8] == 0)
        for m in masks:
            branches.add("bound" if m & 1 else "building" if m & 8 else "goal" if m & 4 else "normal")
        nonzero |= np.any(terms != 0, axis=0)
    assert branches == {"bound", "building", "goal", "normal"}
    assert nonzero[:6].all() and nonzero[8:].all()


def test_names_table_matches_the_header():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "aac_terms.h")).read()
    names = re.search(r'#define AAC_TERMS_NAMES "([^"]+)"', src).group(1).split(",")
    assert tuple(names) == R.NAMES
    assert int(re.search(r"#define AAC_TERMS_W (\d+)", src).group(1)) == R.WIDTH == len(names)
    assert int(re.search(r"#define AAC_TERMS_SLOTS (\d+)", src).group(1)) == R.SLOTS
    assert int(re.search(r"#define AAC_STATS_EPW (\d+)",
                         open(os.path.join(root, "include", "aac_stats.h")).read()).group(1)) == R.EPW


def test_ledger_fold_rule():
    """The numpy ledger against a plain per-episode tally: counts exact, min / max exact, sums within
    rounding; the quota skips an env for good; the tree's order is the documented one."""
    rng = np.random.default_rng(0)
    E, N, steps = 300, 3, 12
    led = R.LedgerRef(E, N)
    run = np.zeros((E, R.SLOTS))
    eps = [[] for _ in range(E)]
    quota = np.full(E, 2)
    for s in range(steps):
        terms = rng.normal(size=(E, N, R.WIDTH))
        done = rng.random(E) < 0.3
        led.accumulate(terms, done, quota)
        for e in range(E):
            if len(eps[e]) >= 2:
                continue
            run[e] += terms[e, :, :R.SLOTS].sum(0)
            if done[e]:
                eps[e].append(run[e].copy())
                run[e] = 0
    allv = np.array([v for l in eps for v in l])
    n, s, q, lo, hi = led.reduce()
    assert n == len(allv) and n > E and np.array_equal(led.ep_count, [len(l) for l in eps])
    np.testing.assert_allclose(s, allv.sum(0), rtol=0, atol=1e-9)
    np.testing.assert_allclose(q, (allv ** 2).sum(0), rtol=0, atol=1e-9)
    np.testing.assert_allclose(lo, allv.min(0), rtol=0, atol=1e-12)
    np.testing.assert_allclose(hi, allv.max(0), rtol=0, atol=1e-12)
    # the tree: entry j meets j + 128 first
    v = np.zeros(256)
    v[0], v[128], v[1] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert R._tree(v, np.add) == 1.0 and (1.0 + 2.0 ** -53) + 2.0 ** -53 == 1.0 and 1.0 + 2.0 ** -52 != 1.0
    v[128], v[129] = 0.0, 2.0 ** -53          # now 1 and 129 meet first: their sum survives
    assert R._tree(v, np.add) == 1.0 + 2.0 ** -52
