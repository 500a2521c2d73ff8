"""The two WGRU oracles on the exact-threshold states of tests/wgru_thresholds.py, without a GPU: the C
oracle's variant 1 (oracle/aac_oracle.c) and the reference-shaped scalar restatement
(oracle/wgru_env_ref.py) step every state and must agree bit for bit; ``oc_cross_track`` equals
``geos.cross_track_distance`` on every state's path; ``check`` (rationals on the float coordinates) holds on
the oracle's outputs, both outcomes of every boolean family occur, and the builder dropped no state -- so
a failure of tests/test_wgru_threshold_gpu.py is never the builder's."""
import numpy as np
import pytest

from oracle import c_oracle, geos
from tests import thresholds as T
from tests import wgru_thresholds as WT

WS, NS = (4, 8, 9, 32), (3, 8)


@pytest.fixture(scope="module")
def occ():
    return T.threshold_map()


def _oracle_step(N, W, occ):
    fam, var, st = WT.build(N, W)
    E = len(fam)
    co = c_oracle.BatchedOracle(E, N, occ, W=W, variant="wgru")
    WT.oracle_state(co, st)
    co.step(np.zeros((E, N, 2), np.float32))
    return fam, var, st, co


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("N", NS)
def test_oracles_agree_and_check_holds(occ, N, W):
    fam, var, st, co = _oracle_step(N, W, occ)
    E = len(fam)
    assert E == len(var) == st["pos"].shape[0] and fam.count("xt_random") == WT.N_RANDOM
    assert (st["cnt"] <= W).all() and (st["cnt"] >= 1).all()
    assert np.array_equal(co.pos, st["post"])                  # dyadic moves: the post-step position is the builder's
    zero = np.zeros((N, 2))
    for e in range(E):
        env, kept = WT.scalar_env(st, e, occ)
        (o, r, n), rew, d, cg, bbc, masks, over = env.full_step(zero)
        tag = (fam[e], var[e], e)
        assert np.array_equal(co.mask[e], np.array(masks, np.uint8)), tag
        assert np.array_equal(co.done[e], np.array(d, np.uint8)), tag
        assert np.array_equal(co.reward[e], np.array([float(x) for x in rew], np.float32)), tag
        assert np.array_equal(co.own[e], o.astype(np.float32)) and np.array_equal(co.radar[e], r.astype(np.float32)), tag
        assert np.array_equal(co.bbc[e], np.array(bbc, np.uint8)) and bool(co.env_done[e]) == over, tag
        for i in range(N):
            ag = env.all_agents[i]
            cnt, m = int(st["cnt"][e, i]), int(co.wp_cur[e, i]) & 0xffffffff
            left = [list(st["wp"][e, i, k]) for k in range(cnt) if not (m >> k) & 1]
            assert left == [list(map(float, g)) for g in ag.goal], tag + (i, m)          # wp_cur
            assert np.array_equal(co.goal[e, i], np.array(ag.goal[-1], float)), tag + (i,)
            assert bool(co.reach[e, i]) == ag.reach_target, tag + (i,)
        s = int(st["subj"][e])
        cnt = int(st["cnt"][e, s])
        path = [tuple(st["start"][e, s])] + [tuple(w) for w in st["wp"][e, s, :cnt]]
        p = st["post"][e, s]
        assert c_oracle.cross_track(p[0], p[1], path[0], path[1:]) == geos.cross_track_distance(p[0], p[1], path), tag
    post = dict(pos=co.pos, wp_cur=co.wp_cur, goal=co.goal)
    seen = WT.check(fam, var, st, post, co.mask, co.reward, f"oracle N{N} W{W}")
    WT.both_ways(seen)


@pytest.mark.parametrize("W", WS)
def test_states_cover_the_named_cases(occ, W):
    """The cases this net exists for occur among the states, shown on the CPU alone: deciding waypoint indices 7, 8, 9
    and 31, cnt = 32, lists shorter than and equal to the kernel's 8-entry cache, every reward fix-up kind,
    the decisive xt_later pairs."""
    N = 3
    fam, var, st, co = _oracle_step(N, W, occ)
    subj = st["subj"]
    E = np.arange(len(fam))
    cnt = st["cnt"][E, subj]
    old = st["wp_cur"][E, subj].astype(np.int64) & 0xffffffff
    new = co.wp_cur[E, subj].astype(np.int64) & 0xffffffff
    popped = {int(x).bit_length() - 1 for x in (old ^ new) if x}
    idx = {v[1] for f, v in zip(fam, var) if f == "wp_index"}
    assert cnt.max() == W and st["wp"].shape[2] == W
    assert {0, 1, W - 2, W - 1} <= idx <= popped
    if W == 32:
        assert {7, 8, 9, 31} <= popped and (cnt == 32).sum() > 20
        assert any(o >> 31 for o in old) and any(n >> 31 and not o >> 31 for o, n in zip(old, new))
        nxt = {v[2] for f, v in zip(fam, var) if f == "wp_index"}
        assert min(nxt) < 8 <= max(nxt)
    m = co.mask[E, subj]
    kind = np.array([v[0] if f == "fix_kind" else "" for f, v in zip(fam, var)])
    assert {"none", "building", "bound", "goal", "corner", "corner_goal", "corner_building"} <= set(kind)
    # the states with a ray through a cell corner (the ones the kernel lists for the reward fix-up) take the
    # no-crash branch (rk = 2), the goal branch (rk = 0) and the building-crash branch (rk = 1)
    assert ((m[kind == "corner"] & 0b1101) == 0).all() and ((m[kind == "corner_goal"] & 0b1101) == 4).all()
    assert ((m[kind == "corner_building"] & 0b1001) == 8).all() and (m[kind == "bound"] & 1).any()
    pairs = [v for f, v in zip(fam, var) if f == "xt_later" and v[0].startswith("pair")]
    assert {(v[0], v[4]) for v in pairs} == {(a, b) for a in ("pairA", "pairB") for b in ("listed", "swapped")}
    # pair A's later segment wins: cross = 2.5 exactly, the reward's path term is 0 (else -3)
    for e, (f, v) in enumerate(zip(fam, var)):
        if f == "xt_later" and v[0] == "pairA":
            assert co.reward[e, subj[e]] == np.float32(0.0 + 0.0 - 3.0), (v, co.reward[e, subj[e]])
