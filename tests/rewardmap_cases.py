"""Shared inputs of the reward-map tests (CPU and GPU): the exact-threshold batches of tests/thresholds.py
and tests/wgru_thresholds.py, their at-rest form (every agent standing on a landing position with zero
velocity, so that a zero-action step lands exactly there with ``pos == pre_pos``), seeded random states
in motion and the points the map is asked for.  No GPU needed."""
import functools

import numpy as np

from oracle.consts import BOUND
from tests import thresholds as T
from tests import wgru_thresholds as WT

ATT_CASES = (3, 5)                                              # N
WGRU_CASES = ((3, 4), (3, 9), (3, 32), (8, 4), (8, 9), (8, 32))  # (N, W): W shorter than, just past and at the
                                                                #  32-bit mask form of the step's waypoint cache


@functools.lru_cache(maxsize=None)
def att_batch(N):
    """(state dict, occ): thresholds.py's families plus the near-band ones, wp_cur = 0."""
    fam, var, st, occ = T.build(N, seed=N)
    near = T.build_near(N)
    st = {k: np.concatenate([st[k], near[2][k]]) for k in st}
    st["wp_cur"] = np.zeros(st["cnt"].shape, np.int32)
    st["start"] = st["pos"].copy()
    return st, occ


def _collision_rows(st, n=4):
    """WGRU envs appended to the threshold batch: copies of its first envs with agent 1 moved to within
    2 pB of agent 0 (and agent 0 of the last copy across a bound line).  The batch itself holds no
    drone contact, so mask bit 1 would otherwise never be set among the compared rows."""
    ext = {k: v[:n].copy() for k, v in st.items()}
    for e in range(n):
        p = ext["pos"][e, 0]
        ext["pos"][e, 1] = (p[0] + 3.0, p[1] + (4.0 if e % 2 else 3.5))       # 5 m (contact) / 4.6 m
        ext["pre_pos"][e, 1] = ext["pos"][e, 1]
        ext["vel"][e] = 0.0
        ext["post"][e] = ext["pos"][e]
    return {k: np.concatenate([st[k], ext[k]]) for k in st}


@functools.lru_cache(maxsize=None)
def wgru_batch(N, W):
    """(state dict, occ) without the random polylines (they test nothing the others do not), plus the
    drone-contact rows."""
    fam, var, st = WT.build(N, W)
    keep = tuple(sorted(f for f in set(fam) if f != "xt_random"))
    fam, var, st = WT.select(fam, var, st, keep)
    st = _collision_rows(st)
    return st, T.threshold_map()


def at_rest(st, landing):
    """The batch with every agent standing on its landing position: pos = pre_pos = landing, vel = 0."""
    out = {k: v.copy() for k, v in st.items()}
    out["pos"], out["pre_pos"] = landing.copy(), landing.copy()
    out["vel"] = np.zeros_like(st["vel"])
    return out


def all_rows(E, N):
    """(env_idx, agent) of every (env, agent) pair, env-major."""
    return np.repeat(np.arange(E, dtype=np.int32), N), np.tile(np.arange(N, dtype=np.int32), E)


def coverage(variant, mask, terms):
    """Every mask bit 0..5 takes both values; every reward branch of the variant occurs (WGRU: bound,
    building, goal, normal with and without the +3 bonus, penalty on and off)."""
    mask = np.asarray(mask).reshape(-1)
    terms = np.asarray(terms).reshape(-1, 12)
    for b in range(6):
        on = (mask >> b) & 1
        assert on.any() and not on.all(), (variant, "mask bit", b, int(on.sum()), on.size)
    if variant == "wgru":
        bound, building = (mask & 1) != 0, ((mask & 1) == 0) & ((mask & 8) != 0)
        goal, normal = ((mask & 9) == 0) & ((mask & 4) != 0), (mask & 13) == 0
        for name, sel in (("bound", bound), ("building", building), ("goal", goal), ("normal", normal)):
            assert sel.any(), name
        assert (terms[normal][:, 1] == 3).any() and (terms[normal][:, 1] == 0).any()
        assert (terms[:, 5] != 0).any() and (terms[~goal][:, 5] == 0).any()
        assert (terms[:, 2] == -3).any() and (terms[:, 2] > -3).any()


@functools.lru_cache(maxsize=None)
def moving_state(variant, N, W, E=6, seed=0):
    """A seeded random state in motion on the threshold map: agents spread over the map with non-zero
    velocities, waypoint lists of random length; WGRU: a random subset of the waypoints removed (never
    all).  Keys as the threshold batches'."""
    rng = np.random.default_rng(1000 * N + W + seed)
    pos = np.stack([rng.uniform(BOUND[0] + 10, BOUND[1] - 10, (E, N)), rng.uniform(BOUND[2] + 10, BOUND[3] - 10, (E, N))], -1)
    vel = rng.uniform(-3, 3, (E, N, 2))
    pre = pos - 0.5 * vel
    cnt = rng.integers(1, W + 1, (E, N)).astype(np.int32)
    wp = np.round(np.stack([rng.uniform(BOUND[0] + 5, BOUND[1] - 5, (E, N, W)),
                            rng.uniform(BOUND[2] + 5, BOUND[3] - 5, (E, N, W))], -1) * 8) / 8
    cur = np.zeros((E, N), np.int32)
    goal = np.zeros((E, N, 2))
    for e in range(E):
        for i in range(N):
            c = int(cnt[e, i])
            wp[e, i, c:] = wp[e, i, c - 1]
            last = c - 1
            if variant == "wgru" and c > 1:
                m = int(rng.integers(0, 1 << c)) & ~(1 << int(rng.integers(0, c)))
                cur[e, i] = WT._i32(m & 0xffffffff)
                last = max(k for k in range(c) if not (m >> k) & 1)
            goal[e, i] = wp[e, i, last]
    start = pos + rng.uniform(-20, 20, (E, N, 2))
    return dict(pos=pos, pre_pos=pre, vel=vel, goal=goal, wp=wp, cnt=cnt, wp_cur=cur, start=start)


def sample_points(st, e, i, rng, n_each=3):
    """Points for subject i of env e: inside the map's cells' neighbourhood, in the near-drone band of
    another agent (2.5 .. 10 m, and inside 5 m), on a waypoint, and outside the bound."""
    pts = []
    N = st["pos"].shape[1]
    for q in range(n_each):
        pts.append((rng.uniform(BOUND[0] + 3, BOUND[1] - 3), rng.uniform(BOUND[2] + 3, BOUND[3] - 3)))
        ci, cj = T.CELLS[int(rng.integers(len(T.CELLS)))]
        x0, x1, y0, y1 = T.square_of(ci, cj)
        pts.append((rng.uniform(x0 - 6, x1 + 6), rng.uniform(y0 - 6, y1 + 6)))
        j = (i + 1 + int(rng.integers(N - 1))) % N
        ang, rad = rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 11.0)
        pts.append((st["pos"][e, j, 0] + rad * np.cos(ang), st["pos"][e, j, 1] + rad * np.sin(ang)))
        k = int(rng.integers(int(st["cnt"][e, i]))) if q else 0          # the ATT flag looks at wp[0] alone
        pts.append((st["wp"][e, i, k, 0] + rng.uniform(-4, 4), st["wp"][e, i, k, 1] + rng.uniform(-4, 4)))
    pts.append((BOUND[0] - rng.uniform(0.5, 8), rng.uniform(BOUND[2], BOUND[3])))
    pts.append((rng.uniform(BOUND[0], BOUND[1]), BOUND[3] + rng.uniform(0.5, 8)))
    pts.append((BOUND[1] - rng.uniform(0.1, 2.4), rng.uniform(BOUND[2] + 5, BOUND[3] - 5)))
    return np.array(pts)
