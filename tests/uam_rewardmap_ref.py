"""Test-side restatement of the UAM reward map (include/aac_uam_rmap.h): one aircraft of one env of a state
dict evaluated at a test position by the oracle's own code.  Test infrastructure only, no GPU needed.

``MapRef(state, e, N).row(i, point, pre, prev2, rmin)`` takes env e of the state (``oracle.uam_ref.
env_from_state``), puts aircraft i at the point, recomputes its neighbour dict (``UAMEnv.neighbours``) and its
``observableSpace`` (``UAMEnv.radar``) there, and runs ``tests.uam_terms_ref.UamTerms.ss_reward_terms`` over
that one aircraft: the coefficients start at their base values and only its own bearings double them; the
other aircraft keep the state's ``pos`` and ``reach``.  tests/test_uam_rewardmap_cpu.py holds the rows, pushed
through ``rewardmap.uam_step_rows``, to the whole-env ``ss_reward_terms`` bit for bit.

Also here, shared by the CPU and the GPU tests: the seeded random batch (``random_batch``), the displaced
points aimed at features (``feature_points``) and the coverage assertion (``assert_coverage``)."""
import functools

import numpy as np

from oracle import uam_ref as U
from tests import uam_terms_ref as R

BAND, BAND_DBL, CRASH_DBL, PREV_TWO = 1, 2, 4, 8
KEYS = ("reward", "terms", "mask", "done", "bbc", "flags", "rays")


class _Only(dict):
    """The env's aircraft dict whose iteration shows one aircraft (lookups by index see them all)."""

    def __init__(self, d, i):
        super().__init__(d)
        self._i = i

    def items(self):
        return [(self._i, self[self._i])]


class MapRef:
    def __init__(self, state, e, N):
        self.state, self.e, self.N = state, e, N
        self.env = R.uam_env(state, e, N)
        self.top2 = [int(j) for j in state["top2"][e].reshape(N, 2).reshape(-1)]

    def row(self, i, point, pre=None, prev2=None, rmin=None):
        """The map row of aircraft i at ``point``: dict of reward, terms [12], mask, done, bbc [4], flags,
        rays [18] (the radar at the point, also when ``rmin`` replaces its minimum)."""
        env, N = self.env, self.N
        ag = env.all_agents[i]
        keep = (ag.pos, ag.pre_pos, ag.reach_target, ag.surroundingNeighbor, ag.pre_surroundingNeighbor,
                ag.observableSpace)
        everyone = env.all_agents
        try:
            ag.pos = np.array([float(point[0]), float(point[1])])
            ag.pre_pos = ag.pos.copy() if pre is None else np.array([float(pre[0]), float(pre[1])])
            ag.surroundingNeighbor = env.neighbours(ag)
            rays = env.radar(i)
            ag.observableSpace = rays if rmin is None else np.array([float(rmin)])
            p2 = self.top2[2 * i:2 * i + 2] if prev2 is None else [int(j) for j in prev2]
            ag.pre_surroundingNeighbor = {j: None for j in p2 if j != 255}
            env.all_agents = _Only(everyone, i)
            terms, reward, done, _, bbc, mask = env.ss_reward_terms()
            ev = env.events
        finally:
            env.all_agents = everyone
            (ag.pos, ag.pre_pos, ag.reach_target, ag.surroundingNeighbor, ag.pre_surroundingNeighbor,
             ag.observableSpace) = keep
            ag.bound_collision = ag.cloud_collision = ag.drone_collision = False
        fl = (BAND if ev["band"][0] else 0) | (BAND_DBL if ev["band_dbl"][0] else 0) | \
             (CRASH_DBL if ev["crash_dbl"][0] else 0) | (PREV_TWO if int(mask[0]) & 32 else 0)
        return dict(reward=float(reward[0]), terms=terms[i].copy(), mask=np.uint8(mask[0]), done=np.uint8(done[0]),
                    bbc=np.array(bbc, dtype=np.uint8), flags=np.uint8(fl), rays=np.asarray(rays, dtype=np.float64))


def rows(state, N, points, env=0, agent=0, pre=None, prev2=None, rmin=None):
    """M rows as stacked numpy arrays (``KEYS``); env / agent scalars or [M]; pre None, [M][2]; prev2 None or
    [M][2]; rmin None, a scalar or [M]."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    M = len(points)
    env = np.broadcast_to(np.asarray(env), (M,))
    agent = np.broadcast_to(np.asarray(agent), (M,))
    rmin = None if rmin is None else np.broadcast_to(np.asarray(rmin, dtype=np.float64), (M,))
    refs, out = {}, {k: [] for k in KEYS}
    for m in range(M):
        e = int(env[m])
        if e not in refs:
            refs[e] = MapRef(state, e, N)
        r = refs[e].row(int(agent[m]), points[m], None if pre is None else pre[m],
                        None if prev2 is None else prev2[m], None if rmin is None else rmin[m])
        for k in KEYS:
            out[k].append(r[k])
    return {k: np.array(v) for k, v in out.items()}


def kinds(mask):
    """The reward branch from the mask: 0 bound, 1 cloud, 2 drone, 3 goal, 4 normal."""
    mask = np.asarray(mask).astype(np.int64)
    k = np.full(mask.shape, 4)
    k[(mask & 16) != 0] = 3
    k[(mask & 4) != 0] = 2
    k[(mask & 2) != 0] = 1
    k[(mask & 1) != 0] = 0
    return k


def assert_coverage(mask, flags, blocks=None):
    """Every branch occurs and every flag bit occurs both ways over the rows (``mask``, ``flags`` of any
    shape).  ``blocks``: a list of per-env (rows [N][12], flags [N], mask [N]) in aircraft order -- at least
    one env must carry a doubling from an earlier aircraft into a later aircraft's non-zero crash value or
    near-drone term, so that the scaling rule of ``rewardmap.uam_step_rows`` is observed, not vacuous."""
    mask, flags = np.asarray(mask).reshape(-1), np.asarray(flags).reshape(-1)
    k = kinds(mask)
    assert set(np.unique(k)) == {0, 1, 2, 3, 4}, np.unique(k)
    for bit in (BAND, BAND_DBL, CRASH_DBL, PREV_TWO):
        assert ((flags & bit) != 0).any() and ((flags & bit) == 0).any(), bit
    if blocks is not None:
        crash_seen = band_seen = 0
        for t, fl, mk in blocks:
            fl, kk = np.asarray(fl).astype(np.int64), kinds(mk)
            cd = ((kk == 2) & ((fl & CRASH_DBL) != 0)).astype(np.int64)
            bd = (((fl & BAND) != 0) & ((fl & BAND_DBL) != 0)).astype(np.int64)
            crash_seen += int(((np.cumsum(cd) - cd > 0) & (kk < 3)).sum())
            band_seen += int(((np.cumsum(bd) - bd > 0) & (np.asarray(t)[:, 6] != 0)).sum())
        assert crash_seen > 0 and band_seen > 0, (crash_seen, band_seen)


# ------------------------------------------------------------------ shared inputs
def _top2(pos):
    N = len(pos)
    top2 = np.full((N, 2), 255, np.uint8)
    for i in range(N):
        order = sorted((j for j in range(N) if j != i), key=lambda j: float(np.linalg.norm(pos[j] - pos[i])))
        top2[i, :len(order[:2])] = order[:2]
    return top2


CENTRES = ((9.0, 20.0), (30.0, 14.0), (16.2, 20.0), (23.8, 12.0), (10.0, 12.5), (34.0, 29.0), (2.0, 20.0),
           (20.0, 38.4), (13.0, 31.0), (30.0, 26.0))


@functools.lru_cache(maxsize=None)
def random_batch(E, N, seed=0):
    """(pre-step state dict, actions [E][N][2]): aircraft clustered around a centre per env (open space, beside
    the runway, the clouds and the bound), so that one step shows every branch, both bearings of the band
    and of the collision, finished aircraft and goal touches."""
    rng = np.random.default_rng(seed)
    st = dict(pos=np.zeros((E, N, 2)), vel=np.zeros((E, N, 2)), goal=np.zeros((E, N, 2)), reach=np.zeros((E, N), np.uint8),
              clouds=np.zeros((E, 2, 2)), cloud_kind=np.zeros((E, 2), np.int32), cloud_tgt=np.zeros(E, np.int32),
              step=np.zeros(E, np.int32), top2=np.zeros((E, N, 2), np.uint8), heading=np.zeros((E, N)))
    spread = 1.2 + 0.35 * np.sqrt(N)
    for e in range(E):
        c = np.array(CENTRES[e % len(CENTRES)])
        pos = c + rng.uniform(-spread, spread, (N, 2))
        pos = np.clip(pos, 0.2, 39.8)
        ang, spd = rng.uniform(0, 2 * np.pi, N), rng.uniform(0, 1, N)
        st["pos"][e] = pos
        st["vel"][e] = np.stack([spd * np.cos(ang), spd * np.sin(ang)], 1)
        g = np.where(pos[:, :1] < 20.0, np.array([[38.0, 3.0]]), np.array([[3.0, 37.0]])) + rng.uniform(-1, 1, (N, 2))
        near = rng.random(N) < 0.15                      # a goal within reach of the step
        g[near] = pos[near] + rng.uniform(-1.2, 1.2, (int(near.sum()), 2))
        st["goal"][e] = g
        st["reach"][e] = rng.random(N) < 0.08
        st["cloud_kind"][e] = (e % 2, e % 4)
        st["clouds"][e, 0] = (10.0, 10.0) if e % 2 == 0 else (35.0, 30.0)
        st["clouds"][e, 1] = ((5.0, 22.5), (35.0, 22.5))[e % 2] if e % 3 else c + rng.uniform(-2, 2, 2)
        st["cloud_tgt"][e] = 3
        st["top2"][e] = _top2(pos)
    st["pre_pos"] = st["pos"] - 0.5 * st["vel"]
    st["pre_vel"] = st["vel"].copy()
    st["start"] = st["pos"] - rng.uniform(0.5, 3.0, (E, N, 1)) * np.sign(st["goal"] - st["pos"])
    return st, rng.uniform(-1, 1, (E, N, 2))


def oracle_step(pre, e, N, act):
    """Env e of ``pre`` stepped by the oracle: (post-step state of that env as a batch of one, terms [N][12],
    reward, done, bbc, mask)."""
    env = R.uam_env(pre, e, N)
    t, r, d, _, bbc, mk, _ = env.full_step_terms(act)
    s = U.state_of(env)
    post = {k: np.asarray(v)[None] for k, v in s.items()}
    post["cloud_kind"] = np.asarray(pre["cloud_kind"][e])[None]
    return post, t, r, np.asarray(d, dtype=np.uint8), np.asarray(bbc, dtype=np.uint8), mk


def feature_points(state, N, seed=0, per=2):
    """Seeded test positions aimed at what the reward reacts to, for every env of ``state``: around another
    aircraft at 0.9-5.5 m on both sides of the bearing window, inside and beside both clouds and the runway,
    within pB of each bound (``pre`` the subject's live position), on the goal, in open space.  Returns
    (points [M][2], env [M], agent [M], pre [M][2])."""
    rng = np.random.default_rng(seed)
    E = state["pos"].shape[0]
    pts, env, agent, pre = [], [], [], []

    def add(e, i, p, live=False):
        p = np.clip(np.asarray(p, dtype=np.float64), -0.4, 40.4)
        pts.append(p)
        env.append(e)
        agent.append(i)
        pre.append(state["pos"][e, i] if live else p)

    for e in range(E):
        for _ in range(per):
            i = int(rng.integers(N))
            j = int((i + 1 + rng.integers(N - 1)) % N)
            q = state["pos"][e, j]
            for lo, hi in ((0.9, 1.1), (1.9, 2.1), (2.0, 5.0), (4.9, 5.5)):
                d = rng.uniform(lo, hi)
                for a in (rng.uniform(0.0, 0.5 * np.pi), rng.uniform(0.5 * np.pi, 2 * np.pi)):
                    # the subject at q - d (cos a, sin a): bearing(subject -> q) = 360 - deg(a) or -deg(a)
                    add(e, i, q - d * np.array([np.cos(a), np.sin(a)]))
            for k, rad in enumerate(U.CLOUD_RADIUS):
                c = state["clouds"][e, k]
                a = rng.uniform(0, 2 * np.pi)
                u = np.array([np.cos(a), np.sin(a)])
                add(e, i, c + rng.uniform(0, rad) * u)
                add(e, i, c + (rad + U.PB + rng.uniform(-0.05, 0.6)) * u)
            x0, x1, y0, y1 = U.RUNWAY
            add(e, i, (rng.uniform(x0, x1), rng.uniform(y0, y1)))
            add(e, i, (x0 - U.PB + rng.uniform(-0.3, 0.1), rng.uniform(y0, y1)))
            add(e, i, (rng.uniform(x0, x1), y1 + U.PB + rng.uniform(-0.1, 0.3)))
            b = U.BOUND
            add(e, i, (b[0] + rng.uniform(0, U.PB), rng.uniform(5, 35)), live=True)
            add(e, i, (b[1] - rng.uniform(0, U.PB), rng.uniform(5, 35)), live=True)
            add(e, i, (rng.uniform(5, 35), b[2] + rng.uniform(0, U.PB)), live=True)
            add(e, i, (rng.uniform(5, 35), b[3] - rng.uniform(0, U.PB)), live=True)
            add(e, i, state["goal"][e, i] + rng.uniform(-0.7, 0.7, 2))
            add(e, i, state["goal"][e, i] + np.array([1.5 * U.APO + rng.uniform(-0.02, 0.02), 0.0]))
            add(e, i, rng.uniform(3, 37, 2))
    return np.array(pts), np.array(env, np.int32), np.array(agent, np.int32), np.array(pre)
