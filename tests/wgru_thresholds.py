"""Exact-threshold states of the WGRU environment's reward (config 4, ``variant="wgru"``;
``wgru_reward`` in csrc/aac_env.hip, oracle/wgru_env_ref.py): the counterpart of tests/thresholds.py and
tests/uam_thresholds.py for the rules only this variant has.  Test infrastructure only, no GPU needed.

Each env has one subject agent (slot 0 in even envs, slot N - 1 in odd ones); the other agents are parked
along the top of the map on reference paths of their own (start = position, one waypoint).  The map is
``thresholds.threshold_map()``; outside ``fix_kind`` the subject stays more than 20 m from every cell and
bound line, so its radar reads 15 m on every ray and the near-building penalty is 0.  Coordinates are
multiples of 1/8 and the offsets 3-4-5 triples, so every distance the reference computes on a threshold
member is exact in float64; ``Batch.add`` proves it: the rational outcome (``exact_outcome``) and the
reference's float formulas (GEOS point distance, pointToSegment / closestPoint) must decide alike on
every state, and a member meant to sit on 5 m or 2.5 m must give exactly that float.  Siblings move one
coordinate by +-1 and +-2 ulp with ``nextafter``; they are stationary (zero velocity, zero action), so the
kinematics keep the position bit for bit.  Moving subjects have dyadic velocities below 10 m/s and a
dyadic post-step position, verified with rationals.  The unused waypoint slots of a subject hold its own
post-step position (inside the bound): a read past ``cnt`` would find a waypoint at distance 0.

Families (the list of remaining waypoints = the entries whose bit in ``wp_cur`` is clear):
  wp5_len1/2/3  the first remaining waypoint at GEOS point distance exactly 5 (strict <) and +-1, +-2 ulp,
                with 1, 2 and 3 remaining entries: flag only / pop without the bonus / pop and +3
  wp_prefix     only prefix minima are candidates and the first one inside 5 m is popped: a nearer later
                entry stays; the third prefix minimum as the first one inside
  wp_tie        two remaining waypoints at bit-equal distance below 5 (mirror images): the earlier is popped
  wp_next_tie   after the pop two entries at bit-equal distance: the first is next_wp; the subject moves, so
                the progress term tells them apart (by 4.0)
  wp_index      the deciding waypoint at list index 0, 1, 6, 7, 8, 9, cnt - 2, cnt - 1 for cnt in
                {8, 9, 16, 31, 32} (as far as W allows, and cnt = W): empty mask, earlier bits set, all but
                two removed, bit 31 set; the follow-up minimum below and at or above index 8; removed
                entries lie 1-4 m from the subject, so a reader that ignores the mask pops one of them
  wp_final_pop  the last entry is the one inside 5 m with more entries remaining: goal[-1] becomes the
                previous remaining entry
  xt_pb         cross-track distance exactly 2.5 and +-1, +-2 ulp: from the interior of an axis-parallel and
                of a 3-4-5 segment, beyond the path's start (1.5-2-2.5), at the vertex between two segments
  xt_proj       the subject on the perpendicular through a segment end (projection factor exactly 0 or 1)
                and +-1 ulp along the segment, the distance on either side of 2.5
  xt_degenerate start == wp[0], and two equal consecutive waypoints, 2.5 +- ulp from the subject
  xt_on_path    the subject on a vertex, on a segment's interior, and with a later segment through the point
  xt_later      the nearest segment is the k-th (k = 1, 2, 7, 8, 9, cnt - 1), the others far; and decisive
                pairs: an earlier segment at 2.5 + 1 ulp with a later one at exactly 2.5 (the later wins,
                reward term 0 instead of -3), an earlier one at 2.5 with a later one at 2.5 - 1 ulp, each
                also in swapped list order
  xt_random     random polylines on the 1/8 grid with repeated vertices and collinear runs, the subject
                within 6 m: compared with the oracles only (``check`` skips them)
  fix_kind      every reward branch (none, building contact, goal reached, bound crash) from the ``edge_near``
                geometry of tests/thresholds.py (a ray along a cell edge; the contact is the 64-gon's vertex 0
                on the corner the ray runs along) -- and, since the kernel lists a reward for the exact
                fix-up only where a ray touches a cell corner, from the ``corner`` construction: no crash
                (rk = 2), the goal on the subject (rk = 0), and the corner 3 m up the ray from inside the
                cell's row or column, where the 64-gon overlaps the cell (rk = 1).  A bound crash cannot
                have a flagged ray: no cell of the map lies within 15 m of a bound line.

``check`` states every non-random subject's outcome from rationals on the float coordinates: the popped
index, mask bit 4, the new wp_cur, goal[-1], the +3 bonus and cross <= pB.  The reference compares float
distances, so off the dyadic grid its float result is the truth; the builder only admits states where the
two agree."""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

from oracle import geos
from oracle.consts import BOUND, PB
from tests import thresholds as T

HOME = T.HOME
CENTRE = ((BOUND[0] + BOUND[1]) / 2.0, (BOUND[2] + BOUND[3]) / 2.0)
ULPS = (-2, -1, 0, 1, 2)
KEYS = ("pos", "pre_pos", "vel", "goal", "wp", "cnt", "wp_cur", "start")
BOOL_FAMILIES = ("wp5_len1", "wp5_len2", "wp5_len3", "xt_pb", "xt_proj", "xt_degenerate", "xt_later")
TWO_STEP_FAMILIES = ("wp5_len1", "wp5_len2", "wp5_len3", "wp_index", "wp_final_pop")
N_RANDOM = 1000
# (cell index, corner, ray) of tests/thresholds.py's corner construction used by fix_kind: fixed, so the
# builder's count is fixed (``_corner_start`` finds a lattice start for each)
CORNER_RAYS = ((0, 0, 3), (0, 1, 12), (1, 2, 6), (1, 3, 15), (2, 0, 12), (2, 3, 6))
# the same construction 3 m from the corner (a fifth of the ray), from inside the cell's row or column: the
# 64-gon overlaps the cell (1.5 m from its edge) while the 60-degree-family ray only touches the corner
CONTACT_RAYS = ((0, 0, 12), (1, 1, 3), (2, 2, 15), (0, 3, 6))
_up = T._up


def _corner_start_at(q, r, frac):
    """tests/thresholds.py ``_corner_start`` with the corner at the ray parameter nearest ``frac`` among the
    lattice points of the float segment (there it is 1/2): a start c whose ray r passes EXACTLY through q."""
    rad = float(20 * r) * (math.pi / 180.0)
    dx, dy = 15.0 * math.cos(rad), 15.0 * math.sin(rad)
    c0 = (q[0] - dx * frac, q[1] - dy * frac)
    e0 = T.ray_end(c0, r)
    ddx, ddy = e0[0] - c0[0], e0[1] - c0[1]
    u = min(float(np.spacing(c0[0])), float(np.spacing(c0[1])))
    nx, ny = int(Fr(ddx) / Fr(u)), int(Fr(ddy) / Fr(u))
    g = math.gcd(abs(nx), abs(ny))
    if g < 2 or Fr(ddx) != nx * Fr(u) or Fr(ddy) != ny * Fr(u):
        return None
    m = max(1, min(g - 1, round(frac * g)))
    cx, cy = q[0] - (m * (nx // g)) * u, q[1] - (m * (ny // g)) * u
    ex, ey = T.ray_end((cx, cy), r)
    C, E, Q = (Fr(cx), Fr(cy)), (Fr(ex), Fr(ey)), (Fr(q[0]), Fr(q[1]))
    if (E[0] - C[0]) * (Q[1] - C[1]) - (E[1] - C[1]) * (Q[0] - C[0]) != 0:
        return None
    t = (Q[0] - C[0]) / (E[0] - C[0])
    return (cx, cy) if 0 < t < 1 else None


def _far(j):
    """Distinct waypoints 40 m and more from HOME, inside the bound."""
    return (HOME[0] - 60.0 + 2.0 * j, HOME[1] - 44.0 - (j % 3))


def _d2(a, b):
    return (Fr(a[0]) - Fr(b[0])) ** 2 + (Fr(a[1]) - Fr(b[1])) ** 2


def _seg_d2(p, a, b):
    """Exact squared distance from p to the segment a-b."""
    P, A, B = (Fr(p[0]), Fr(p[1])), (Fr(a[0]), Fr(a[1])), (Fr(b[0]), Fr(b[1]))
    dx, dy = B[0] - A[0], B[1] - A[1]
    L = dx * dx + dy * dy
    if L == 0:
        return _d2(p, a)
    t = ((P[0] - A[0]) * dx + (P[1] - A[1]) * dy) / L
    t = min(max(t, Fr(0)), Fr(1))
    qx, qy = A[0] + t * dx, A[1] + t * dy
    return (P[0] - qx) ** 2 + (P[1] - qy) ** 2


# the float distance the reference compares is the rounded one: a squared distance within half an ulp of
# the threshold rounds onto it (ulp(2.5) = 2^-51; 2.5 has an even mantissa, the tie goes to it)
_PB_IN = (Fr(PB) + Fr(1, 2 ** 52)) ** 2


def exact_outcome(p, pre, vel, start, wps, mask):
    """``_exact_outcome`` (cached: the batches of different N share their subjects)."""
    return dict(_exact_outcome(tuple(p), tuple(pre), tuple(vel), tuple(start), tuple(tuple(w) for w in wps), int(mask)))


@functools.lru_cache(maxsize=None)
def _exact_outcome(p, pre, vel, start, wps, mask):
    """What WGRU/env:1815-1832 and :2621-2632, :1878-1890 give for a subject at p (rationals on the float
    coordinates).  wps: the cnt waypoints; mask: the removed bits.  Returns a dict: flag, pop (index or
    None), cur (the new mask), goal (index of goal[-1]), bonus, nxt (index of next_wp), seg (the nearest
    segment), cross2 (Fraction), cross_in, reward (the no-crash branch, near-building penalty 0)."""
    cnt = len(wps)
    rem = [k for k in range(cnt) if not (mask >> k) & 1]
    smallest, flag, pop, nxt = None, False, None, None
    for k in rem:
        d = _d2(p, wps[k])
        if smallest is None or d < smallest:
            smallest, nxt = d, k
            if d < 25:
                flag = True
                if len(rem) > 1:
                    pop = k
                    rest = [q for q in rem if q != k]
                    nxt = min(rest, key=lambda q: _d2(p, wps[q]))       # the first minimum
                break
    left = [k for k in rem if k != pop]
    cur = mask | ((1 << pop) if pop is not None else 0)
    bonus = flag and len(left) > 1
    pts = [tuple(start)] + [tuple(w) for w in wps]
    best, seg = None, None
    for k in range(cnt):
        d = _seg_d2(p, pts[k], pts[k + 1])
        if best is None or d < best:
            best, seg = d, k
        if best == 0:
            break
    cross_in = best < _PB_IN
    cross = math.sqrt(float(best))
    out = dict(flag=flag, pop=pop, cur=cur, goal=left[-1], bonus=bonus, nxt=nxt, seg=seg, cross2=best,
               cross_in=cross_in)
    out["reward"] = _reward(p, pre, vel, wps[nxt], bonus, cross if cross_in else None)
    return out


def _reward(p, pre, vel, nx, bonus, cross):
    """The no-crash branch of WGRU/env ss_reward without a near-building penalty; cross None = outside pB."""
    dref = 3 * ((-1 / PB) * cross + 1) if cross is not None else -3.0
    dtg = math.hypot(pre[0] - nx[0], pre[1] - nx[1]) - math.hypot(p[0] - nx[0], p[1] - nx[1])
    ssp = 3 * ((5.0 - min(math.hypot(vel[0], vel[1]), 5.0)) / 5.0)
    return (3.0 if bonus else 0.0) + dref + dtg - ssp


def _float_outcome(p, start, wps, mask):
    """The same decisions by the reference's float formulas (GEOS point distance, DistanceOp)."""
    cnt = len(wps)
    rem = [k for k in range(cnt) if not (mask >> k) & 1]
    smallest, flag, pop, nxt = math.inf, False, None, None
    for k in rem:
        d = geos.point_dist(p[0], p[1], wps[k][0], wps[k][1])
        if d < smallest:
            smallest, nxt = d, k
            if smallest < 5:
                flag = True
                if len(rem) > 1:
                    pop = k
                    rest = [q for q in rem if q != k]
                    nxt = min(rest, key=lambda q: geos.point_dist(wps[q][0], wps[q][1], p[0], p[1]))
                break
    cross = geos.cross_track_distance(p[0], p[1], [tuple(start)] + [tuple(w) for w in wps])
    return dict(flag=flag, pop=pop, nxt=nxt, cross=cross, cross_in=cross <= PB)


class Batch:
    def __init__(self, N, W):
        self.N, self.W = N, W
        self.rows, self.planned = [], 0

    def plan(self, n):
        self.planned += n

    def add(self, family, variant, p, wps, start=None, removed=(), vel=(0.0, 0.0), on=None, prove=True):
        """One env.  p: the subject's post-step position; its pre-step position is p - vel / 2.  on: the
        float the threshold member's deciding distance must equal exactly (5.0 or 2.5), with what it is
        ("wp" the first remaining waypoint's distance, "xt" the cross-track distance)."""
        N, W = self.N, self.W
        s = 0 if len(self.rows) % 2 == 0 else N - 1
        wps = [(float(x), float(y)) for x, y in wps]
        cnt = len(wps)
        assert 1 <= cnt <= W, (family, variant, cnt, W)
        p = (float(p[0]), float(p[1]))
        vel = (float(vel[0]), float(vel[1]))
        pre = (p[0] - vel[0] * 0.5, p[1] - vel[1] * 0.5)
        assert math.hypot(*vel) < 10.0
        for c in range(2):      # the kinematics' pos + vel * dt lands on p bit for bit
            assert Fr(pre[c]) + Fr(vel[c]) / 2 == Fr(p[c]) and pre[c] + vel[c] * 0.5 == p[c], (family, variant)
        start = p if start is None else (float(start[0]), float(start[1]))
        mask = 0
        for k in removed:
            assert 0 <= k < cnt
            mask |= 1 << k
        assert mask != (1 << cnt) - 1, "an empty goal list"
        for x, y in [p, pre, start] + wps:
            assert BOUND[0] < x < BOUND[1] and BOUND[2] < y < BOUND[3], (family, variant, x, y)
        if prove:
            ex, fl = exact_outcome(p, pre, vel, start, wps, mask), _float_outcome(p, start, wps, mask)
            for k in ("flag", "pop", "nxt", "cross_in"):
                assert ex[k] == fl[k], (family, variant, k, ex[k], fl[k], fl["cross"])
            if on is not None:
                what, val = on
                if what == "wp":
                    k = next(q for q in range(cnt) if not (mask >> q) & 1)
                    assert _d2(p, wps[k]) == Fr(val) ** 2 and geos.point_dist(p[0], p[1], *wps[k]) == val
                else:
                    assert ex["cross2"] == Fr(val) ** 2 and fl["cross"] == val, (family, variant, fl["cross"])
        pos = np.zeros((N, 2))
        for k in range(N):                           # the others along the top, 12 m apart
            pos[k] = (468.0 + 12.0 * k, 378.0)
        post = pos.copy()
        pos[s], post[s] = pre, p
        w = np.empty((N, W, 2))
        w[:] = CENTRE
        w[:, 0] = pos + np.array([0.0, -100.0])
        w[s] = p
        w[s, :cnt] = wps
        c = np.ones(N, np.int32)
        c[s] = cnt
        cur = np.zeros(N, np.int64)
        cur[s] = mask
        goal = w[:, 0].copy()
        goal[s] = wps[max(k for k in range(cnt) if not (mask >> k) & 1)]
        st = pos.copy()
        st[s] = start
        v = np.zeros((N, 2))
        v[s] = vel
        self.rows.append(dict(family=family, variant=variant, subj=s, pos=pos, pre_pos=pos.copy(), vel=v, goal=goal,
                              wp=w, cnt=c, wp_cur=cur.astype(np.uint32).view(np.int32), start=st, post=post))

    def arrays(self):
        assert len(self.rows) == self.planned, (len(self.rows), self.planned)
        fam = [r["family"] for r in self.rows]
        var = [r["variant"] for r in self.rows]
        st = {k: np.stack([r[k] for r in self.rows]) for k in KEYS + ("post",)}
        st["subj"] = np.array([r["subj"] for r in self.rows], np.int32)
        return fam, var, st


def _axis_point(d, j):
    """A point at distance exactly d from HOME, the direction turning with j."""
    return [(HOME[0] + d, HOME[1]), (HOME[0], HOME[1] + d), (HOME[0] - d, HOME[1]), (HOME[0], HOME[1] - d)][j % 4]


def _wp_families(B):
    W = B.W
    hx, hy = HOME
    # ---- wp5_len{1,2,3}: the first remaining waypoint on 5 m
    offs = ((3.0, 4.0), (-4.0, 3.0), (0.0, -5.0), (5.0, 0.0))
    for L in (1, 2, 3):
        B.plan(len(offs) * len(ULPS))
        for n, (ox, oy) in enumerate(offs):
            for u in ULPS:      # u > 0 moves the waypoint away from the subject
                if ox != 0.0:
                    D = (_up(hx + ox, u if ox > 0 else -u), hy + oy)
                else:
                    D = (hx, _up(hy + oy, u if oy > 0 else -u))
                lead = n % 2 == 1 and L + 1 <= W           # a removed entry 1 m away in front of it
                wps = ([(hx + 1.0, hy)] if lead else []) + [D] + [_far(j) for j in range(1, L)]
                B.add(f"wp5_len{L}", u, HOME, wps, removed=(0,) if lead else (), on=("wp", 5.0) if u == 0 else None)
    # ---- wp_prefix
    # (the last entry is goal[-1]: 4 m and more away, outside the goal test's 3.5 m)
    lists = [l for l in ([3.0, 2.0, 30.0], [6.0, 4.0, 3.0, 30.0], [9.0, 7.0, 8.0, 4.5, 2.0, 30.0], [6.0, 7.0, 4.5, 4.0],
                         [4.5, 6.0, 4.0], [8.0, 9.0, 4.0, 3.0, 30.0]) if len(l) <= W]
    B.plan(len(lists))
    for n, l in enumerate(lists):
        B.add("wp_prefix", n, HOME, [_axis_point(d, j + n) for j, d in enumerate(l)])
    # ---- wp_tie: mirror images about the subject
    ties = ((3.0, 2.5), (3.0, 3.5), (0.0, 4.875), (2.25, -4.0))
    B.plan(3 * len(ties))
    for n, (a, b) in enumerate(ties):
        D1, D2 = (hx + a, hy + b), (hx - a, hy - b)
        assert geos.point_dist(hx, hy, *D1) == geos.point_dist(hx, hy, *D2) < 5
        B.add("wp_tie", (n, 0), HOME, [D1, D2])
        B.add("wp_tie", (n, 1), HOME, [D2, D1, _far(2)])
        B.add("wp_tie", (n, 2), HOME, [_far(0), D1, D2, _far(3)])
    # ---- wp_next_tie: the subject moves by (2, 0); the candidates 8 m either side of it
    T1, T2, D = (hx + 8.0, hy), (hx - 8.0, hy), (hx, hy + 3.0)
    lists = [[D, T1, T2], [D, T2, T1], [T1, D, T2], [T2, D, T1], [_far(0), T2, D, T1], [_far(0), T1, D, T2]]
    B.plan(len(lists))
    for n, l in enumerate(lists):
        B.add("wp_next_tie", n, HOME, l, vel=(4.0, 0.0))
    # ---- wp_index
    cnts = sorted({c for c in (8, 9, 16, 31, 32) if c <= W} | {W})
    cases = []
    for cnt in cnts:
        for idx in sorted({k for k in (0, 1, 6, 7, 8, 9, cnt - 2, cnt - 1) if 0 <= k < cnt}):
            lowmod = min(cnt, 8)
            f_low = (idx + 3) % lowmod
            f_low = f_low if f_low != idx else (f_low + 1) % lowmod
            f_high = None
            if cnt > 8:
                f_high = 8 + (idx * 5 + 1) % (cnt - 8)
                if f_high == idx:
                    f_high = 8 + (f_high - 8 + 1) % (cnt - 8)
                if f_high == idx:
                    f_high = None
            fs = [f_low] + ([f_high] if f_high is not None else [])
            for f in fs:
                cases.append((cnt, idx, f, "empty"))
            cases.append((cnt, idx, fs[-1], "some"))
            cases.append((cnt, idx, fs[idx % len(fs)], "all_but_two"))
            if cnt == 32 and 31 not in (idx, fs[0]):
                cases.append((cnt, idx, fs[0], "bit31"))
    B.plan(len(cases))
    for cnt, idx, f, kind in cases:
        if kind == "empty":
            removed = set()
        elif kind == "some":
            removed = {r for r in range(cnt) if r not in (idx, f) and (r * 7 + idx) % 3 == 0}
        elif kind == "all_but_two":
            removed = {r for r in range(cnt) if r not in (idx, f)}
        else:
            removed = {31} | {r for r in range(cnt) if r not in (idx, f) and (r + idx) % 5 == 0}
        wps = []
        for k in range(cnt):
            if k == idx:
                wps.append((hx + 3.0, hy + 3.5))
            elif k == f:
                wps.append((hx, hy + 8.0))
            elif k in removed:
                wps.append((hx + 0.125 * (k + 1), hy - 1.0))
            else:
                wps.append(_far(k))
        B.add("wp_index", (cnt, idx, f, kind), HOME, wps, removed=sorted(removed), vel=(4.0, 0.0))
    # ---- wp_final_pop
    finals = [(3.0, 3.5), (-3.0, 2.5), (0.0, -4.875)]
    B.plan(2 * len(finals) + 1)
    for n, (a, b) in enumerate(finals):
        B.add("wp_final_pop", (n, 0), HOME, [_far(0), _far(1), (hx + a, hy + b)][-min(W, 3):])
        wps = [_far(0), (hx + 1.0, hy + 1.0), _far(2), (hx + a, hy + b)]
        B.add("wp_final_pop", (n, 1), HOME, wps, removed=(1,))
    wps = [_far(k) for k in range(W - 1)] + [(hx + 3.0, hy - 2.5)]
    B.add("wp_final_pop", ("full", W), HOME, wps, removed=tuple(range(1, W - 2)))


def _xt_families(B):
    W = B.W
    hx, hy = HOME
    on = lambda u: ("xt", 2.5) if u == 0 else None
    # ---- xt_pb
    B.plan(7 * len(ULPS))
    for u in ULPS:      # u > 0 moves the subject away from the path
        B.add("xt_pb", ("axis_x", u), (hx, _up(hy, u)), [(hx + 20.0, hy - 2.5), (hx + 20.0, hy - 30.0)][:W],
              start=(hx - 20.0, hy - 2.5), on=on(u))
        B.add("xt_pb", ("axis_y", u), (_up(hx, -u), hy), [(hx + 2.5, hy + 24.0)], start=(hx + 2.5, hy - 16.0), on=on(u))
        a = (hx - 13.0, hy - 21.5)                       # foot at the middle of a 30-40-50 segment
        B.add("xt_pb", ("345", u), (_up(hx, -u), hy), [(a[0] + 30.0, a[1] + 40.0)], start=a, on=on(u))
        a = (hx - 21.5, hy - 13.0)
        B.add("xt_pb", ("435", u), (_up(hx, u), hy), [(a[0] + 40.0, a[1] + 30.0)], start=a, on=on(u))
        S = (hx + 1.5, hy + 2.0)                         # beyond the path's start
        B.add("xt_pb", ("end", u), (_up(hx, -u), hy), [(S[0] + 18.0, S[1] + 24.0)], start=S, on=on(u))
        S = (hx - 2.0, hy + 1.5)
        B.add("xt_pb", ("end2", u), (_up(hx, u), hy), [(S[0] - 24.0, S[1] + 18.0)], start=S, on=on(u))
        V = (hx + 1.5, hy + 2.0)                         # the vertex between two segments (projection 0 on one)
        B.add("xt_pb", ("vertex", u), (_up(hx, -u), hy), [V, (V[0] + 24.0, V[1] - 18.0)], start=(V[0] + 18.0, V[1] + 24.0),
              on=on(u))
    # ---- xt_proj
    B.plan(18)
    for ux in (-1, 0, 1):
        for uy in (-1, 0, 1):
            p = (_up(hx, ux), _up(hy, uy))
            o = ("xt", 2.5) if ux == 0 and uy == 0 else None
            B.add("xt_proj", ("f0", ux, uy), p, [(hx + 20.0, hy - 2.5)], start=(hx, hy - 2.5), on=o)
            B.add("xt_proj", ("f1", ux, uy), p, [(hx, hy - 2.5), (hx, hy - 30.0)], start=(hx - 20.0, hy - 2.5), on=o)
    # ---- xt_degenerate
    B.plan(2 * len(ULPS))
    Dg = (hx + 1.5, hy + 2.0)
    for u in ULPS:
        B.add("xt_degenerate", ("start", u), (_up(hx, -u), hy), [Dg, (Dg[0] + 18.0, Dg[1] + 24.0)], start=Dg, on=on(u))
        B.add("xt_degenerate", ("repeat", u), (_up(hx, -u), hy),
              [(Dg[0] + 9.0, Dg[1] + 12.0), Dg, Dg, (Dg[0] + 24.0, Dg[1] - 18.0)], start=(Dg[0] + 18.0, Dg[1] + 24.0),
              on=on(u))
    # ---- xt_on_path
    B.plan(4)
    B.add("xt_on_path", "vertex", HOME, [HOME, (hx, hy + 20.0)], start=(hx - 20.0, hy), on=("xt", 0.0))
    B.add("xt_on_path", "interior", HOME, [(hx + 20.0, hy)], start=(hx - 20.0, hy), on=("xt", 0.0))
    B.add("xt_on_path", "interior345", HOME, [(hx + 15.0, hy + 20.0)], start=(hx - 15.0, hy - 20.0), on=("xt", 0.0))
    B.add("xt_on_path", "later", HOME, [(hx + 20.0, hy), (hx + 20.0, hy + 20.0), (hx, hy + 20.0), (hx, hy - 20.0)],
          start=(hx - 20.0, hy), on=("xt", 0.0))
    # ---- xt_later
    def path(cnt, near):
        """start + cnt waypoints far from HOME, but for the segments near = {k: (y, reversed)}: horizontal,
        20 m long, centred on the subject's x."""
        V = [(hx - 60.0 + j, hy - 50.0) for j in range(cnt + 1)]
        for k, (y, rev) in near.items():
            V[k], V[k + 1] = ((hx + 10.0, y), (hx - 10.0, y)) if rev else ((hx - 10.0, y), (hx + 10.0, y))
        return V[0], V[1:]

    singles, pairs = [], []
    for cnt in sorted({min(W, 16), W}):
        ks = sorted({k for k in (1, 2, 7, 8, 9, cnt - 1) if 1 <= k < cnt})
        singles += [(cnt, k) for k in ks]
        pairs.append((cnt, 1, cnt - 1))
        if cnt > 10:
            pairs.append((cnt, 7, 9))
    B.plan(len(singles) * len(ULPS) + 4 * len(pairs))
    for cnt, k in singles:
        for u in ULPS:
            st, wps = path(cnt, {k: (hy - 2.5, False)})
            p = (hx, _up(hy, u))
            B.add("xt_later", ("single", cnt, k, u), p, wps, start=st, on=on(u))
            assert exact_outcome(p, p, (0, 0), st, wps, 0)["seg"] == k
    below_far, above_near = _up(hy - 2.5, -1), _up(hy + 2.5, -1)        # 2.5 + 1 ulp below, 2.5 - 1 ulp above
    assert hy - below_far > 2.5 and above_near - hy < 2.5
    for cnt, k1, k2 in pairs:
        for name, ye, yl, win in (("A", below_far, hy + 2.5, "later"), ("B", hy - 2.5, above_near, "later")):
            for order in ("listed", "swapped"):
                # E = the segment below the subject, L = the one above (run right to left, so that the
                # connection between neighbouring near segments is a vertical 10 m away)
                ke, kl = (k1, k2) if order == "listed" else (k2, k1)
                st, wps = path(cnt, {ke: (ye, False), kl: (yl, True)})
                B.add("xt_later", ("pair" + name, cnt, k1, k2, order), HOME, wps, start=st,
                      on=("xt", 2.5) if name == "A" else None)
                ex = exact_outcome(HOME, HOME, (0, 0), st, wps, 0)
                assert ex["seg"] == kl and ex["cross_in"], (name, order, ex["seg"])
                # every other segment is out of reach of a rounding error
                pts = [st] + wps
                for q in range(cnt):
                    assert q in (ke, kl) or _seg_d2(HOME, pts[q], pts[q + 1]) > 9, (cnt, k1, k2, q)


def _xt_random(B, rng):
    W = B.W
    B.plan(N_RANDOM)
    x0, x1, y0, y1 = 560.0, 598.0, 335.0, 359.0
    q8 = lambda v: round(v * 8.0) / 8.0
    for n in range(N_RANDOM):
        cnt = 1 + n % W if n < 4 * W else int(rng.integers(1, W + 1))
        pts = [(q8(rng.uniform(x0, x1)), q8(rng.uniform(y0, y1)))]
        step = (0.0, 0.0)
        for _ in range(cnt):
            r = rng.random()
            if r < 0.15:
                step = (0.0, 0.0)                               # a repeated vertex
            elif r > 0.4 or step == (0.0, 0.0):                 # else: the same step again, a collinear run
                step = (q8(rng.uniform(-12, 12)), q8(rng.uniform(-12, 12)))
            x, y = pts[-1][0] + step[0], pts[-1][1] + step[1]
            pts.append((min(max(x, x0), x1), min(max(y, y0), y1)))
        while True:
            k = int(rng.integers(cnt))
            t = int(rng.integers(0, 9)) / 8.0
            ang, rad = rng.uniform(0, 2 * math.pi), rng.uniform(0, 5.5)
            p = (q8(pts[k][0] + t * (pts[k + 1][0] - pts[k][0]) + rad * math.cos(ang)),
                 q8(pts[k][1] + t * (pts[k + 1][1] - pts[k][1]) + rad * math.sin(ang)))
            if geos.cross_track_distance(p[0], p[1], pts) < 6.0:
                break
        mask = 0
        if rng.random() < 0.5:
            for b in range(cnt):
                if rng.random() < 0.4:
                    mask |= 1 << b
            if mask == (1 << cnt) - 1:
                mask &= ~(1 << int(rng.integers(cnt)))
        vel = [(0.0, 0.0), (4.0, 0.0), (-2.0, 2.0), (0.0, -6.0), (1.5, 2.0)][int(rng.integers(5))]
        B.add("xt_random", n, p, pts[1:], start=pts[0], removed=[b for b in range(cnt) if (mask >> b) & 1], vel=vel,
              prove=False)


def _fix_kind(B):
    """A flagged radar ray in each reward branch (the reward is rebuilt from the exact radar minimum)."""
    far_goal = [(470.0, 262.0)]
    corners = []
    for ci, qi, r in CORNER_RAYS:
        x0, x1, y0, y1 = T.square_of(*T.CELLS[ci])
        q = ((x1, y0), (x0, y1), (x0, y0), (x1, y1))[qi]
        c = T._corner_start(q, r)
        assert c is not None, (ci, qi, r)
        corners.append(c)
    contacts = []
    for ci, qi, r in CONTACT_RAYS:
        x0, x1, y0, y1 = T.square_of(*T.CELLS[ci])
        c = _corner_start_at(((x1, y0), (x0, y1), (x0, y0), (x1, y1))[qi], r, 0.2)
        assert c is not None and T.exact_building(c, T.threshold_map()), (ci, qi, r)
        contacts.append(c)
    B.plan(len(T.CELLS) * 3 * (4 + 1 + 2) + 3 * 2 * len(corners) + 3 * len(contacts) + 3 * 4)
    for i, j in T.CELLS:
        x0, x1, y0, y1 = T.square_of(i, j)
        for u in (-1, 0, 1):
            for d in (3.0, 4.5):                        # thresholds.py edge_near: no crash
                B.add("fix_kind", ("none", d, u), (x0 - d, _up(y1, u)), far_goal, prove=False)
                B.add("fix_kind", ("none_b", d, u), (x0 - d, _up(y0, u)), far_goal, prove=False)
            # the 64-gon's vertex 0 on the corner (x0, y1), the 0-degree ray along the top edge
            B.add("fix_kind", ("building", u), (_up(x0 - PB, u), y1), far_goal, prove=False)
            for d in (3.0, 4.5):                        # the goal on the subject
                p = (x0 - d, _up(y1, u))
                B.add("fix_kind", ("goal", d, u), p, [p], prove=False)
    for c in corners:
        for u in (-1, 0, 1):
            p = (c[0], _up(c[1], u))
            B.add("fix_kind", ("corner", u), p, far_goal, prove=False)
            B.add("fix_kind", ("corner_goal", u), p, [p], prove=False)
    for c in contacts:
        for u in (-1, 0, 1):
            B.add("fix_kind", ("corner_building", u), (c[0], _up(c[1], u)), far_goal, prove=False)
    for u in (-1, 0, 1):
        B.add("fix_kind", ("bound", 0, u), (_up(BOUND[0] + PB, u), 300.0), far_goal, prove=False)
        B.add("fix_kind", ("bound", 1, u), (_up(BOUND[1] - PB, u), 320.0), far_goal, prove=False)
        B.add("fix_kind", ("bound", 2, u), (560.0, _up(BOUND[2] + PB, u)), far_goal, prove=False)
        B.add("fix_kind", ("bound", 3, u), (590.0, _up(BOUND[3] - PB, u)), far_goal, prove=False)


_CACHE = {}


def build(N, W):
    """The batch for N agents and waypoint lists of W slots: (families, variants, state dict).  The state
    dict holds the pre-step arrays ``KEYS`` plus ``subj`` (the subject's slot per env) and ``post`` (the
    post-step positions)."""
    if (N, W) not in _CACHE:
        assert N >= 2 and 4 <= W <= 32
        B = Batch(N, W)
        _wp_families(B)
        _xt_families(B)
        _fix_kind(B)
        _xt_random(B, np.random.default_rng(1000 * W + N))
        _CACHE[(N, W)] = B.arrays()
    fam, var, st = _CACHE[(N, W)]
    return list(fam), list(var), {k: v.copy() for k, v in st.items()}


def select(fam, var, st, families):
    """The sub-batch of the given families."""
    idx = [e for e, f in enumerate(fam) if f in families]
    return [fam[e] for e in idx], [var[e] for e in idx], {k: v[idx].copy() for k, v in st.items()}


def _i32(mask):
    return mask - (1 << 32) if mask >> 31 else mask


def fix_outcome(p, goal, occ):
    """``_fix_outcome`` (cached)."""
    return _fix_outcome(tuple(p), tuple(goal), occ.tobytes(), occ.shape)


@functools.lru_cache(maxsize=None)
def _fix_outcome(p, goal, occ_bytes, shape):
    """The reward branch and reward of a stationary fix_kind subject at p on its path's start (cross 0):
    bound > building > goal > none (WGRU/env:1940-2030), the penalty from the exact radar minimum."""
    occ = np.frombuffer(occ_bytes, np.uint8).reshape(shape)
    rmin = float(T.exact_radar(tuple(p), [], occ, 1).min())
    nbp = 3 * ((-1 / (5 - PB)) * rmin + 2) if PB <= rmin <= 5 else 0.0
    base = 3.0 + 0.0 - 3.0                # cross 0, no progress, the full small-step penalty
    if geos.bound_crash(p, p, BOUND):
        return "bound", base - 5 - nbp, base - nbp
    if T.exact_building(p, occ):
        return "building", base - 5 - nbp, base - nbp
    if T.exact_goal(p, goal):
        return "goal", 5.0, base - nbp
    return "none", base - nbp, base - 5 - nbp


def check(families, variants, pre, post, mask, reward, where=""):
    """Every non-random subject against the outcome its construction gives (``exact_outcome``;
    ``fix_outcome`` for fix_kind).  pre: the builder's state dict; post: pos, wp_cur, goal after the step;
    mask, reward: (E, N).  Where two outcomes differ in the reward, the observed reward must be nearer the
    expected branch's value than the other's.  Returns {family: set of outcomes}."""
    seen = {}
    occ = T.threshold_map()
    for e, fam in enumerate(families):
        if fam == "xt_random":
            continue
        s = int(pre["subj"][e])
        tag = (where, fam, variants[e], e)
        p = tuple(pre["post"][e, s])
        assert np.array_equal(post["pos"][e, s], p), tag
        cnt = int(pre["cnt"][e, s])
        wps = [tuple(w) for w in pre["wp"][e, s, :cnt]]
        m, r = int(mask[e, s]), float(reward[e, s])
        if fam == "fix_kind":
            kind, want, other = fix_outcome(p, wps[-1], occ)
            assert (bool(m & 1), bool(m & 8)) == (kind == "bound", kind == "building"), tag + (kind, m)
            assert bool(m & 4) == bool(T.exact_goal(p, wps[-1])), tag + (kind, m)
            assert abs(r - want) < abs(r - other) and abs(r - want) < 1e-4, tag + (kind, r, want, other)
            seen.setdefault(fam, set()).add(kind)
            continue
        old = int(pre["wp_cur"][e, s]) & 0xffffffff
        ex = exact_outcome(p, tuple(pre["pos"][e, s]), tuple(pre["vel"][e, s]), tuple(pre["start"][e, s]), wps, old)
        assert bool(m & 16) == ex["flag"], tag + (m, ex["flag"])
        assert m & 0b101111 == 0, tag + (m,)
        assert int(post["wp_cur"][e, s]) == _i32(ex["cur"]), tag + (int(post["wp_cur"][e, s]), ex["cur"], ex["pop"])
        assert np.array_equal(post["goal"][e, s], wps[ex["goal"]]), tag + (post["goal"][e, s].tolist(), ex["goal"])
        want = ex["reward"]
        assert abs(r - want) < 1e-4, tag + (r, want, ex)
        # the other branch: the bonus (wp5), the other tie candidate (wp_next_tie), cross on the other side
        cross = math.sqrt(float(ex["cross2"]))
        pp, vel = tuple(pre["pos"][e, s]), tuple(pre["vel"][e, s])
        if fam.startswith("wp5") or fam in ("wp_prefix", "wp_tie", "wp_index", "wp_final_pop"):
            other = want + (-3.0 if ex["bonus"] else 3.0)
            out = ex["flag"] if fam.startswith("wp5") else ex["pop"]
        elif fam == "wp_next_tie":
            nx = wps[ex["nxt"]]
            twin = (2 * p[0] - nx[0], 2 * p[1] - nx[1])
            other = _reward(p, pp, vel, twin, ex["bonus"], cross if ex["cross_in"] else None)
            assert abs(other - want) >= 0.1
            out = ex["nxt"]
        else:
            other = _reward(p, pp, vel, wps[ex["nxt"]], ex["bonus"], None if ex["cross_in"] else cross)
            out = ex["cross_in"]
        if abs(other - want) > 1e-3:
            assert abs(r - want) < abs(r - other), tag + (r, want, other)
        seen.setdefault(fam, set()).add(out)
    return seen


def both_ways(seen):
    """Both outcomes of every boolean threshold occurred; every fix-up kind occurred."""
    for f in BOOL_FAMILIES:
        assert seen.get(f) == {True, False}, (f, seen.get(f))
    assert seen["fix_kind"] == {"none", "building", "bound", "goal"}, seen["fix_kind"]
    for f in ("wp_prefix", "wp_tie", "wp_next_tie", "wp_index", "wp_final_pop", "xt_on_path"):
        assert seen.get(f), f


def oracle_state(co, st):
    """Install a batch's pre-step state in a c_oracle.BatchedOracle(variant="wgru")."""
    co.pos[:] = st["pos"]
    co.pre_pos[:] = st["pre_pos"]
    co.vel[:] = st["vel"]
    co.pre_vel[:] = st["vel"]
    co.goal[:] = st["goal"]
    co.wp[:] = st["wp"]
    co.wp_cnt[:] = st["cnt"]
    co.wp_cur[:] = st["wp_cur"]
    co.reach[:] = 0
    co.wall[:] = 0
    co.step_count[:] = 0
    co.start[:] = st["start"]


def scalar_env(st, e, occ):
    """oracle/wgru_env_ref.WgruEnv holding env e of the batch: the goal list = the remaining waypoints,
    ref_line = start + all waypoints (WGRU/env:339-343).  Returns (env, kept): kept[i] = the indices the
    goal list of agent i was made from."""
    from oracle import wgru_env_ref
    N = st["pos"].shape[1]
    env = wgru_env_ref.WgruEnv(N, occ)
    kept = []
    for i, ag in env.all_agents.items():
        cnt, m = int(st["cnt"][e, i]), int(st["wp_cur"][e, i]) & 0xffffffff
        ks = [k for k in range(cnt) if not (m >> k) & 1]
        kept.append(ks)
        ag.pos = st["pos"][e, i].copy()
        ag.pre_pos = st["pre_pos"][e, i].copy()
        ag.ini_pos = st["start"][e, i].copy()
        ag.vel = st["vel"][e, i].copy()
        ag.pre_vel = st["vel"][e, i].copy()
        ag.goal = [list(st["wp"][e, i, k]) for k in ks]
        ag.waypoints = [list(w) for w in st["wp"][e, i, :cnt]]
        ag.ref_line = [tuple(st["start"][e, i])] + [tuple(w) for w in st["wp"][e, i, :cnt]]
        ag.removed_goal, ag.reach_target, ag.collide_wall_count = None, False, 0
    return env, kept
