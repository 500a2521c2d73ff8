"""Exact-threshold states of the UAM environment (config 5; csrc/aac_uam.hip, oracle/uam_ref.py):
the counterpart of tests/thresholds.py.  Test infrastructure only, no GPU needed.

Each env of a batch puts one subject aircraft on one threshold of ss_reward_Mar_changeskin
(UAM/env:3892-4629), the go-around aircraft's target switch (UAM/util:41-51) or the radar
(UAM/env:1360-1486); sibling envs move one coordinate +-1 and +-2 ulp off it.  The subject is
stationary (zero velocity, zero action: the kinematics leave its position bit for bit) or moves by
dyadic amounts, so the post-step positions are exact; ``Batch.add`` verifies that with rationals
(``bound`` excepted: its capsule is built from the float pre / post positions on both sides).  The
other aircraft are parked on a grid, farther than the 5 m radar + pB from the subject and its
partners, away from the clouds, the runway and each other's near band.  The subject's index
alternates between 0 and N - 1 (the per-env walk that doubles the reward coefficients depends on the
order); ``near5`` alone keeps it at 0, because its only observable is the doubling it passes on.
Threshold coordinates stay in [4, 36] (``bound`` excepted), where the touching vertices lie within a
factor 2 of each other and the kernel's exact orientation test is decidable.

Families (strict: touching is no conflict):
  goal_apo / goal_vtx    64-gon(p, 0.5) against 64-gon(goal, 1), touching counts; the goal offset on an
                         apothem (edge index k) or on a vertex direction of the Minkowski 64-gon
  cloud_apo / cloud_vtx  against the cloud (r = 3, at its goal or drifting along an axis) and the go-around
                         aircraft (r = 1, flying an axis-parallel leg), strict
  rw_edge / rw_corner    the runway rectangle, strict: the four edges (extreme vertices 0 / 16 / 32 / 48)
                         and the four corners along edge-normal and vertex directions
  go_target              the go-around aircraft touching path[target].buffer(0.5); read from cloud_tgt
                         and the next cloud position
  bound                  the capsule band of test_bound_capsule_band_bit_exact for the lines 0 / 40,
                         r = 0.5: the capsule's extreme r u from a line, u in
                         [cos(pi/32) - 2e-3, 1 + 2e-3]; moving, axis-parallel and stationary aircraft
  contact                np.linalg.norm <= 1.0 (2 pB), each variant labelled with its own float norm;
                         one partner has finished (no collision)
  near2 / near5          the near-drone band's ends.  Only the nearest neighbour enters the UAM term,
                         which is 0 at 5 m: near5 is observed through the coefficient doubling (bearing
                         in [90, 180]) that the subject hands to a later aircraft with a 3 m neighbour
  bearing90 / bearing180 a colliding partner exactly below / left (bearing exactly 90 / 180), and off the
                         axis by BEARING_OFF = 2^-20 m at 0.75 m: 1.3e-6 rad = 7e-5 degrees, against
                         atan2 errors of a few ulp (1e-13 degrees) in glibc and ocml; the crash penalty
                         doubles inside [90, 180]
  tdcpa_d / tdcpa_t0 / tdcpa_t1 / tdcpa_zero
                         compute_t_cpa_d_cpa_potential_col (UAM/util:916-938): d < 1.0 at tcpa = 0, tcpa
                         on 0 and on 1, and zero relative velocity (tcpa = -10, d of the look-ahead)
  tangent                an axis ray through an aircraft's or a cloud's extreme vertex
  start_on               the subject on a partner's vertex 0
  rw_corner_ray          a ray through exactly one runway corner (the lattice construction of
                         tests/thresholds.py ``_corner_start``, length 5)
  rw_edge_run            the 0 / 180 degree ray along y = 10 / y = 30, from outside and from on the edge
  rw_graze               an axis ray an ulp beside an edge that passes the far corner (the edge parameter
                         rounds to exactly 1), and its mirror images

Expectations come from the reference's own semantics: exact rational predicates on the GEOS float
vertices where it asks GEOS (``U.gons_meet_exact``, ``U.gon_rect_overlap_exact``, ``geos.bound_crash``,
``geos.ray_square_boundary_t_exact``, ``geos._seg_seg_first_t_exact``; a radar value is the exact t
times the float ray length), float norms / atan2 where it compares floats."""
import functools
import math
from fractions import Fraction

import numpy as np

from oracle import geos
from oracle import uam_ref as U

PB = U.PB
ULPS = (-2, -1, 0, 1, 2)
BEARING_OFF = 2.0 ** -20
RADAR_FAMILIES = ("tangent", "start_on", "rw_corner_ray", "rw_edge_run", "rw_graze")
BOOL_FAMILIES = ("goal_apo", "goal_vtx", "cloud_apo", "cloud_vtx", "rw_edge", "rw_corner", "go_target", "bound",
                 "contact", "near2", "near5", "bearing90", "bearing180", "tdcpa_d", "tdcpa_t0", "tdcpa_t1",
                 "tdcpa_zero")
PREDICATE_FAMILIES = BOOL_FAMILIES[:8]

HOMES = ((9.25, 20.5), (28.75, 14.25), (13.5, 31.125), (30.5, 26.75))
# parking grid: clear of the runway's x range, spacings 5.4 / 5.05 (> the near band's 5 m end)
PARK = [(x, 2.3 + 5.05 * j) for x in (2.3, 7.7, 13.1, 26.9, 32.3, 37.7) for j in range(8)]
# cloud 0 (r = 3): (position, kind); the last two sit on their goals and do not move
CLOUD0 = (((8.0, 30.0), 0), ((30.0, 10.0), 1), ((10.0, 10.0), 0), ((35.0, 30.0), 1))
# go-around aircraft (r = 1) on axis-parallel legs of its loop: (kind, position, target index)
GO = ((0, (5.0, 22.5), 3), (0, (12.5, 35.0), 2), (0, (12.5, 5.0), 4),
      (2, (35.0, 22.5), 3), (2, (27.5, 35.0), 2), (2, (27.5, 5.0), 4))


def _up(x, n=1):
    for _ in range(abs(n)):
        x = float(np.nextafter(x, math.inf if n > 0 else -math.inf))
    return x


def _dist(a, b):
    return math.hypot(a[0] - b[0], a[1] - b[1])


def float_norm(a, b):
    """np.linalg.norm of a 2-vector difference, the reference's form (UAM/env:4001-4083)."""
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))


def ray_end(c, r, length=U.RADAR_DIST):
    """The radar segment's end as the kernel and the oracle compute it."""
    rad = math.radians(20 * r)
    return c[0] + length * math.cos(rad), c[1] + length * math.sin(rad)


def cloud_step(pos, target, speed):
    """calculate_next_position (UAM/util:300-318) for the cloud move of one step."""
    p = U.calculate_next_position(np.array(pos, dtype=float), np.array(target, dtype=float), speed, U.DT)
    return float(p[0]), float(p[1])


def _corner_start(q, r, length=U.RADAR_DIST):
    """A start c with the radar ray r passing EXACTLY through the point q at a parameter t near 1/2
    (tests/thresholds.py ``_corner_start`` for the UAM ray length)."""
    rad = math.radians(20 * r)
    dx, dy = length * math.cos(rad), length * math.sin(rad)
    c0 = (q[0] - dx / 2, q[1] - dy / 2)
    e0 = ray_end(c0, r, length)
    ddx, ddy = e0[0] - c0[0], e0[1] - c0[1]
    u = min(float(np.spacing(c0[0])), float(np.spacing(c0[1])))
    nx, ny = int(Fraction(ddx) / Fraction(u)), int(Fraction(ddy) / Fraction(u))
    g = math.gcd(abs(nx), abs(ny))
    if g < 2 or Fraction(ddx) != nx * Fraction(u) or Fraction(ddy) != ny * Fraction(u):
        return None
    m = g // 2
    cx, cy = q[0] - (m * (nx // g)) * u, q[1] - (m * (ny // g)) * u
    ex, ey = ray_end((cx, cy), r, length)
    C, E, Q = (Fraction(cx), Fraction(cy)), (Fraction(ex), Fraction(ey)), (Fraction(q[0]), Fraction(q[1]))
    if (E[0] - C[0]) * (Q[1] - C[1]) - (E[1] - C[1]) * (Q[0] - C[0]) != 0:
        return None
    t = (Q[0] - C[0]) / (E[0] - C[0]) if E[0] != C[0] else (Q[1] - C[1]) / (E[1] - C[1])
    return (cx, cy) if 0 < t < 1 else None


# ------------------------------------------------------------------ exact radar (rationals)
_BOUND_SEGS = (((0.0, 0.0), (0.0, 40.0)), ((40.0, 0.0), (40.0, 40.0)), ((0.0, 40.0), (40.0, 40.0)),
               ((0.0, 0.0), (40.0, 0.0)))          # UAM/env:594-598


@functools.lru_cache(maxsize=None)
def exact_radar(c, gons):
    """The 18 radar distances of an aircraft at c with every hit decided and located exactly: the
    runway boundary, the 4 bound segments and the boundaries of the 64-gons ``gons`` = ((x, y, r), ...);
    exact t times the float ray length."""
    C = geos._fr(c)
    out = []
    near = gons
    for r in range(U.N_RAYS):
        e = ray_end(c, r)
        L = geos.point_dist(e[0], e[1], c[0], c[1])
        E = geos._fr(e)
        D = (E[0] - C[0], E[1] - C[1])
        best = geos.ray_square_boundary_t_exact(c, e, *U.RUNWAY)
        for a, b in _BOUND_SEGS:
            if min(c[0], e[0], c[1], e[1]) > 1e-3 and max(c[0], e[0], c[1], e[1]) < 40.0 - 1e-3:
                break
            t = geos._seg_seg_first_t_exact(C, D, geos._fr(a), geos._fr(b))
            if t is not None and (best is None or t < best):
                best = t
        for px, py, rad in near:
            # the 64-gon lies inside its circle: a float segment farther than r + 1e-3 from the centre misses it
            wx, wy, fx, fy = px - c[0], py - c[1], e[0] - c[0], e[1] - c[1]
            tt = min(max((wx * fx + wy * fy) / (fx * fx + fy * fy), 0.0), 1.0)
            if math.hypot(tt * fx - wx, tt * fy - wy) > rad + 1e-3:
                continue
            ring = [geos._fr(v) for v in geos.circle_vertices(px, py, rad)]
            for k in range(len(ring)):
                t = geos._seg_seg_first_t_exact(C, D, ring[k], ring[(k + 1) % len(ring)])
                if t is not None and (best is None or t < best):
                    best = t
        out.append(L if best is None else float(best) * L)
    return tuple(out)


def _in_reach(c, gons):
    """The 64-gons the radar of an aircraft at c can reach (the others cannot change exact_radar)."""
    return tuple(g for g in gons if _dist(c, g) <= U.RADAR_DIST + g[2] + 1e-3)


def tdcpa_conflict(other_pos, host_pos, other_vel, host_vel):
    """One neighbour's contribution to the potential-conflict count (UAM/util:916-938), in the
    reference's float operations."""
    o, h = np.asarray(other_pos, dtype=float), np.asarray(host_pos, dtype=float)
    ov, hv = np.asarray(other_vel, dtype=float), np.asarray(host_vel, dtype=float)
    rel = -1 * (o - h)
    w = ov - hv
    sq = np.square(np.linalg.norm(w))
    if sq == 0:
        return int(np.linalg.norm((h + hv * 1) - (o + ov * 1)) < 2 * PB)
    t = np.dot(rel, w) / sq
    d = np.linalg.norm((rel * -1) + (w * t))
    return int(t <= 1 and t >= 0 and d < 2 * PB)


def bearing_in(h, o):
    b = U.calculate_bearing(h[0], h[1], o[0], o[1])
    return 90.0 <= b <= 180


# ------------------------------------------------------------------ batch
class Batch:
    """Envs of N aircraft with one subject each.  ``exp[e]`` holds what the reference's semantics give
    for env e: ``want`` (the family's boolean outcome), and the observables it shows in -- ``bit`` (a
    mask bit of the subject), ``reward`` (the subject's), ``conf`` (its conf_cur), ``cloud`` ((target,
    position) of the go-around aircraft), ``witness`` ((aircraft, near-drone coefficient)), ``radar``."""

    def __init__(self, N):
        self.N = N
        self.fam, self.var, self.subj, self.exp, self.rows = [], [], [], [], []

    def __len__(self):
        return len(self.fam)

    def add(self, family, variant, subject, partners=(), goal=None, vel=None, cloud0=None, go=None, exp=None,
            first=False, exact_move=True):
        """subject: pre-step position; partners: (position, velocity, reach) each; cloud0: (position, kind);
        go: (kind, position, target).  Unset clouds are put far from the subject."""
        N = self.N
        si = 0 if (first or len(self.fam) % 2 == 0) else N - 1
        idx = [si] + [(1 + k if si == 0 else N - 2 - k) for k in range(len(partners))]
        assert len(idx) <= N
        pos, v, reach = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(N, np.uint8)
        pos[si] = subject
        if vel is not None:
            v[si] = vel
        for i, (pp, pv, pr) in zip(idx[1:], partners):
            pos[i], v[i], reach[i] = pp, pv, pr
        post = pos + v * U.DT
        if exact_move:
            for i in idx:
                for a in range(2):
                    assert Fraction(float(post[i, a])) == Fraction(float(pos[i, a])) + Fraction(float(v[i, a])) / 2
        busy = [tuple(pos[i]) for i in idx] + [tuple(post[i]) for i in idx]
        far = lambda q: min(_dist(q, b) for b in busy)
        if cloud0 is None:
            cloud0 = max(CLOUD0, key=lambda c: far(c[0]))
            assert far(cloud0[0]) > U.RADAR_DIST + 3.0 + 1.0
        if go is None:
            go = max(GO, key=lambda g: far(g[1]))
            assert far(go[1]) > U.RADAR_DIST + 1.0 + 1.0 + 1.0
        spots = [q for q in PARK if far(q) > U.RADAR_DIST + PB + 1.0 and _dist(q, cloud0[0]) > 3.0 + PB + 2.0
                 and _dist(q, go[1]) > 1.0 + PB + 2.0]
        rest = [i for i in range(N) if i not in idx]
        assert len(spots) >= len(rest), (family, len(spots))
        for i, q in zip(rest, spots):
            pos[i] = q
        post = pos + v * U.DT
        goals = np.where(pos[:, :1] < 20.0, np.array([[38.0, 2.0]]), np.array([[2.0, 38.0]]))
        if goal is not None:
            goals[si] = goal
        assert all(_dist(goals[i], post[i]) > 3.0 for i in range(N) if not (i == si and goal is not None))
        # the two nearest neighbours before the step, as a reset leaves them (stable sort by np.linalg.norm)
        top2 = np.full((N, 2), 255, np.uint8)
        for i in range(N):
            order = sorted((j for j in range(N) if j != i), key=lambda j: float_norm(pos[i], pos[j]))
            top2[i, :len(order[:2])] = order[:2]
        self.rows.append(dict(pos=pos, vel=v, pre_pos=pos.copy(), pre_vel=v.copy(), goal=goals, start=pos.copy(),
                              heading=np.zeros(N), reach=reach, clouds=np.array([cloud0[0], go[1]], dtype=float),
                              cloud_kind=np.array([cloud0[1], go[0]], np.int32), cloud_tgt=np.int32(go[2]),
                              step=np.int32(0), top2=top2, post=post))
        self.fam.append(family)
        self.var.append(variant)
        self.subj.append(si)
        self.exp.append(dict(exp or {}))
        return len(self.fam) - 1

    def state(self):
        keys = ("pos", "vel", "pre_pos", "pre_vel", "goal", "start", "heading", "reach", "clouds", "cloud_kind",
                "cloud_tgt", "step", "top2")
        return {k: np.stack([r[k] for r in self.rows]) for k in keys}

    def clouds_after(self, e):
        """The two cloud positions after the step (the target switch cannot fire: the builder keeps the
        go-around aircraft off its target except in ``go_target``, whose expectation carries it)."""
        r = self.rows[e]
        k0, k1 = int(r["cloud_kind"][0]), int(r["cloud_kind"][1])
        c0 = cloud_step(r["clouds"][0], U.CLOUDS[k0][2:4], U.CLOUD_VEL[0])
        path = [(float(U.GO_AC[k1][i]), float(U.GO_AC[k1][i + 1])) for i in range(0, 12, 2)]
        c1 = cloud_step(r["clouds"][1], path[int(r["cloud_tgt"])], U.CLOUD_VEL[1])
        return c0, c1

    def radar_gons(self, e, clouds=None):
        """The 64-gons the subject's radar of env e can see (post-step), as exact_radar's argument."""
        r, si = self.rows[e], self.subj[e]
        c0, c1 = clouds if clouds is not None else self.clouds_after(e)
        g = [(float(p[0]), float(p[1]), PB) for i, p in enumerate(r["post"]) if i != si]
        return _in_reach(r["post"][si], g + [(c0[0], c0[1], 3.0), (c1[0], c1[1], 1.0)])


def _dir(ang):
    return math.cos(ang), math.sin(ang)


def _add_pair_thresholds(B, fam_apo, fam_vtx, centre, R, ks, strict, make):
    """Subject on the Minkowski 64-gon (circumradius R) around ``centre``: apothem direction k + 1/2 and
    vertex direction k, its x moved by the ulp variants.  make(subject) -> Batch.add keyword arguments."""
    for k in ks:
        for fam, ang, rad in ((fam_apo, (k + 0.5) * math.pi / 32, R * U.APO), (fam_vtx, k * math.pi / 32, R)):
            c, s = _dir(ang)
            px, py = centre[0] + rad * c, centre[1] + rad * s
            for u in ULPS:
                p = (_up(px, u), py)
                kw = make(p)
                other, r1 = kw.pop("_other")
                want = U.gons_meet_exact(p, PB, other, r1, strict)
                kw["exp"] = dict(want=want, bit=kw.pop("_bit"))
                B.add(fam, u, p, **kw)


@functools.lru_cache(maxsize=None)
def build(N, seed=0):
    """The threshold batch for N aircraft (N >= 3)."""
    assert N >= 3
    rng = np.random.default_rng(seed)
    B = Batch(N)

    # ---- goal: 64-gon(p, 0.5) vs 64-gon(goal, 1), touching counts (mask bit 3)
    for h, ks in zip(HOMES, ((3,), (30,), (50,), (16,))):
        _add_pair_thresholds(B, "goal_apo", "goal_vtx", h, PB + U.GOAL_R, ks, False,
                             lambda p, h=h: dict(goal=h, _other=(h, U.GOAL_R), _bit=8))
    # ---- clouds, strict (mask bit 1): cloud 0 on its goal / drifting down an axis, the go-around aircraft
    # on an axis-parallel leg; directions that keep the contact point inside [4, 36]
    for (cpos, kind), ks in ((((10.0, 10.0), 0), (2,)), (((35.0, 30.0), 1), (29,)),
                             (((10.0, 14.0), 0), (52,))):
        after = cloud_step(cpos, U.CLOUDS[kind][2:4], U.CLOUD_VEL[0])
        _add_pair_thresholds(B, "cloud_apo", "cloud_vtx", after, PB + 3.0, ks, True,
                             lambda p, c=(cpos, kind), a=after: dict(cloud0=c, _other=(a, 3.0), _bit=2))
    for go, ks in (((0, (5.0, 22.5), 3), (12,)), ((0, (12.5, 35.0), 2), (45,))):
        path = [(float(U.GO_AC[go[0]][i]), float(U.GO_AC[go[0]][i + 1])) for i in range(0, 12, 2)]
        after = cloud_step(go[1], path[go[2]], U.CLOUD_VEL[1])
        _add_pair_thresholds(B, "cloud_apo", "cloud_vtx", after, PB + 1.0, ks, True,
                             lambda p, g=go, a=after: dict(go=g, _other=(a, 1.0), _bit=2))
    # ---- runway edges (extreme vertices) and corners, strict (mask bit 1)
    x0, x1, y0, y1 = U.RUNWAY
    for u in ULPS:
        for y in (12.25,):
            for p in ((_up(x0 - PB, u), y), (_up(x1 + PB, u), y)):
                B.add("rw_edge", u, p, exp=dict(want=U.gon_rect_overlap_exact(p, PB, U.RUNWAY), bit=2))
        for x in (21.25,):
            for p in ((x, _up(y0 - PB, u)), (x, _up(y1 + PB, u))):
                B.add("rw_edge", u, p, exp=dict(want=U.gon_rect_overlap_exact(p, PB, U.RUNWAY), bit=2))
    for (qx, qy), k0 in (((x1, y1), 0), ((x0, y1), 16), ((x0, y0), 32), ((x1, y0), 48)):
        dirs = [((k0 + dk + 0.5) * math.pi / 32, PB * U.APO) for dk in ((0, 11) if k0 % 32 else (6, 15))]
        dirs += [((k0 + dk) * math.pi / 32, PB) for dk in ((4,) if k0 % 32 else ())]
        for ang, rad in dirs:
            c, s = _dir(ang)
            for u in ULPS:
                p = (_up(qx + rad * c, u), qy + rad * s)
                B.add("rw_corner", u, p, exp=dict(want=U.gon_rect_overlap_exact(p, PB, U.RUNWAY), bit=2))
    # ---- the go-around aircraft touching its target's 0.5 buffer (touching counts)
    for kind, t, ks in ((0, 2, (50,)), (0, 3, (13,)), (0, 1, (40,)), (2, 3, (29,))):
        path = [(float(U.GO_AC[kind][i]), float(U.GO_AC[kind][i + 1])) for i in range(0, 12, 2)]
        for k in ks:
            for ang, rad in (((k + 0.5) * math.pi / 32, 1.5 * U.APO), (k * math.pi / 32, 1.5)):
                c, s = _dir(ang)
                for u in ULPS:
                    g = (_up(path[t][0] + rad * c, u), path[t][1] + rad * s)
                    want = U.gons_meet_exact(g, 1.0, path[t], 0.5, False)
                    t2 = (U.preset_target_index(path, t) + 1) % len(path) if want else t
                    B.add("go_target", u, HOMES[0] if g[0] > 20 else HOMES[1], go=(kind, g, t),
                          exp=dict(want=want, cloud=(t2, cloud_step(g, path[t2], U.CLOUD_VEL[1]))))
    # ---- bound capsule band (mask bit 0)
    q = 0
    for line in range(4):
        for kind in range(4):           # free move, move along x, along y, stationary
            for _ in range(2):
                u = rng.uniform(math.cos(math.pi / 32) - 2e-3, 1 + 2e-3)
                v = rng.uniform(-0.7, 0.7, 2)
                if kind == 1:
                    v[1] = 0.0
                elif kind == 2:
                    v[0] = 0.0
                elif kind == 3:
                    v[:] = 0.0
                ax = line >> 1
                step = 0.5 * v
                p = [0.0, 0.0]
                p[1 - ax] = (12.0, 28.0, 9.0, 31.0)[q % 4] + rng.uniform(-1, 1)
                q += 1
                if line % 2 == 0:
                    p[ax] = U.BOUND[line] + PB * u - min(0.0, step[ax])
                else:
                    p[ax] = U.BOUND[line] - PB * u - max(0.0, step[ax])
                post = (p[0] + v[0] * U.DT, p[1] + v[1] * U.DT)
                B.add("bound", kind, tuple(p), vel=tuple(v), exact_move=False,
                      exp=dict(want=bool(geos.bound_crash(p, post, U.BOUND, PB)), bit=1))
    # ---- float-compare thresholds
    hx, hy = HOMES[0]
    for k, (ox, oy) in enumerate(((0.6, 0.8), (-0.8, 0.6), (1.0, 0.0), (0.0, -1.0))):
        for u in ULPS:
            done = (k == 1)
            pp = (_up(hx + ox, u), hy + oy)
            want = float_norm((hx, hy), pp) <= 2 * PB
            B.add("contact", u, (hx, hy), partners=[(pp, (0, 0), int(done))],
                  exp=dict(want=want, bit=4, bit_want=want and not done))
    hx, hy = HOMES[1]
    c_d, m_d = 1 + (U.NEAR_LO / (U.NEAR_HI - U.NEAR_LO)), (0 - 1) / (U.NEAR_HI - U.NEAR_LO)
    for ox, oy in ((-1.2, 1.6), (-1.6, 1.2)):   # partner up-left: neither side's bearing doubles
        for u in ULPS:
            pp = (_up(hx + ox, u), hy + oy)
            d = float_norm((hx, hy), pp)
            want = U.NEAR_LO <= d <= U.NEAR_HI
            B.add("near2", u, (hx, hy), partners=[(pp, (0, 0), 0)],
                  exp=dict(want=want, near=(U.NEAR_DRONE_COEF * (m_d * d + c_d)) if want else 0.0))
    hx, hy = HOMES[3]
    for ox, oy in ((-3.0, -4.0), (-4.0, -3.0)):  # partner down-left: the subject's bearing is in [90, 180]
        for u in ULPS:
            pp = (_up(hx + ox, u), hy + oy)
            w = (pp[0] - 2.4, pp[1] + 1.8)       # the witness: 3 m up-left of the partner (no doubling of its own)
            want = U.NEAR_LO <= float_norm((hx, hy), pp) <= U.NEAR_HI
            assert bearing_in((hx, hy), pp) and not bearing_in(pp, w) and not bearing_in(w, pp)
            assert _dist(w, (hx, hy)) > U.RADAR_DIST + PB + 0.25
            d = float_norm(w, pp)
            B.add("near5", u, (hx, hy), partners=[(pp, (0, 0), 0), (w, (0, 0), 0)], first=True,
                  exp=dict(want=want, witness=(2, (4.0 if want else 2.0) * (m_d * d + c_d))))
    hx, hy = HOMES[2]
    for fam, offs in (("bearing90", ((0.0, -0.75), (BEARING_OFF, -0.75), (-BEARING_OFF, -0.75))),
                      ("bearing180", ((-0.75, 0.0), (-0.75, BEARING_OFF), (-0.75, -BEARING_OFF)))):
        for ox, oy in offs:
            pp = (hx + ox, hy + oy)
            want = bearing_in((hx, hy), pp)
            assert not bearing_in(pp, (hx, hy))
            for rep in range(2):                 # the subject first and last in the walk
                B.add(fam, rep, (hx, hy), partners=[(pp, (0, 0), 0)],
                      exp=dict(want=want, reward=-(U.CRASH * 2 if want else U.CRASH)))
    hx, hy = HOMES[3]
    td = []
    for u in ULPS:      # post-step offsets: (1 +- ulps, 0) with tcpa = 0; tcpa = +-2 ulps; tcpa = 1 +- ulps
        td.append(("tdcpa_d", u, (_up(hx + 1.0, u), hy + 0.25), (0.0, 0.25), (0.0, -0.25)))
        td.append(("tdcpa_t0", u, (hx + 0.75, _up(hy + 0.25, u)), (0.0, 0.25), (0.0, -0.25)))
        td.append(("tdcpa_t1", u, (_up(hx + 0.75, u), hy), (0.25, 0.0), (-0.25, 0.0)))
        td.append(("tdcpa_zero", u, (_up(hx + 0.6, u), hy + 0.8), (0.25, -0.125), (0.25, -0.125)))
        td.append(("tdcpa_zero", u, (_up(hx + 1.0, u), hy), (-0.125, 0.25), (-0.125, 0.25)))
    for fam, u, pp, hv, ov in td:
        hp = (hx + hv[0] * U.DT, hy + hv[1] * U.DT)
        op = (pp[0] + ov[0] * U.DT, pp[1] + ov[1] * U.DT)
        c = tdcpa_conflict(op, hp, ov, hv)
        B.add(fam, u, (hx, hy), vel=hv, partners=[(pp, ov, 0)], exp=dict(want=bool(c), conf=c))
    # ---- radar
    hx, hy = HOMES[0]
    for d in (1.75, 3.5):
        for side in (1, -1):
            for u in (-1, 0, 1):
                B.add("tangent", u, (hx, hy), partners=[((hx + d, _up(hy + side * PB, u)), (0, 0), 0)], exp=dict(ray=0))
                B.add("tangent", u, (hx, hy), partners=[((hx - d, _up(hy + side * PB, u)), (0, 0), 0)], exp=dict(ray=9))
    for u in (-1, 0, 1):
        B.add("tangent", u, (6.0, _up(13.0, u)), cloud0=((10.0, 10.0), 0), exp=dict(ray=0))     # the cloud's top vertex
        B.add("tangent", u, (13.5, _up(7.0, u)), cloud0=((10.0, 10.0), 0), exp=dict(ray=9))     # its bottom vertex
        B.add("tangent", u, (8.0, _up(22.5, u)), go=(0, (5.0, 22.5), 3), exp=dict(ray=9))       # go-around at (5, 21.5): top
        B.add("start_on", u, HOMES[1], partners=[((_up(HOMES[1][0] - PB, u), HOMES[1][1]), (0, 0), 0)])
    for q, rays in (((x1, y0), (1, 2, 3, 4, 10, 11, 12, 13)), ((x0, y1), (1, 2, 3, 4, 10, 11, 12, 13)),
                    ((x0, y0), (5, 6, 7, 8, 14, 15, 16, 17)), ((x1, y1), (5, 6, 7, 8, 14, 15, 16, 17))):
        for r in rays:
            c = _corner_start(q, r)
            if c is not None:
                for u in (-1, 0, 1):
                    B.add("rw_corner_ray", u, (c[0], _up(c[1], u)), exp=dict(ray=r))
    for u in (-1, 0, 1):
        B.add("rw_edge_run", u, (x0 - 2.5, _up(y0, u)))         # 0 degrees along y = 10 from outside
        B.add("rw_edge_run", u, (x1 + 1.5, _up(y1, u)))         # 180 degrees along y = 30
        B.add("rw_edge_run", u, (x0 + 1.0, _up(y0, u)))         # from on the edge
        B.add("rw_edge_run", u, (x1 - 0.5, _up(y1, u)))
    for u in (-2, -1, 1, 2):
        for cx in (17.25, 17.4):
            B.add("rw_graze", u, (cx, _up(y0, u)), exp=dict(ray=0))              # 0 degrees past (22, 10)
            B.add("rw_graze", u, (cx, _up(y1, u)), exp=dict(ray=0))
            B.add("rw_graze", u, (40.0 - cx, _up(y0, u)), exp=dict(ray=9))       # 180 degrees past (18, 10) / (18, 30)
            B.add("rw_graze", u, (40.0 - cx, _up(y1, u)), exp=dict(ray=9))
        for cy in (7.5,):                                       # 90 degrees beside x = 18 / x = 22
            B.add("rw_graze", u, (_up(x0, u), cy))
            B.add("rw_graze", u, (_up(x1, u), cy))
        for cy in (32.75,):                                     # 270 degrees
            B.add("rw_graze", u, (_up(x0, u), cy))
            B.add("rw_graze", u, (_up(x1, u), cy))
    for e, f in enumerate(B.fam):
        if f in RADAR_FAMILIES:
            c = B.rows[e]["post"][B.subj[e]]
            B.exp[e]["radar"] = np.array(exact_radar((float(c[0]), float(c[1])), B.radar_gons(e)))
    return B


def reset_radar(B, e):
    """The subject's exact radar when env e's positions serve as an episode start (aac_uam_reset): the
    clouds sit on their start points, the go-around aircraft on (20, 20)."""
    r, si = B.rows[e], B.subj[e]
    c0 = U.CLOUDS[int(r["cloud_kind"][0])][:2]
    c = r["pos"][si]
    g = [(float(p[0]), float(p[1]), PB) for i, p in enumerate(r["pos"]) if i != si]
    g += [(float(c0[0]), float(c0[1]), 3.0), (20.0, 20.0, 1.0)]
    return np.array(exact_radar((float(c[0]), float(c[1])), _in_reach(c, g)))


# ------------------------------------------------------------------ checking
RTOL_FLOAT = 1e-9       # the float bar of tests/test_uam_gpu.py


def check(B, out, envs=None, where=""):
    """The subject rows of ``out`` against the expectations.  out: dict of numpy arrays -- mask [E, N],
    reward [E, N], radar [E, N, 18], conf_cur [E, N], cloud_tgt [E], clouds [E, 2, 2] (post-step).
    Returns ({family: set of outcomes}, {family: envs compared})."""
    seen, count = {}, {}
    for e in (range(len(B)) if envs is None else envs):
        f, si, x = B.fam[e], B.subj[e], B.exp[e]
        tag = (where, f, B.var[e], e)
        m = int(out["mask"][e, si])
        if "bit" in x:
            assert bool(m & x["bit"]) == x.get("bit_want", x["want"]), (tag, m, x)
        if "cloud" in x:
            t2, p2 = x["cloud"]
            assert int(out["cloud_tgt"][e]) == t2, (tag, int(out["cloud_tgt"][e]), t2)
            np.testing.assert_allclose(out["clouds"][e, 1], p2, rtol=0, atol=1e-12, err_msg=str(tag))
        if "reward" in x:
            assert abs(float(out["reward"][e, si]) - x["reward"]) <= RTOL_FLOAT, (tag, out["reward"][e, si], x)
        if "conf" in x:
            assert int(out["conf_cur"][e, si]) == x["conf"], (tag, int(out["conf_cur"][e, si]), x)
        for key, who in (("near", si), ("witness", None)):
            if key in x:
                i, nd = (who, x[key]) if key == "near" else x[key]
                # a stationary aircraft on its start: dist_to_goal = 0; the near-building penalty from
                # its own radar minimum (UAM/env:4466-4481)
                mn = float(out["radar"][e, i].min())
                nb = U.NEAR_BUILDING_COEF * (((0 - 1) / (U.TURNING_PT - PB)) * mn + 2) if PB <= mn <= U.TURNING_PT else 0
                assert abs(float(out["reward"][e, i]) - (0.0 - nb - nd)) <= RTOL_FLOAT, (tag, out["reward"][e, i], nb, nd)
        if "radar" in x:
            np.testing.assert_allclose(out["radar"][e, si], x["radar"], rtol=0, atol=RTOL_FLOAT, err_msg=str(tag))
        if "want" in x:
            seen.setdefault(f, set()).add(bool(x["want"]))
        count[f] = count.get(f, 0) + 1
    return seen, count


def both_ways(seen, families=BOOL_FAMILIES):
    for f in families:
        assert seen.get(f) == {True, False}, (f, seen.get(f))


def one_per_family(B):
    out, got = [], set()
    for e, f in enumerate(B.fam):
        if f not in got:
            got.add(f)
            out.append(e)
    return out
