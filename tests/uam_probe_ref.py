"""Test-side restatement of the UAM radar probe (include/aac_uam_probe.h): ``UAMEnv.radar``
(oracle/uam_ref.py:488-515) ray by ray, keeping beside each ray's minimum the candidate that gave it, the
point its distance was formed from, and the runner-up distance.  Test infrastructure only, no GPU needed.

The oracle's ``_seg_hits`` / ``_seg_seg`` / ``_seg_gon`` return distances only; ``seg_hits_pt`` /
``seg_seg_pt`` / ``seg_gon_pt`` below are the same statements with the point returned too
(tests/test_uam_probe_cpu.py holds ``dist`` to ``UAMEnv.radar`` bit for bit).  Candidates are tested in the
reference's order -- runway, the four bound segments in the order of ``UAMEnv.boundaries``, the two clouds,
the other aircraft by index -- each on a strict ``<`` against the running minimum (UAM/env:1385-1486)."""
import functools
import math

import numpy as np

from oracle import geos
from oracle import uam_ref as U

BATCHES = ((20, 3, 0), (20, 5, 0), (10, 16, 0))      # (E, N, seed) of tests/uam_rewardmap_ref.random_batch
NONE, RUNWAY, BOUND, CLOUD, AIRCRAFT = range(5)
KINDS = ("none", "runway", "bound", "cloud", "aircraft")
N_RAYS = 18


def seg_hits_pt(c, e, ring):
    """``U._seg_hits`` with the point: (distance, (x, y)) of the nearest intersection, or None."""
    best = None
    dx, dy = e[0] - c[0], e[1] - c[1]
    n = len(ring)
    BT = geos.BAND_T
    for k in range(n):
        v, w = ring[k], ring[(k + 1) % n]
        ex, ey = w[0] - v[0], w[1] - v[1]
        den = dx * ey - dy * ex
        qx, qy = v[0] - c[0], v[1] - c[1]
        if den == 0.0:
            band = True
        else:
            t = (qx * ey - qy * ex) / den
            s = (qx * dy - qy * dx) / den
            if not (-BT <= t <= 1.0 + BT and -BT <= s <= 1.0 + BT):
                continue
            band = min(abs(t), abs(t - 1.0), abs(s), abs(s - 1.0)) <= BT
        if band:
            C, V, W = geos._fr(c), geos._fr(v), geos._fr(w)
            E = geos._fr(e)
            tx = geos._seg_seg_first_t_exact(C, (E[0] - C[0], E[1] - C[1]), V, W)
            if tx is None:
                continue
            t = float(tx)
        p = (c[0] + t * dx, c[1] + t * dy)
        d = geos.point_dist(p[0], p[1], c[0], c[1])
        if best is None or d < best[0]:
            best = (d, p)
    return best


def seg_gon_pt(c, e, p, r):
    """``U._seg_gon`` with the point."""
    dx, dy = e[0] - c[0], e[1] - c[1]
    wx, wy = p[0] - c[0], p[1] - c[1]
    tt = (wx * dx + wy * dy) / (dx * dx + dy * dy)
    tt = min(max(tt, 0.0), 1.0)
    qx, qy = tt * dx - wx, tt * dy - wy
    if qx * qx + qy * qy > (r + 1e-6) ** 2:
        return None
    return seg_hits_pt(c, e, U._gon(p, r))


def seg_seg_pt(c, e, a, b):
    """``U._seg_seg`` with the point."""
    dx, dy = e[0] - c[0], e[1] - c[1]
    ex, ey = b[0] - a[0], b[1] - a[1]
    den = dx * ey - dy * ex
    if den == 0.0:
        return None
    qx, qy = a[0] - c[0], a[1] - c[1]
    t = (qx * ey - qy * ex) / den
    s = (qx * dy - qy * dx) / den
    if 0.0 <= t <= 1.0 and 0.0 <= s <= 1.0:
        p = (c[0] + t * dx, c[1] + t * dy)
        return geos.point_dist(p[0], p[1], c[0], c[1]), p
    return None


def select(length, end, cands):
    """The selection rule on one ray: ``cands`` is the list of (kind, id, hit) in test order, hit None or
    (distance, point).  Each hit replaces the record on a strict ``<`` against the running minimum, which
    starts at the ray's own length (NONE, id -1, the ray end).  Returns (dist, kind, id, point, runner_up):
    runner_up the smallest distance among the candidates that are not the record's (the ray length
    included; inf if there is none)."""
    best, kind, idx, point = length, NONE, -1, end
    for k, i, hit in cands:
        if hit is not None and hit[0] < best:
            best, kind, idx, point = hit[0], k, i, hit[1]
    others = [hit[0] for k, i, hit in cands if hit is not None and (k, i) != (kind, idx)]
    if kind != NONE:
        others.append(length)
    return best, kind, idx, point, (min(others) if others else math.inf)


def probe_agent(env, i):
    """The 18 records of aircraft i of a ``UAMEnv``: dict of dist [18], kind [18], id [18], point [18][2],
    end [18][2], runner_up [18]."""
    ag = env.all_agents[i]
    c = (float(ag.pos[0]), float(ag.pos[1]))
    out = dict(dist=[], kind=[], id=[], point=[], end=[], runner_up=[])
    for deg in range(0, 360, 20):
        e = (c[0] + U.RADAR_DIST * math.cos(math.radians(deg)), c[1] + U.RADAR_DIST * math.sin(math.radians(deg)))
        cands = [(RUNWAY, 0, seg_hits_pt(c, e, env.runway_ring))]
        cands += [(BOUND, k, seg_seg_pt(c, e, a, b)) for k, (a, b) in enumerate(env.boundaries)]
        cands += [(CLOUD, k, seg_gon_pt(c, e, cl.pos, cl.radius)) for k, cl in enumerate(env.clouds)]
        cands += [(AIRCRAFT, j, seg_gon_pt(c, e, other.pos, ag.protectiveBound))
                  for j, other in env.all_agents.items() if j != i]
        d, kind, idx, point, ru = select(geos.point_dist(e[0], e[1], c[0], c[1]), e, cands)
        for k, v in zip(("dist", "kind", "id", "point", "end", "runner_up"), (d, kind, idx, point, e, ru)):
            out[k].append(v)
    return {k: np.array(v, dtype={"kind": np.uint8, "id": np.int32}.get(k, np.float64)) for k, v in out.items()}


def probe_state(state, N):
    """Every env of a state dict: dist / kind / id / runner_up [E][N][18], point / end [E][N][18][2]."""
    E = state["pos"].shape[0]
    rows = []
    for e in range(E):
        env = U.env_from_state(state, e, N)
        per = [probe_agent(env, i) for i in range(N)]
        rows.append({k: np.stack([p[k] for p in per]) for k in per[0]})
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


@functools.lru_cache(maxsize=None)
def reference(E, N, seed):
    """(state, records) of ``tests.uam_rewardmap_ref.random_batch(E, N, seed)``'s pre-step state: computed
    once, shared by the CPU and the GPU tests, read-only."""
    from tests import uam_rewardmap_ref as M
    st, _ = M.random_batch(E, N, seed)
    ref = probe_state(st, N)
    for v in ref.values():
        v.setflags(write=False)
    return st, ref
