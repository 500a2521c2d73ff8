"""Scalar restatement of the radar probe (include/aac_probe.h) from oracle/geos.py's radar functions: the
per-candidate distances of one ray, the candidate and tie rules, the hit point and the ray end.  Test
infrastructure only (no GPU).

Candidates of ray r of agent i (position p, end = p + 15 (cos, sin), len = |end - p|):
  (1, j)            drone j != i whose 64-gon ``geos.ray_polygon_entry`` enters, at the GEOS distance of
                    the entry point                                                   (modes 0, 2)
  (2, ci * gh + cj) occupied cell with ``geos.ray_square_crossing`` d <= len           (modes 1, 2)
  (3, k)            bound line k (x-min, x-max, y-min, y-max) crossed at d < len       (modes 1, 2)
D is the radar value as ``ScalarEnv.radar`` forms it; among the candidates with d == D bit for bit the lowest
(kind, id) is the record, none (kind 0, id -1, point = end) if no candidate attains D.
"""
import math

import numpy as np

from oracle import geos
from oracle.consts import BOUND, PB
from tests import thresholds as T

NONE, DRONE, CELL, BOUND_K = 0, 1, 2, 3
CLOSE = 1e-9        # the two best candidates this close: the record's kind / id / point may go either way


def candidates(pos, i, r, occ, mode, bound=BOUND):
    """(c, e, L, [(d, kind, id, point)]) with every hit of the ray, a candidate or not (``eligible``)."""
    c = (float(pos[i][0]), float(pos[i][1]))
    e = T.ray_end(c, r)
    L = geos.point_dist(e[0], e[1], c[0], c[1])
    out = []
    if mode != 1:
        for j in range(len(pos)):
            if j == i:
                continue
            t = geos.ray_polygon_entry(c[0], c[1], e[0], e[1], geos.circle_vertices(float(pos[j][0]), float(pos[j][1]), PB))
            if t is None:
                continue
            px, py = c[0] + t * (e[0] - c[0]), c[1] + t * (e[1] - c[1])
            out.append((geos.point_dist(px, py, c[0], c[1]), DRONE, j, (px, py)))
    if mode != 0:
        gw, gh = occ.shape
        gx0, gy0 = math.ceil(bound[0] / 10.0) * 10.0, math.ceil(bound[2] / 10.0) * 10.0
        i0, i1 = int(math.floor((min(c[0], e[0]) - 5.0 - gx0) / 10.0)) - 1, int(math.ceil((max(c[0], e[0]) + 5.0 - gx0) / 10.0)) + 1
        j0, j1 = int(math.floor((min(c[1], e[1]) - 5.0 - gy0) / 10.0)) - 1, int(math.ceil((max(c[1], e[1]) + 5.0 - gy0) / 10.0)) + 1
        for ci in range(max(i0, 0), min(i1, gw - 1) + 1):
            for cj in range(max(j0, 0), min(j1, gh - 1) + 1):
                if not occ[ci, cj]:
                    continue
                qx, qy = gx0 + 10.0 * ci, gy0 + 10.0 * cj
                d = geos.ray_square_crossing(c[0], c[1], e[0], e[1], qx - 5.0, qx + 5.0, qy - 5.0, qy + 5.0)
                if d is not None:
                    out.append((d, CELL, ci * gh + cj, None))
        for k in range(4):
            v = float(bound[k])
            if k < 2:
                d = geos.ray_vline_crossing(c[0], c[1], e[0], e[1], v)
                pt = None if d is None or d == 0.0 else (v, c[1] + ((v - c[0]) / (e[0] - c[0])) * (e[1] - c[1]))
            else:
                d = geos.ray_hline_crossing(c[0], c[1], e[0], e[1], v)
                pt = None if d is None or d == 0.0 else (c[0] + ((v - c[1]) / (e[1] - c[1])) * (e[0] - c[0]), v)
            if d is not None:
                out.append((d, BOUND_K, k, pt))
    return c, e, L, out


def eligible(cand, L):
    d, kind = cand[0], cand[1]
    return kind == DRONE or (kind == CELL and d <= L) or (kind == BOUND_K and d < L)


def probe_ray(pos, i, r, occ, mode, bound=BOUND):
    """The record of one ray: dict(dist, kind, id, point, end, close).  ``close``: the ray's two best
    candidates lie within CLOSE of each other, so kind / id / point are not determined to the parity bar."""
    c, e, L, hits = candidates(pos, i, r, occ, mode, bound)
    cands = [h for h in hits if eligible(h, L)]
    dd = min([h[0] for h in cands if h[1] == DRONE], default=L)
    do = min([h[0] for h in cands if h[1] != DRONE], default=L)
    D = dd if mode == 0 else (do if mode == 1 else (dd if dd < do else do))
    att = sorted((h[1], h[2], k) for k, h in enumerate(cands) if h[0] == D)
    ds = sorted(h[0] for h in cands)
    close = len(ds) >= 2 and ds[1] - ds[0] <= CLOSE
    if not att:
        return dict(dist=D, kind=NONE, id=-1, point=e, end=e, close=close)
    d, kind, idx, pt = cands[att[0][2]]
    if pt is None:                      # the point at distance d along the ray
        pt = (c[0] + (d / L) * (e[0] - c[0]), c[1] + (d / L) * (e[1] - c[1])) if d > 0.0 else c
    return dict(dist=D, kind=kind, id=idx, point=pt, end=e, close=close)


def probe_rows(pos, occ, mode, map_idx=None, bound=BOUND):
    """``probe_ray`` over rows [M][N][2] -> arrays dist / point / end / kind / id / close [M][N][18]..."""
    pos = np.asarray(pos, dtype=np.float64)
    occ = np.asarray(occ)
    M, N = pos.shape[:2]
    out = dict(dist=np.zeros((M, N, 18)), point=np.zeros((M, N, 18, 2)), end=np.zeros((M, N, 18, 2)),
               kind=np.zeros((M, N, 18), np.uint8), id=np.zeros((M, N, 18), np.int32), close=np.zeros((M, N, 18), bool))
    for m in range(M):
        o = occ if occ.ndim == 2 else occ[0 if map_idx is None else int(map_idx[m])]
        for i in range(N):
            for r in range(18):
                rec = probe_ray(pos[m], i, r, o, mode, bound)
                for k in out:
                    out[k][m, i, r] = rec[k]
    return out
