"""Plain-numpy restatement of the exploration maps (include/aac_visits.h): the bin rule of one axis by
``searchsorted`` on the edges, and the per-row rule of one accumulate call."""
import numpy as np

COUNTERS = 4      # samples, pos_outside, act_outside, reserved


def edges(lo, hi, G):
    """edge[k] = lo + k * ((hi - lo) / G) for k < G, edge[G] = hi, all in double."""
    lo, hi = np.float64(lo), np.float64(hi)
    w = (hi - lo) / np.float64(G)
    e = np.empty(G + 1, dtype=np.float64)
    for k in range(G):
        e[k] = lo + np.float64(k) * w
    e[G] = hi
    return e


def bins(v, e):
    """Bin index of every value of ``v`` over the edges ``e`` (v in bin k iff e[k] <= v < e[k + 1], the
    last bin closed), -1 for a value outside [e[0], e[-1]] or not finite."""
    v = np.asarray(v, dtype=np.float64)
    G = len(e) - 1
    with np.errstate(invalid="ignore"):
        inside = (v >= e[0]) & (v <= e[-1])          # False for NaN
    k = np.searchsorted(e, np.where(inside, v, e[0]), side="right") - 1
    k = np.minimum(k, G - 1)                         # v == hi: the last bin
    return np.where(inside, k, -1)


def hist2d(x, y, ex, ey):
    """(table [GX][GY], rows outside): a row with either coordinate outside is in no bin."""
    bx, by = bins(x, ex), bins(y, ey)
    ok = (bx >= 0) & (by >= 0)
    h = np.zeros((len(ex) - 1, len(ey) - 1), dtype=np.int64)
    np.add.at(h, (bx[ok], by[ok]), 1)
    return h, int((~ok).sum())


class VisitsRef:
    def __init__(self, n_maps, GX, GY, A, xr, yr, ar=(-1.0, 1.0)):
        self.n_maps, self.GX, self.GY, self.A = n_maps, GX, GY, A
        self.ex, self.ey, self.ea = edges(*xr, GX), edges(*yr, GY), edges(*ar, A)
        self.pos = np.zeros((2 * n_maps, GX, GY), dtype=np.int64)
        self.act = np.zeros((2, A, A), dtype=np.int64)
        self.cnt = np.zeros((2 * n_maps, COUNTERS), dtype=np.int64)

    def accumulate(self, pos, act, episode, explore_until, map_idx=None, sel=None):
        """pos float64 [E][N][2], act float32 / float64 [E][N][2], episode int32 [E]."""
        E, N = pos.shape[:2]
        mp = np.zeros(E, dtype=np.int64) if map_idx is None else np.asarray(map_idx, dtype=np.int64)
        on = np.ones(E, dtype=bool) if sel is None else np.asarray(sel) != 0
        bad = on & ((mp < 0) | (mp >= self.n_maps))
        self.cnt[0, 3] += int(bad.sum()) * N
        period = np.where(np.asarray(episode, dtype=np.int64) <= explore_until, 0, 1)
        a64 = np.asarray(act).astype(np.float64)      # a float widens exactly
        rows = np.repeat(on & ~bad, N)
        pl = np.repeat(2 * np.where(bad, 0, mp) + period, N)[rows]
        pr = np.repeat(period, N)[rows]
        np.add.at(self.cnt[:, 0], pl, 1)
        bx, by = bins(pos[..., 0].reshape(-1)[rows], self.ex), bins(pos[..., 1].reshape(-1)[rows], self.ey)
        ok = (bx >= 0) & (by >= 0)
        np.add.at(self.pos, (pl[ok], bx[ok], by[ok]), 1)
        np.add.at(self.cnt[:, 1], pl[~ok], 1)
        bu, bv = bins(a64[..., 0].reshape(-1)[rows], self.ea), bins(a64[..., 1].reshape(-1)[rows], self.ea)
        ok = (bu >= 0) & (bv >= 0)
        np.add.at(self.act, (pr[ok], bu[ok], bv[ok]), 1)
        np.add.at(self.cnt[:, 2], pl[~ok], 1)
