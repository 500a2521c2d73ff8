"""Plain-numpy restatement of the flight recorder (include/aac_record.h): the two phases, one track at
a time, and the separation arithmetic with separate ``*`` and ``+`` and ``np.sqrt``.  The GPU tests
compare against it: every copied field, index, header and summary integer and ``ret`` bit-exact,
the square roots within 1 ulp.

``RecordRef`` fills its arrays with a byte pattern first, so a device recording that started from the
same pattern can be compared over whole arrays: rows that were never written must still hold it."""
import numpy as np

from multi_agent_aac_amd.record import EPISODE, TRACK_FIELDS, Trajectories, row_fields

ROOTS = ("nearest", "min_sep")          # row fields that hold a square root (1-ulp fields)


def separation(pos):
    """pos [N][2] -> (nearest [N], nearest_idx [N], min_sep)."""
    pos = np.asarray(pos, dtype=np.float64)
    N = pos.shape[0]
    if N == 1:
        return np.full(1, np.inf), np.full(1, -1, dtype=np.int32), np.float64(np.inf)
    x, y = pos[:, 0], pos[:, 1]
    dx = x[:, None] - x[None, :]
    dy = y[:, None] - y[None, :]
    d2 = dx * dx + dy * dy                  # two roundings of the products, one of the sum: no fma
    d2[np.arange(N), np.arange(N)] = np.inf
    idx = np.argmin(d2, axis=1).astype(np.int32)      # the lowest index among equal minima
    best = d2[np.arange(N), idx]
    idx[np.isinf(best)] = -1
    near = np.sqrt(best)
    return near, idx, near.min()


class RecordRef:
    def __init__(self, env_ids, S, P, N, return_mode, max_episodes, heading=False, clouds=False, fill=0):
        self.env_ids = np.asarray(env_ids, dtype=np.int32)
        self.T, self.S, self.P, self.N = len(self.env_ids), S, P, N
        self.return_mode, self.max_episodes = return_mode, max_episodes
        T = self.T

        def patt(shape, dt):
            a = np.empty(shape, dtype=dt)
            a.view(np.uint8).fill(fill)
            return a
        self.rows = {k: patt((T, S) + shp, dt) for k, (dt, shp) in row_fields(N, heading, clouds).items()}
        self.summaries = patt((T, P), EPISODE)
        self.track = {k: np.zeros(T, dtype=dt) for k, dt in TRACK_FIELDS}
        self.track["run_min_sep"][:] = np.inf

    def _row(self, k, e, src, step, fin):
        """Write (or drop) the row of track k, update its running min-sep; returns nothing."""
        tr, R, N = self.track, self.rows, self.N
        near, idx, sep = separation(src["pos"][e])
        t = int(tr["run_len"][k])
        if sep < tr["run_min_sep"][k]:
            tr["run_min_sep"][k] = sep
            tr["run_min_t"][k] = t
        c = int(tr["cursor"][k])
        if c >= self.S:
            tr["dropped"][k] += 1
            tr["run_flags"][k] |= 2
            return
        R["header"][k, c] = (src["episode"][e], t, (1 if fin else 0) | (0 if step else 2),
                             src["map_idx"][e] if src.get("map_idx") is not None else 0)
        for f in ("pos", "vel", "goal"):
            R[f][k, c] = src[f][e]
        if step:
            R["act"][k, c] = np.asarray(src["act"][e]).astype(np.float32)
            R["reward"][k, c] = np.asarray(src["reward"][e]).astype(np.float64)
            R["done"][k, c] = src["done"][e]
            R["mask"][k, c] = src["mask"][e]
        else:
            for f in ("act", "reward", "done", "mask"):
                R[f][k, c] = 0
        R["nearest"][k, c], R["nearest_idx"][k, c], R["min_sep"][k, c] = near, idx, sep
        for f in ("heading", "clouds"):
            if f in R:
                R[f][k, c] = src[f][e]
        tr["cursor"][k] = c + 1

    def reset_phase(self, src, sel=None):
        """src: dict of the env state arrays (pos, vel, goal [E][N][2], episode [E], map_idx [E] or
        absent, heading / clouds where recorded)."""
        tr = self.track
        for k, e in enumerate(self.env_ids):
            if tr["ep_seen"][k] >= self.max_episodes or (sel is not None and not sel[e]):
                continue
            tr["run_len"][k] = 0
            tr["run_return"][k] = 0.0
            tr["run_flags"][k] = 0
            tr["run_min_sep"][k] = np.inf
            tr["run_min_t"][k] = 0
            tr["row0"][k] = tr["cursor"][k]
            self._row(k, e, src, False, False)

    def step_phase(self, src):
        """src as for reset_phase plus act [E][N][2], reward / done / mask [E][N], env_done [E]."""
        tr = self.track
        for k, e in enumerate(self.env_ids):
            if tr["ep_seen"][k] >= self.max_episodes:
                continue
            tr["run_len"][k] += 1
            r = tr["run_return"][k]
            if self.return_mode == 1:
                r = r + np.float64(src["reward"][e, 0])
            else:
                for i in range(self.N):
                    r = r + np.float64(src["reward"][e, i])
            tr["run_return"][k] = r
            if np.any(src["done"][e]):
                tr["run_flags"][k] |= 1
            fin = bool(src["env_done"][e])
            self._row(k, e, src, True, fin)
            if fin:
                p = int(tr["ep_seen"][k])
                self.summaries[k, p] = (r, tr["run_min_sep"][k], tr["run_min_t"][k], tr["row0"][k],
                                        tr["cursor"][k] - tr["row0"][k], tr["run_len"][k], src["episode"][e], e,
                                        tr["run_flags"][k], 0)
                tr["ep_seen"][k] = p + 1

    def trajectories(self):
        tr = self.track
        return Trajectories(self.env_ids, tr["cursor"], tr["ep_seen"], tr["dropped"], self.summaries, self.rows)


def ulps(a, b):
    """Largest distance in units in the last place between two float64 arrays of non-negative values
    (+inf included: its bit pattern follows the largest finite one)."""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check(got, ref, what=""):
    """``got``: dict with ``rows`` (name -> [T][S]...), ``summaries`` [T][P] of EPISODE, ``track`` (name ->
    [T]) as numpy arrays downloaded from the device; ``ref``: a RecordRef that started from the same fill
    pattern.  Whole arrays are compared, the never-written rows included.  Returns the largest ulp
    distance of the square roots (0: exact equality held)."""
    worst = 0
    for k, w in ref.rows.items():
        g = got["rows"][k]
        if k in ROOTS:
            u = ulps(g, w)
            assert u <= 1, (what, k, u)
            worst = max(worst, u)
        else:
            assert same_bits(g, w), (what, k, np.argwhere(g != w)[:4])
    gs, ws = got["summaries"], ref.summaries
    for f in EPISODE.names:
        if f == "min_sep":
            u = ulps(gs[f], ws[f])
            assert u <= 1, (what, "summary min_sep", u)
            worst = max(worst, u)
        else:
            assert same_bits(gs[f], ws[f]), (what, "summary", f, gs[f], ws[f])
    for k, w in ref.track.items():
        g = got["track"][k]
        if k == "run_min_sep":
            assert ulps(g, w) <= 1, (what, k)
        else:
            assert same_bits(g, w), (what, k, g, w)
    return worst
