"""Plain-numpy restatement of the episode statistics (include/aac_stats.h): the per-env rule,
replayed one env at a time, step by step.  The GPU tests compare against it: integers and the running
state bit-exact (the add order of ``run_return`` is fixed), floating-point totals within the bound
for any summation order, ``sum_bound``."""
import math

import numpy as np

COUNTERS = ("episodes", "steps", "timeout", "crash", "goal", "collision_count", "crash_bound", "crash_building",
            "crash_drone", "crash_nearest", "all_steps_used")
TIMEOUT, CRASH, GOAL = 0, 1, 2


class StatsRef:
    def __init__(self, E, N, episode_length, goal_bit, return_mode, log=0):
        self.E, self.N, self.episode_length = E, N, episode_length
        self.goal_bit, self.return_mode, self.L = goal_bit, return_mode, log
        self.reset()

    def reset(self):
        E = self.E
        self.run_return = np.zeros(E, dtype=np.float64)
        self.run_len = np.zeros(E, dtype=np.int32)
        self.run_reach = [0] * E                     # Python ints: 64 bits and more
        self.ep_count = np.zeros(E, dtype=np.int32)
        self.clear()
        self.rows = []                               # every finished episode, in (step, env) order
        self.calls = 0
        self.under_quota = 0

    def clear(self):
        self.c = {k: 0 for k in COUNTERS}
        self.returns = []                            # finished episodes' returns, in order
        self.reach_hist = [0] * (self.N + 1)

    def accumulate(self, reward, done, mask, env_done, bbc, quota=None, step_index=-1):
        step_index = self.calls if step_index < 0 else step_index
        under = 0
        for e in range(self.E):
            if quota is not None and self.ep_count[e] >= quota[e]:
                continue
            r = self.run_return[e]
            if self.return_mode == 1:
                r = r + np.float64(reward[e, 0])
            else:
                for i in range(self.N):
                    r = r + np.float64(reward[e, i])
            self.run_return[e] = r
            self.run_len[e] += 1
            for i in range(self.N):
                if (int(mask[e, i]) >> self.goal_bit) & 1:
                    self.run_reach[e] |= 1 << i
            if env_done[e]:
                self._finish(e, bool(done[e].any()), bbc[e], step_index)
            if quota is None or self.ep_count[e] < quota[e]:
                under += 1
        self.under_quota = under
        self.calls += 1

    def _finish(self, e, anyd, b, step_index):
        c, ln, ret = self.c, int(self.run_len[e]), float(self.run_return[e])
        k = bin(self.run_reach[e]).count("1")
        reason = TIMEOUT if self.episode_length < ln else CRASH if anyd else GOAL
        crash = 0
        c["episodes"] += 1
        c["steps"] += ln
        c[("timeout", "crash", "goal")[reason]] += 1
        if anyd and ln < self.episode_length:        # ATT/main:581-595
            c["collision_count"] += 1
            crash = 5
            if b[0]:
                crash = 1
                c["crash_bound"] += 1
            elif b[1]:
                crash = 2
                c["crash_building"] += 1
            elif b[2]:
                crash = 3
                c["crash_drone"] += 1
                if b[3]:
                    crash = 4
                    c["crash_nearest"] += 1
        else:
            c["all_steps_used"] += 1
        self.reach_hist[k] += 1
        self.returns.append(ret)
        self.rows.append((ret, step_index, ln, e, reason, crash, k))
        self.ep_count[e] += 1
        self.run_return[e] = 0.0
        self.run_len[e] = 0
        self.run_reach[e] = 0

    # ------------------------------------------------------------------- comparisons
    def log_rows(self):
        return self.rows[-self.L:] if self.L else []

    def reach_array(self):
        return np.array(self.run_reach, dtype=np.uint64).view(np.int64)


def sum_bound(xs):
    """|S - S'| of two float64 sums of the same n terms in any two orders: each is within
    (n - 1) u sum|x| (1 + O(n u)) of the exact sum with u = 2^-53, so n 2^-53 sum|x| bounds the
    difference to first order for n >= 2; the issue states the bound as n 2^-53 sum|x|."""
    xs = np.asarray(xs, dtype=np.float64)
    return len(xs) * 2.0 ** -53 * float(np.abs(xs).sum())


def check_totals(got, ref):
    """``got``: EpisodeStats.read(); ``ref``: a StatsRef.  Integers exact, sums within sum_bound,
    min / max exact."""
    for k in COUNTERS:
        assert got[k] == ref.c[k], (k, got[k], ref.c[k])
    assert got["reach_hist"] == ref.reach_hist, (got["reach_hist"], ref.reach_hist)
    r = np.array(ref.returns, dtype=np.float64)
    s, q = float(r.sum()), float((r * r).sum())
    print("return_sum", got["return_sum"], s, "bound", sum_bound(r), "sqsum", got["return_sqsum"], q, "bound",
          sum_bound(r * r))
    assert abs(got["return_sum"] - s) <= sum_bound(r), (got["return_sum"], s)
    assert abs(got["return_sqsum"] - q) <= sum_bound(r * r), (got["return_sqsum"], q)
    if len(r):
        assert got["return_min"] == r.min() and got["return_max"] == r.max()
    else:
        assert math.isnan(got["return_min"]) and math.isnan(got["return_max"])


def check_state(stats, ref):
    """Running state of an EpisodeStats against the restatement, bit-exact."""
    assert np.array_equal(stats.run_return.cpu().numpy().view(np.int64), ref.run_return.view(np.int64))
    assert np.array_equal(stats.run_len.cpu().numpy(), ref.run_len)
    assert np.array_equal(stats.run_reach.cpu().numpy(), ref.reach_array())
    assert np.array_equal(stats.ep_count.cpu().numpy(), ref.ep_count)


def check_log(stats, ref):
    rows = stats.log_rows()
    want = ref.log_rows()
    assert len(rows) == len(want), (len(rows), len(want))
    for g, w in zip(rows, want):
        assert (float(g["ret"]), int(g["step"]), int(g["len"]), int(g["env"]), int(g["reason"]), int(g["crash"]),
                int(g["reach"])) == w, (g, w)
