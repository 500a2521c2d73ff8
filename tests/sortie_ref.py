"""Plain-Python restatement of the sortie rule of include/aac_sortie.h: scalar double arithmetic (Python
floats), the same order of additions as the header, sequential sums over (call, env, aircraft).  The GPU
tests compare the kernel's counters, running state and log rows with it bit for bit, and the double sums
within the bound of a reordered sum."""
import math

import numpy as np

CLASSES = ("bound", "obstacle", "drone", "reached", "idle")
COUNTERS = ("sorties",) + CLASSES + ("degenerate", "episodes", "reach_step_sum")
BITS_ENV = dict(bound_bit=0, drone_bit=1, obstacle_bit=3, goal_bit=5)      # aac_env.h (ATT / WGRU)
BITS_UAM = dict(bound_bit=0, obstacle_bit=1, drone_bit=2, goal_bit=4)      # aac_uam.h
ROW = np.dtype([("env", "<i4"), ("agent", "<i4"), ("episode", "<i4"), ("cls", "<i4"), ("len", "<i4"),
                ("reach_step", "<i4"), ("flown", "<f8"), ("straight", "<f8"), ("ratio", "<f8")])


def norm(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def classify(flags, bound_bit, obstacle_bit, drone_bit, goal_bit):
    for cls, b in enumerate((bound_bit, obstacle_bit, drone_bit, goal_bit)):
        if (flags >> b) & 1:
            return cls
    return 4


class SortieRef:
    def __init__(self, E, N, episode_length, reach_margin, bound_bit, obstacle_bit, drone_bit, goal_bit):
        self.E, self.N, self.episode_length, self.margin = E, N, int(episode_length), float(reach_margin)
        self.bits = (bound_bit, obstacle_bit, drone_bit, goal_bit)
        self.goal_bit = goal_bit
        self.straight = np.zeros((E, N))
        self.first_seg = np.zeros((E, N))
        self.run_dist = np.zeros((E, N))
        self.last_pos = np.zeros((E, N, 2))
        self.run_flags = np.zeros((E, N), dtype=np.uint8)
        self.reach_step = np.zeros((E, N), dtype=np.int32)
        self.run_len = np.zeros(E, dtype=np.int32)
        self.ep_count = np.zeros(E, dtype=np.int32)
        self.collide_hist = np.zeros(self.episode_length + 2, dtype=np.int64)
        self.cnt = {k: 0 for k in COUNTERS}
        self.ratios, self.flowns, self.straights = [], [], []      # of the counted reached sorties, in order
        self.rows = []

    def accumulate(self, pos, start, goal, done, mask, env_done, quota=None, episode=None):
        E, N = self.E, self.N
        for e in range(E):
            if quota is not None and self.ep_count[e] >= quota[e]:
                continue
            rl = int(self.run_len[e])
            for i in range(N):
                px, py = float(pos[e, i, 0]), float(pos[e, i, 1])
                if rl == 0:
                    sx, sy = float(start[e, i, 0]), float(start[e, i, 1])
                    self.straight[e, i] = norm(float(goal[e, i, 0]) - sx, float(goal[e, i, 1]) - sy)
                    self.first_seg[e, i] = norm(px - sx, py - sy)
                    self.run_dist[e, i] = 0.0
                else:
                    self.run_dist[e, i] = float(self.run_dist[e, i]) + norm(px - float(self.last_pos[e, i, 0]),
                                                                            py - float(self.last_pos[e, i, 1]))
                self.last_pos[e, i] = (px, py)
                self.run_flags[e, i] |= mask[e, i]
                if (int(mask[e, i]) >> self.goal_bit) & 1 and self.reach_step[e, i] == 0:
                    self.reach_step[e, i] = rl + 1
            ln = rl + 1
            self.run_len[e] = ln
            if not env_done[e]:
                continue
            for i in range(N):
                cls = classify(int(self.run_flags[e, i]), *self.bits)
                straight = float(self.straight[e, i])
                flown = (float(self.run_dist[e, i]) + float(self.first_seg[e, i])) + self.margin
                ratio = math.nan
                self.cnt["sorties"] += 1
                self.cnt[CLASSES[cls]] += 1
                if cls == 3:
                    self.cnt["reach_step_sum"] += int(self.reach_step[e, i])
                    if straight > 0.0 and math.isfinite(flown):
                        ratio = flown / straight
                        self.ratios.append(ratio)
                        self.flowns.append(flown)
                        self.straights.append(straight)
                    else:
                        self.cnt["degenerate"] += 1
                self.rows.append((e, i, int(episode[e]) if episode is not None else int(self.ep_count[e]), cls, ln,
                                  int(self.reach_step[e, i]), flown, straight, ratio))
            self.cnt["episodes"] += 1
            if bool(np.any(done[e])) and ln < self.episode_length and 0 <= ln < len(self.collide_hist):
                self.collide_hist[ln] += 1
            self.ep_count[e] += 1
            self.run_len[e] = 0
            self.run_flags[e] = 0
            self.reach_step[e] = 0

    # ------------------------------------------------------------------- results
    def sums(self):
        """The six double totals by sequential sums, and the number of summands."""
        r = self.ratios
        out = dict(ratio_sum=0.0, ratio_sqsum=0.0, ratio_min=math.inf, ratio_max=-math.inf, flown_sum=0.0,
                   straight_sum=0.0)
        for x, f, s in zip(r, self.flowns, self.straights):
            out["ratio_sum"] += x
            out["ratio_sqsum"] += x * x
            out["ratio_min"] = min(out["ratio_min"], x)
            out["ratio_max"] = max(out["ratio_max"], x)
            out["flown_sum"] += f
            out["straight_sum"] += s
        return out, len(r)

    def log_rows(self, L=None):
        rows = np.array(self.rows, dtype=ROW) if self.rows else np.zeros(0, dtype=ROW)
        return rows if L is None else rows[-L:]

    def running(self):
        return dict(straight=self.straight, first_seg=self.first_seg, run_dist=self.run_dist, last_pos=self.last_pos,
                    run_flags=self.run_flags, reach_step=self.reach_step, run_len=self.run_len, ep_count=self.ep_count)
