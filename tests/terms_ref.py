"""Test-side restatement of the reward terms (include/aac_terms.h): ``ss_reward`` of
oracle/env_ref.py (ATT) and oracle/wgru_env_ref.py (WGRU) copied with their locals kept, so that every
agent's 12 slots come out beside the reward.  Test infrastructure only, no GPU needed.

The copies follow the oracles line by line (the same calls in the same order, the same state changes);
tests/test_terms_cpu.py holds them to the oracles' own rewards bit for bit.  ``step`` of both classes
skips the observation (the radar of the ATT env feeds no reward term); the WGRU env keeps its obstacle
radar, whose minimum the near-building penalty reads.

Slots (``NAMES``): 0 event, 1 waypoint bonus, 2 path, 3 progress, 4 speed, 5 building, 6 drone,
7 reserved | 8 cross-track distance, 9 |v|, 10 distance to the progress term's target, 11 radar minimum.
A slot holds what the taken branch added to the agent's own reward, sign included, 0 where the branch
leaves the term out; ``slot_sum`` adds slots 0..6 left to right."""
import math

import numpy as np

from oracle import geos
from oracle.consts import BOUND, CRASH_PENALTY, NEAR_HI, NEAR_LO, REACH_REWARD, WP_REACH
from oracle.env_ref import ScalarEnv
from oracle import wgru_env_ref as W

NAMES = ("event", "waypoint", "path", "progress", "speed", "building", "drone", "reserved",
         "cross_track", "speed_norm", "goal_dist", "radar_min")
WIDTH, SLOTS = 12, 8


def slot_sum(t):
    """((((((s0+s1)+s2)+s3)+s4)+s5)+s6) over the last axis, in double."""
    t = np.asarray(t, dtype=np.float64)
    s = t[..., 0] + t[..., 1]
    for k in range(2, 7):
        s = s + t[..., k]
    return s


class AttTerms(ScalarEnv):
    """oracle/env_ref.ScalarEnv whose ``ss_reward_terms`` also returns the (N, 12) terms."""

    def cur_state_norm_state_v3(self):
        for ag in self.all_agents.values():
            self.get_current_agent_nei(ag)
        return None

    def ss_reward_terms(self):
        """``ScalarEnv.ss_reward`` (ATT/env:2105-2618) with the locals kept.  Returns (terms (N, 12),
        own rewards (N,) before the team sum, done list, masks list)."""
        terms = np.zeros((self.N, WIDTH))
        own, done, masks = [], [], []
        c_drone = 1 + (NEAR_LO / (NEAR_HI - NEAR_LO))
        m_drone = (0 - 1) / (NEAR_HI - NEAR_LO)
        for idx, ag in self.all_agents.items():
            collision_drones = []
            shortest = math.inf
            all_dist = []
            for k in ag.surroundingNeighbor:
                diff = ag.pos - self.all_agents[k].pos
                d = np.linalg.norm(diff)
                all_dist.append(d)
                if d < shortest:
                    shortest = d
                if np.linalg.norm(diff) <= ag.protectiveBound * 2:
                    collision_drones.append(k)
            building = 0
            for cx, cy in self.cells:
                if geos.building_hit_cell(ag.pos[0], ag.pos[1], cx, cy):
                    building = 1
                    ag.collide_wall_count += 1
                    break
            goal_hit = geos.goal_reached(ag.pos[0], ag.pos[1], float(ag.goal[-1][0]), float(ag.goal[-1][1]))
            wp0 = ag.waypoints[0]
            wp_flag = geos.point_dist(ag.pos[0], ag.pos[1], float(wp0[0]), float(wp0[1])) < WP_REACH
            before = np.linalg.norm(ag.pre_pos - ag.goal[-1])
            after = np.linalg.norm(ag.pos - ag.goal[-1])
            dist_to_goal = 1 * (before - after)
            dist_to_goal = dist_to_goal / ag.maxSpeed
            near_pen = 0
            for d in all_dist:
                if d >= NEAR_LO and d <= NEAR_HI:
                    near_pen = near_pen + (1 * (m_drone * shortest + c_drone))
                else:
                    near_pen = near_pen + 1 * 0
            bound_hit = geos.bound_crash(ag.pre_pos, ag.pos, BOUND, ag.protectiveBound)
            m = (bound_hit << 0) | ((len(collision_drones) > 0) << 1) | (goal_hit << 2) | (building << 3) | (wp_flag << 4)
            t = terms[idx]
            if bound_hit:
                rew = 0 - CRASH_PENALTY - 0.0 - 0
                t[0] = -CRASH_PENALTY
                done.append(True)
            elif len(collision_drones) > 0:
                done.append(True)
                rew = 0 - CRASH_PENALTY - 0.0 - near_pen
                t[0], t[6] = -CRASH_PENALTY, -near_pen
            elif goal_hit:
                ag.reach_target = True
                rew = 0 + REACH_REWARD + 0.0
                t[0] = REACH_REWARD
                m |= 32
                done.append(False)
            else:
                if wp_flag and len(ag.waypoints) > 1:
                    ag.removed_goal = ag.waypoints.pop(0)
                rew = 0 + 0.0 + dist_to_goal - 0.0 + 0.0 - 0 + 0 - 0 - near_pen - 0
                t[3], t[6] = dist_to_goal, -near_pen
                done.append(False)
            t[9], t[10] = np.linalg.norm(ag.vel), after
            own.append(float(rew))
            masks.append(int(m))
        return terms, np.array(own), done, masks


class WgruTerms(W.WgruEnv):
    """oracle/wgru_env_ref.WgruEnv whose ``ss_reward_terms`` also returns the (N, 12) terms."""

    def cur_state_norm_state_v3(self):
        for i, ag in self.all_agents.items():
            self.get_current_agent_nei(ag)
            ag.observableSpace = self.radar(i)
        return None

    def ss_reward_terms(self, rmin=None):
        """``WgruEnv.ss_reward`` (WGRU/env:1666-2039) with the locals kept.  ``rmin``: radar minima to
        use instead of the agents' own radar rows (N values; the exact minima of a fix-up test).
        Returns (terms (N, 12), rewards (N,), done list, masks list)."""
        terms = np.zeros((self.N, WIDTH))
        reward, done, masks = [], [], []
        for idx, ag in self.all_agents.items():
            collision = False
            for k in ag.surroundingNeighbor:
                if np.linalg.norm(ag.pos - self.all_agents[k].pos) <= ag.protectiveBound * 2:
                    collision = True
            building = 0
            for cx, cy in self.cells:
                if geos.building_hit_cell(ag.pos[0], ag.pos[1], cx, cy):
                    building = 1
                    ag.collide_wall_count += 1
                    break
            goal_hit = geos.goal_reached(ag.pos[0], ag.pos[1], float(ag.goal[-1][0]), float(ag.goal[-1][1]))
            smallest = math.inf
            wp_flag = False
            next_wp = None
            for wpidx, wp in enumerate(ag.goal):
                d = geos.point_dist(ag.pos[0], ag.pos[1], float(wp[0]), float(wp[1]))
                if d < smallest:
                    smallest = d
                    next_wp = np.array(wp, dtype=float)
                    if smallest < W.WP_REACH:
                        wp_flag = True
                        if len(ag.goal) > 1:
                            ag.removed_goal = ag.goal.pop(wpidx)
                            best, pick = math.inf, None
                            for g in ag.goal:
                                dd = geos.point_dist(float(g[0]), float(g[1]), ag.pos[0], ag.pos[1])
                                if dd < best:
                                    best, pick = dd, g
                            next_wp = np.array(pick, dtype=float)
                        break
            before = np.linalg.norm(ag.pre_pos - next_wp)
            after = np.linalg.norm(ag.pos - next_wp)
            dist_to_goal = 1 * (before - after)
            cross = geos.cross_track_distance(ag.pos[0], ag.pos[1], ag.ref_line)
            if cross <= ag.protectiveBound:
                m = (0 - 1) / (ag.protectiveBound - 0)
                dist_to_ref_line = W.COEF_REF_LINE * (m * cross + 1)
            else:
                dist_to_ref_line = -W.COEF_REF_LINE * 1
            thr = 2 * ag.protectiveBound
            speed = np.linalg.norm(ag.vel)
            small_step_penalty = W.SMALL_STEP_COEF * ((thr - np.clip(speed, 0, thr)) * (1.0 / thr))
            min_dist = np.min(ag.observableSpace) if rmin is None else rmin[idx]
            m = (0 - 1) / (W.TURNING_PT - ag.protectiveBound)
            if min_dist >= ag.protectiveBound and min_dist <= W.TURNING_PT:
                near_building_penalty = W.NEAR_BUILDING_COEF * (m * min_dist + 2)
            else:
                near_building_penalty = 0
            bound_hit = geos.bound_crash(ag.pre_pos, ag.pos, BOUND, ag.protectiveBound)
            msk = (bound_hit << 0) | (collision << 1) | (goal_hit << 2) | (building << 3) | (wp_flag << 4)
            rew = 0
            t = terms[idx]
            if bound_hit or building == 1:
                rew = rew + dist_to_ref_line - W.CRASH_PENALTY + dist_to_goal - small_step_penalty + 0 - \
                    near_building_penalty
                t[0], t[2], t[3], t[4], t[5] = (-W.CRASH_PENALTY, dist_to_ref_line, dist_to_goal, -small_step_penalty,
                                                -near_building_penalty)
                done.append(True)
            elif goal_hit:
                ag.reach_target = True
                rew = rew + W.REACH_REWARD + 0
                t[0] = W.REACH_REWARD
                msk |= 32
                done.append(False)
            else:
                if wp_flag and len(ag.goal) > 1:
                    rew = rew + W.COEF_REF_LINE
                    t[1] = W.COEF_REF_LINE
                rew = rew + dist_to_ref_line + dist_to_goal - small_step_penalty + 0 - near_building_penalty + 0
                t[2], t[3], t[4], t[5] = dist_to_ref_line, dist_to_goal, -small_step_penalty, -near_building_penalty
                done.append(False)
            t[8], t[9], t[10], t[11] = cross, speed, after, min_dist
            reward.append(float(rew))
            masks.append(int(msk))
        return terms, np.array(reward), done, masks


def att_env(st, e, occ, mode=0):
    """``AttTerms`` holding env e of a tests/thresholds.py state dict (wp_cur = 0)."""
    N = st["pos"].shape[1]
    env = AttTerms(N, occ, radar_mode=mode)
    for i, ag in env.all_agents.items():
        cnt = int(st["cnt"][e, i])
        ag.pos, ag.pre_pos = st["pos"][e, i].copy(), st["pre_pos"][e, i].copy()
        ag.ini_pos = ag.pos.copy()
        ag.vel, ag.pre_vel = st["vel"][e, i].copy(), st["vel"][e, i].copy()
        ag.goal = [list(w) for w in st["wp"][e, i, :cnt]]
        ag.waypoints = [list(w) for w in st["wp"][e, i, :cnt]]
        ag.removed_goal, ag.reach_target, ag.collide_wall_count = None, False, 0
    return env


def wgru_env(st, e, occ):
    """``WgruTerms`` holding env e of a tests/wgru_thresholds.py state dict."""
    from tests import wgru_thresholds as WT
    env, _ = WT.scalar_env(st, e, occ)
    env.__class__ = WgruTerms
    return env


def batch_terms(variant, st, occ, act, mode=0, rmin=None):
    """Terms (E, N, 12) and own rewards (E, N) of one step of every env of a state dict from ``act``
    (E, N, 2) -- the reference for the kernel's terms buffer.  ``rmin`` (E, N): WGRU radar minima to use
    (NaN: the restatement's own)."""
    E, N = st["pos"].shape[:2]
    terms, rew = np.zeros((E, N, WIDTH)), np.zeros((E, N))
    for e in range(E):
        env = wgru_env(st, e, occ) if variant == "wgru" else att_env(st, e, occ, mode)
        env.step(act[e])
        if variant == "wgru":
            rm = None
            if rmin is not None:
                own = [float(np.min(env.all_agents[i].observableSpace)) for i in range(N)]
                rm = [own[i] if np.isnan(rmin[e, i]) else float(rmin[e, i]) for i in range(N)]
            terms[e], rew[e], _, _ = env.ss_reward_terms(rm)
        else:
            terms[e], rew[e], _, _ = env.ss_reward_terms()
    return terms, rew


# ---------------------------------------------------------------------------- the ledger's fold rule
EPW = 256


def _tree(v, op):
    """Entry j with j + s, s = 128, 64, .. 1 (the fixed tree of aac_terms.h) over 256 entries."""
    v = np.array(v, dtype=np.float64)
    s = 128
    while s:
        v[:s] = op(v[:s], v[s:2 * s])
        s >>= 1
    return v[0]


class LedgerRef:
    """numpy restatement of aac_terms_accumulate / aac_terms_reduce: the same additions in the same
    order, so sums are bit-equal to the device's."""

    def __init__(self, E, N):
        self.E, self.N, self.G = E, N, (E + EPW - 1) // EPW
        self.run = np.zeros((E, N, SLOTS))
        self.ep_count = np.zeros(E, np.int64)
        self.cnt = np.zeros(self.G, np.int64)
        self.sum, self.sq = np.zeros((self.G, SLOTS)), np.zeros((self.G, SLOTS))
        self.min, self.max = np.full((self.G, SLOTS), np.inf), np.full((self.G, SLOTS), -np.inf)

    def accumulate(self, terms, env_done, quota=None):
        for g in range(self.G):
            e0 = g * EPW
            t = np.zeros((SLOTS, EPW))
            fin = np.zeros(EPW, bool)
            for le in range(min(EPW, self.E - e0)):
                e = e0 + le
                if quota is not None and self.ep_count[e] >= quota[e]:
                    continue
                f = bool(env_done[e])
                tk = np.zeros(SLOTS)
                for i in range(self.N):
                    v = self.run[e, i] + terms[e, i, :SLOTS]
                    tk = tk + v
                    self.run[e, i] = 0.0 if f else v
                if f:
                    t[:, le], fin[le] = tk, True
            if not fin.any():
                continue
            self.ep_count[e0:e0 + EPW][fin[:self.E - e0]] += 1
            self.cnt[g] += int(fin.sum())
            for k in range(SLOTS):
                self.sum[g, k] += _tree(t[k], np.add)
                self.sq[g, k] += _tree(t[k] * t[k], np.add)
                self.min[g, k] = min(self.min[g, k], _tree(np.where(fin, t[k], np.inf), np.minimum))
                self.max[g, k] = max(self.max[g, k], _tree(np.where(fin, t[k], -np.inf), np.maximum))

    def reduce(self):
        """(episodes, sum[8], sqsum[8], min[8], max[8]): thread t takes slots t, t + 256, .. in order, then
        the tree."""
        def fold(a, op, ident):
            out = np.zeros(SLOTS)
            for k in range(SLOTS):
                lane = np.full(EPW, ident)
                for g in range(self.G):
                    lane[g % EPW] = op(lane[g % EPW], a[g, k])
                out[k] = _tree(lane, op)
            return out
        return (int(self.cnt.sum()), fold(self.sum, np.add, 0.0), fold(self.sq, np.add, 0.0),
                fold(self.min, np.minimum, np.inf), fold(self.max, np.maximum, -np.inf))
