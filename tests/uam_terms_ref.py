"""Test-side restatement of the UAM reward terms (include/aac_terms.h, the UAM table): ``ss_reward`` of
oracle/uam_ref.py copied with its locals kept, so that every aircraft's 12 slots come out beside the
oracle's outputs.  Test infrastructure only, no GPU needed.

The copy follows the oracle line by line (the same calls in the same order, the same state changes);
tests/test_uam_terms_cpu.py holds it to the oracle's own reward, done, mask and bbc bit for bit.

Slots as tests/terms_ref.py (``NAMES``); the UAM reward uses 0 event, 3 progress, 5 building, 6 drone and
the four gauges.  The crash penalty and the near-drone coefficient double on a bearing in [90, 180] and
stay doubled for the later aircraft of the call, so a row depends on the aircraft before it."""
import math

import numpy as np

from oracle import geos
from oracle import uam_ref as U
from tests.terms_ref import NAMES, SLOTS, WIDTH, LedgerRef, slot_sum  # noqa: F401  (re-exported)

KINDS = ("bound", "cloud", "drone", "goal", "normal")
USED = (0, 3, 5, 6, 8, 9, 10, 11)          # the slots the UAM variant fills


class UamTerms(U.UAMEnv):
    """oracle/uam_ref.UAMEnv whose ``ss_reward_terms`` also returns the (N, 12) terms."""

    def ss_reward_terms(self):
        """``UAMEnv.ss_reward`` (UAM/env:3892-4629) with the locals kept.  Returns (terms (N, 12), reward,
        done, check_goal, bbc, mask) and leaves ``self.events``: per aircraft the branch taken (``kind``,
        an index into ``KINDS``), whether its nearest neighbour was in the near band (``band``) and
        whether that doubled the coefficient (``band_dbl``) or its collision doubled the crash penalty
        (``crash_dbl``)."""
        N = self.N
        crash = U.CRASH
        ndc = U.NEAR_DRONE_COEF
        bbc = [False] * 4
        reward, done, check_goal, mask = [], [], [False] * N, []
        terms = np.zeros((N, WIDTH))
        ev = dict(kind=[], band=[], band_dbl=[], crash_dbl=[])
        for i, ag in self.all_agents.items():
            if U.gons_meet(ag.pos, ag.protectiveBound, ag.goal[-1], U.GOAL_R):
                ag.reach_target = True
        c_drone = 1 + (U.NEAR_LO / (U.NEAR_HI - U.NEAR_LO))
        m_drone = (0 - 1) / (U.NEAR_HI - U.NEAR_LO)
        for i, ag in self.all_agents.items():
            collision = []
            nearest, shortest, bearing, coll_bearing = None, math.inf, None, None
            for j in ag.surroundingNeighbor:
                other = self.all_agents[j]
                diff = ag.pos - other.pos
                d = np.linalg.norm(diff)
                if d < shortest:
                    shortest = d
                    bearing = U.calculate_bearing(ag.pos[0], ag.pos[1], other.pos[0], other.pos[1])
                    nearest = j
                if np.linalg.norm(diff) <= ag.protectiveBound * 2:
                    if not (other.reach_target or ag.reach_target):
                        coll_bearing = U.calculate_bearing(ag.pos[0], ag.pos[1], other.pos[0], other.pos[1])
                        collision.append(j)
                        ag.drone_collision = True
            prev_two = 0
            for cnt, j in enumerate(ag.pre_surroundingNeighbor):
                if j in collision:
                    prev_two = 1
                    break
                if cnt + 1 > 1:
                    break
            cloud = 0
            if not ag.reach_target:
                if U.gon_rect_overlap(ag.pos, ag.protectiveBound, U.RUNWAY):
                    cloud = 1
                for cl in self.clouds:
                    if U.gons_meet(ag.pos, ag.protectiveBound, cl.pos, cl.radius, strict=True):
                        cloud = 1
                        break
            if cloud:
                ag.cloud_collision = True
            goal = U.gons_meet(ag.pos, ag.protectiveBound, ag.goal[-1], U.GOAL_R)
            s, g = ag.ini_pos, np.array(ag.goal[0])
            L = geos.point_dist(g[0], g[1], s[0], s[1])
            ddx, ddy = g[0] - s[0], g[1] - s[1]
            fr = ((ag.pos[0] - s[0]) * ddx + (ag.pos[1] - s[1]) * ddy) / (ddx * ddx + ddy * ddy)
            fr = min(max(fr, 0.0), 1.0)
            near = (s[0] + fr * ddx, s[1] + fr * ddy)
            cross = geos.point_dist(ag.pos[0], ag.pos[1], near[0], near[1])
            left = cross + (L - fr * L)
            dist_to_goal = U.DIST_COEF * (1 - (left / L))
            band = nearest is not None and U.NEAR_LO <= shortest <= U.NEAR_HI
            band_dbl = False
            if band:
                if 90.0 <= bearing <= 180:
                    ndc = ndc * 2
                    band_dbl = True
                near_drone = ndc * (m_drone * shortest + c_drone)
            else:
                near_drone = ndc * 0
            min_dist = float(np.min(ag.observableSpace))
            m = (0 - 1) / (U.TURNING_PT - ag.protectiveBound)
            if ag.protectiveBound <= min_dist <= U.TURNING_PT:
                near_building = U.NEAR_BUILDING_COEF * (m * min_dist + 2)
            else:
                near_building = 0
            bnd = geos.bound_crash(ag.pre_pos, ag.pos, U.BOUND, ag.protectiveBound)
            mk = int(bnd) | (cloud << 1) | ((len(collision) > 0) << 2) | (int(goal) << 3)
            t = terms[i]
            crash_dbl = False
            if bnd:
                ag.bound_collision = True
                rew = 0 - crash
                t[0] = -crash
                done.append(True)
                bbc[0] = True
                kind = 0
            elif cloud == 1:
                done.append(True)
                bbc[1] = True
                rew = 0 - crash
                t[0] = -crash
                kind = 1
            elif collision:
                done.append(True)
                bbc[2] = True
                if 90.0 <= coll_bearing <= 180:
                    crash = crash * 2
                    crash_dbl = True
                rew = 0 - crash
                t[0] = -crash
                if prev_two:
                    bbc[3] = True
                    mk |= 32
                kind = 2
            elif goal:
                ag.reach_target = True
                check_goal[i] = True
                rew = 0 + U.REACH + 0
                t[0] = U.REACH
                done.append(False)
                mk |= 16
                kind = 3
            else:
                rew = 0 + dist_to_goal - near_building - near_drone
                t[3], t[5], t[6] = dist_to_goal, -near_building, -near_drone
                done.append(False)
                kind = 4
            t[8], t[9] = cross, np.linalg.norm(ag.vel)
            t[10], t[11] = np.linalg.norm(ag.pos - np.array(ag.goal[-1])), min_dist
            reward.append(rew)
            mask.append(mk)
            ev["kind"].append(kind)
            ev["band"].append(bool(band))
            ev["band_dbl"].append(band_dbl)
            ev["crash_dbl"].append(crash_dbl)
        self.events = ev
        return (terms, np.array(reward), np.array(done), np.array(check_goal), np.array(bbc),
                np.array(mask, dtype=np.uint8))

    def full_step_terms(self, actions):
        """``full_step`` with the terms: (terms, reward, done, check_goal, bbc, mask, episode over)."""
        self.step(actions)
        t, r, d, cg, bbc, mk = self.ss_reward_terms()
        self.step_count += 1
        return t, r, d, cg, bbc, mk, self.episode_over(d)


def uam_env(state, e, N):
    """``UamTerms`` holding env e of a device state dict (``oracle.uam_ref.env_from_state``)."""
    env = U.env_from_state(state, e, N)
    env.__class__ = UamTerms
    return env


def batch_terms(state, N, envs=None, act=None):
    """One step of the envs ``envs`` (None: all) of a state dict from ``act`` (E, N, 2; None: zeros):
    {env: (terms (N, 12), reward (N,), events)} -- the reference for the kernel's terms buffer."""
    E = state["pos"].shape[0]
    out = {}
    for e in (range(E) if envs is None else envs):
        env = uam_env(state, e, N)
        t, r, _, _, _, _, _ = env.full_step_terms(np.zeros((N, 2)) if act is None else act[e])
        out[e] = (t, r, env.events)
    return out
