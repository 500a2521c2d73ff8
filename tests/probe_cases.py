"""States shared by the radar-probe tests (tests/test_probe_cpu.py, tests/test_probe_gpu.py): the hand-built
ties of exactly representable coordinates, and random rows around the map.  No GPU needed here."""
import numpy as np

from oracle.consts import BOUND
from tests.helpers import random_od

GW, GH = 23, 13
FAR = (470.0, 378.0)        # a partner out of every hand-built ray's reach


def hand_map():
    """Two vertically stacked occupied cells: (10, 5) = [555, 565] x [305, 315] and (10, 6) = [555, 565] x
    [315, 325]; linear indices 135 and 136."""
    occ = np.zeros((GW, GH), np.uint8)
    occ[10, 5] = occ[10, 6] = 1
    return occ


# rows of N = 2 positions for the combined radar on hand_map(), and the records they must give:
# (row, agent, ray) -> (kind, id, dist, point)
HAND_ROWS = np.array([
    [(545.0, 315.0), FAR],              # 0: the 0-degree ray at the shared edge height of the two cells
    [(547.0, 310.0), (557.5, 310.0)],   # 1: the partner's 64-gon vertex 32 = (555, 310) on cell 135's near face
    [(540.0, 310.0), FAR],              # 2: cell 135's near face exactly at the 0-degree ray's end (d == len)
])
HAND_WANT = {
    # both cells at 10 m (x = 555 at y = 315 lies in both closed squares): the lower linear index
    (0, 0, 0): (2, 135, 10.0, (555.0, 315.0)),
    # drone and cell at 8 m: t * 15 rounds into 547 + 8 = 555 exactly on both paths, the drone (kind 1) wins
    (1, 0, 0): (1, 1, 8.0, (555.0, 310.0)),
    # the 180-degree ray of row 2 meets nothing: none, the point is the ray end (cos(pi) = -1 exactly)
    (2, 0, 9): (0, -1, 15.0, (525.0, 310.0)),
    # a cell hit at exactly d == len: the slab parameter is (555 - 540) / 15 = 1.0, d = 15 = len, d <= len holds
    (2, 0, 0): (2, 135, 15.0, (555.0, 310.0)),
}


def random_rows(M, N, seed):
    """M rows of N positions: clusters around a random centre in (and slightly beyond) the bound, so that
    drones, cells and bound lines all come within radar reach."""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(BOUND[0] - 3, BOUND[1] + 3, M), rng.uniform(BOUND[2] - 3, BOUND[3] + 3, M)], -1)
    return centre[:, None, :] + rng.normal(scale=6.0, size=(M, N, 2))


# the GPU cases: name -> (radar mode, N, env variant); E = 16 envs each
E = 16
CASES = {"drones2": (0, 2, "att"), "drones5": (0, 5, "att"), "obstacles3": (1, 3, "att"),
         "obstacles8": (1, 8, "wgru"), "combined5": (2, 5, "att"), "twomap": (2, 5, "att")}
SEEDS = {"drones2": 21, "drones5": 22, "obstacles3": 23, "obstacles8": 24, "combined5": 25, "twomap": 26}


def reset_state(occ, name):
    """(start [E][N][2], wps, cnt, map stack, map_idx or None) of a case: a random OD per env on the env's
    map; ``twomap`` stacks a second synthetic map and mixes the envs over both."""
    mode, N, variant = CASES[name]
    st, wps, cnt = random_od(occ, E, N, seed=SEEDS[name])
    if name != "twomap":
        return st, wps, cnt, np.asarray(occ), None
    from multi_agent_aac_amd import world
    occ2 = world.synthetic_map(7)
    st2, wps2, cnt2 = random_od(occ2, E, N, seed=SEEDS[name] + 100)
    mi = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 0], np.int32)
    on2 = mi.astype(bool)
    st[on2], wps[on2], cnt[on2] = st2[on2], wps2[on2], cnt2[on2]
    return st, wps, cnt, np.stack([np.asarray(occ), occ2]), mi


def actions(name, steps=3, scale=0.3):
    """The free-running steps' actions [steps][E][N][2], float32.  |a| <= 0.3: three steps move an agent at
    most 0.6 + 1.2 + 1.8 = 3.6 m from its start (a free cell's centre), so it stays outside the occupied
    cells -- a start inside a cell ties every ray that leaves it into the next cell bit for bit, which the
    comparison would have to excuse."""
    rng = np.random.default_rng(SEEDS[name] + 1000)
    return rng.uniform(-scale, scale, size=(steps, E, CASES[name][1], 2)).astype(np.float32)


def flown(start, acts, vmax, acc_max=8.0, dt=0.5):
    """Positions after the steps, by the kinematics of ATT/env:2627-2713 in numpy (from rest; close to the
    kernel's, not bit-equal: good for counting the rays a comparison would excuse)."""
    pos, vel = np.array(start, dtype=np.float64), np.zeros_like(start, dtype=np.float64)
    for a in acts:
        v = vel + a.astype(np.float64) * acc_max * dt
        sp = np.linalg.norm(v, axis=-1, keepdims=True)
        vel = np.where(sp >= vmax, v / np.maximum(sp, 1e-300) * vmax, v)
        pos = pos + vel * dt
    return pos
