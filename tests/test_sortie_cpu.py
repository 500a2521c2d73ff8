"""The sortie rule (include/aac_sortie.h) as restated in tests/sortie_ref.py against a direct
transcription of the definition (UAM/util:53-68: the sum of the step-to-step distances, then the start
segment, then the margin, over the straight origin-destination distance) on hand-made paths, the class
precedence, the degenerate case, and the binding's struct sizes against the header.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np

import sortie_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATT = sortie_ref.BITS_ENV
UAM = sortie_ref.BITS_UAM


def definition_ratio(traj, ini, goal, margin):
    """obtain_euclidean_dist_list_all_AC for one aircraft: traj[k] is its position after step k + 1."""
    total = 0
    for k in range(1, len(traj)):
        total = total + np.linalg.norm(np.array(traj[k]) - np.array(traj[k - 1]))
    total = total + np.linalg.norm(np.array(traj[0]) - np.array(ini)) + margin
    return total / np.linalg.norm(np.array(goal) - np.array(ini))


def play(paths, starts, goals, masks, margin, bits, episode_length=50, done_last=None, quota=None):
    """One env, N aircraft: paths[i][k] the position of aircraft i after step k + 1, masks[k][i] the mask
    byte of step k + 1; the episode ends with the last step."""
    N, T = len(paths), len(paths[0])
    ref = sortie_ref.SortieRef(1, N, episode_length, margin, **bits)
    start, goal = np.array([starts], dtype=np.float64), np.array([goals], dtype=np.float64)
    for k in range(T):
        pos = np.array([[paths[i][k] for i in range(N)]], dtype=np.float64)
        last = k == T - 1
        done = np.array([done_last if last and done_last is not None else [0] * N], dtype=np.uint8)
        ref.accumulate(pos, start, goal, done, np.array([masks[k]], dtype=np.uint8), np.array([last], dtype=np.uint8),
                       quota=quota)
    return ref


def test_straight_flight_ratio_is_d_plus_margin_over_d():
    d, T = 12.0, 6
    for margin in (0.0, 5.0):
        path = [(1.0 + d * (k + 1) / T, 2.0) for k in range(T)]
        masks = [[0]] * (T - 1) + [[1 << UAM["goal_bit"]]]
        ref = play([path], [(1.0, 2.0)], [(1.0 + d, 2.0)], masks, margin, UAM)
        assert ref.cnt["reached"] == 1 and ref.cnt["sorties"] == 1 and ref.cnt["degenerate"] == 0
        assert ref.ratios == [definition_ratio(path, (1.0, 2.0), (1.0 + d, 2.0), margin)]
        assert ref.ratios[0] == (d + margin) / d
        assert ref.rows[0][4:6] == (T, T) and ref.cnt["reach_step_sum"] == T


def test_restatement_equals_the_definition_on_random_paths():
    rng = np.random.default_rng(11)
    N, T = 4, 9
    starts, goals = rng.uniform(0, 40, (N, 2)), rng.uniform(0, 40, (N, 2))
    paths = rng.uniform(0, 40, (N, T, 2))
    masks = [[0] * N for _ in range(T)]
    for i in range(N):
        masks[rng.integers(0, T)][i] = 1 << ATT["goal_bit"]      # reached at some step, flies on afterwards
    ref = play(paths.tolist(), starts.tolist(), goals.tolist(), masks, 5.0, ATT)
    want = [definition_ratio(paths[i].tolist(), starts[i], goals[i], 5.0) for i in range(N)]
    assert [float(r).hex() for r in ref.ratios] == [float(w).hex() for w in want]
    assert ref.cnt["reached"] == N == ref.cnt["sorties"] and ref.cnt["episodes"] == 1
    sums, n = ref.sums()
    assert n == N and sums["ratio_min"] == min(want) and sums["ratio_max"] == max(want)


def test_parked_aircraft_adds_nothing():
    T = 5
    path = [(3.0, 4.0)] * T
    masks = [[0]] * (T - 1) + [[1 << ATT["goal_bit"]]]
    ref = play([path], [(3.0, 4.0)], [(6.0, 8.0)], masks, 0.0, ATT)
    assert ref.rows[0][6:] == (0.0, 5.0, 0.0) and ref.ratios == [0.0]
    # parked for three steps, then one hop: only the hop counts
    path = [(3.0, 4.0)] * 3 + [(6.0, 8.0)] * 2
    ref = play([path], [(3.0, 4.0)], [(6.0, 8.0)], masks, 0.0, ATT)
    assert ref.ratios == [1.0]


def test_class_precedence():
    for bits in (ATT, UAM):
        b, o, d, g = (1 << bits[k] for k in ("bound_bit", "obstacle_bit", "drone_bit", "goal_bit"))
        other = 0xFF & ~(b | o | d | g)
        flags = [b | o | d | g, o | d | g, d | g, g, other, 0, b | g, o | g | other, d | other]
        want = [0, 1, 2, 3, 4, 4, 0, 1, 2]
        assert [sortie_ref.classify(f, bits["bound_bit"], bits["obstacle_bit"], bits["drone_bit"], bits["goal_bit"])
                for f in flags] == want
        # flags gathered over several steps of one episode: goal at step 1, drone at step 2, bound at step 3
        N = 3
        masks = [[g, g, 0], [d, 0, 0], [b, 0, 0]]
        paths = [[(1.0 + k, 1.0) for k in range(3)]] * N
        ref = play(paths, [(0.0, 1.0)] * N, [(9.0, 1.0)] * N, masks, 0.0, bits, done_last=[1, 0, 0])
        assert [r[3] for r in ref.rows] == [0, 3, 4]
        assert (ref.cnt["bound"], ref.cnt["reached"], ref.cnt["idle"], ref.cnt["sorties"]) == (1, 1, 1, 3)
        assert [r[5] for r in ref.rows] == [1, 1, 0] and ref.cnt["reach_step_sum"] == 1
        assert ref.collide_hist[3] == 1 and ref.collide_hist.sum() == 1


def test_zero_straight_distance_is_degenerate():
    g = 1 << UAM["goal_bit"]
    ref = play([[(1.0, 1.0), (2.0, 1.0)], [(1.0, 1.0), (2.0, 1.0)], [(1.0, 1.0), (math.nan, 1.0)]],
               [(0.0, 0.0), (0.0, 0.0), (0.0, 0.0)], [(0.0, 0.0), (3.0, 4.0), (3.0, 4.0)], [[0, 0, 0], [g, g, g]], 5.0, UAM)
    assert ref.cnt["reached"] == 3 and ref.cnt["degenerate"] == 2 and len(ref.ratios) == 1
    assert math.isnan(ref.rows[0][8]) and ref.rows[0][7] == 0.0 and math.isnan(ref.rows[2][8])
    assert ref.rows[1][8] == ((1.0 + math.sqrt(2.0)) + 5.0) / 5.0


def test_collision_condition_and_quota():
    # a timeout (len == episode_length + 1) with done set is no collision; a full-length episode neither
    for T, ep, hit in ((4, 3, 0), (3, 3, 0), (2, 3, 1)):
        ref = play([[(float(k), 0.0) for k in range(T)]], [(0.0, 0.0)], [(9.0, 0.0)], [[0]] * T, 0.0, ATT,
                   episode_length=ep, done_last=[1])
        assert ref.collide_hist.sum() == hit and (not hit or ref.collide_hist[T] == 1)
    ref = play([[(1.0, 0.0)]], [(0.0, 0.0)], [(9.0, 0.0)], [[0]], 0.0, ATT, quota=[0])
    assert ref.cnt["sorties"] == 0 and ref.run_len[0] == 0 and ref.last_pos.sum() == 0


def test_struct_sizes_match_the_header():
    """The .hip static_asserts sizeof(struct) == the header's constants; the binding must agree."""
    from multi_agent_aac_amd import _native, sorties
    src = open(os.path.join(ROOT, "include", "aac_sortie.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (AAC_SORTIE_\w+) (\d+)", src)}
    assert ctypes.sizeof(_native.SortieState) == const["AAC_SORTIE_STATE_BYTES"]
    assert ctypes.sizeof(_native.SortieStep) == const["AAC_SORTIE_STEP_BYTES"]
    assert sorties.ROW.itemsize == sortie_ref.ROW.itemsize == const["AAC_SORTIE_ROW_BYTES"]
    assert sorties.ROW == sortie_ref.ROW
    hip = open(os.path.join(ROOT, "multi_agent_aac_amd", "csrc", "aac_sortie.hip")).read()
    for name, typ in (("STATE", "state"), ("STEP", "step"), ("ROW", "row")):
        assert re.search(r"static_assert\(sizeof\(aac_sortie_%s\) == AAC_SORTIE_%s_BYTES" % (typ, name), hip), name
    assert (const["AAC_SORTIE_EPW"], const["AAC_SORTIE_FIELDS"]) == (sorties.EPW, sorties.FIELDS)
    assert sorties.COUNTERS == sortie_ref.COUNTERS and sorties.CLASSES == sortie_ref.CLASSES
    assert [const["AAC_SORTIE_" + c.upper()] for c in sorties.CLASSES] == list(range(5))
    assert sorties.BITS["env"] == sortie_ref.BITS_ENV and sorties.BITS["uam"] == sortie_ref.BITS_UAM
