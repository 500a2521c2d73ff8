"""The exploration maps' bin rule (include/aac_visits.h) as restated in tests/visits_ref.py against
``np.histogram2d`` with explicit edges, and the binding's struct sizes against the header.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import visits_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# range and bins of an axis: the ATT bound (x, y), the UAM bound, the action range
AXES = {"att_x": (455.0, 680.0, 50), "att_y": (255.0, 385.0, 50), "uam": (0.0, 40.0, 50), "act": (-1.0, 1.0, 20),
        "att_x_7": (455.0, 680.0, 7), "act_32": (-1.0, 1.0, 32), "act_3": (-1.0, 1.0, 3)}


def edge_samples(e):
    """Every edge and the doubles 1 ulp either side of it."""
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])


@pytest.mark.parametrize("axis", sorted(AXES))
def test_edges_are_linspace(axis):
    lo, hi, G = AXES[axis]
    e = visits_ref.edges(lo, hi, G)
    assert e.tobytes() == np.linspace(lo, hi, G + 1).tobytes()
    assert np.all(np.diff(e) > 0) and e[0] == lo and e[-1] == hi


@pytest.mark.parametrize("pair", [("att_x", "att_y"), ("uam", "uam"), ("act", "act"), ("att_x_7", "act_3"),
                                  ("act_32", "act_32")])
def test_restatement_equals_histogram2d(pair):
    (x0, x1, GX), (y0, y1, GY) = AXES[pair[0]], AXES[pair[1]]
    ex, ey = visits_ref.edges(x0, x1, GX), visits_ref.edges(y0, y1, GY)
    rng = np.random.default_rng([GX, GY])
    # random rows a little wider than the range, then every edge +- 1 ulp of one axis against a sweep of
    # the other, then float32 values (an action's 0.1f is not the double 0.1)
    xs = [rng.uniform(x0 - 0.05 * (x1 - x0), x1 + 0.05 * (x1 - x0), 20000)]
    ys = [rng.uniform(y0 - 0.05 * (y1 - y0), y1 + 0.05 * (y1 - y0), 20000)]
    sx, sy = edge_samples(ex), edge_samples(ey)
    xs += [sx, rng.uniform(x0, x1, len(sy)), np.resize(sx, max(len(sx), len(sy)))]
    ys += [rng.uniform(y0, y1, len(sx)), sy, np.resize(sy, max(len(sx), len(sy)))]
    f = ex.astype(np.float32).astype(np.float64)
    xs.append(f)
    ys.append(np.resize(ey.astype(np.float32).astype(np.float64), len(f)))
    x, y = np.concatenate(xs), np.concatenate(ys)
    got, outside = visits_ref.hist2d(x, y, ex, ey)
    want = np.histogram2d(x, y, bins=[ex, ey])[0]
    assert np.array_equal(got, want.astype(np.int64))
    assert got.sum() + outside == len(x) and outside > 0
    # the closed last bin, the open first edge below, and values no bin takes
    b = visits_ref.bins(np.array([x0, x1, np.nextafter(x0, -np.inf), np.nextafter(x1, np.inf), np.nan, np.inf, -np.inf]), ex)
    assert list(b) == [0, GX - 1, -1, -1, -1, -1, -1]


def test_float_action_is_binned_as_its_double():
    """edge[11] of the action axis is -1 + 11 * 0.1 = 0.10000000000000009: the double 0.1 lies below it,
    float32(0.1) = 0.10000000149 above it."""
    e = visits_ref.edges(-1.0, 1.0, 20)
    f = np.float64(np.float32(0.1))
    assert 0.1 < e[11] < f
    assert visits_ref.bins([0.1], e)[0] == 10 and visits_ref.bins([f], e)[0] == 11


def test_reference_accumulate_rule():
    r = visits_ref.VisitsRef(2, 4, 3, 2, (0.0, 4.0), (0.0, 3.0))
    pos = np.array([[[0.5, 0.5], [4.0, 3.0]], [[5.0, 1.0], [1.0, np.nan]], [[1.0, 1.0], [1.0, 1.0]],
                    [[2.0, 2.0], [2.0, 2.0]]])
    act = np.array([[[-1.0, 1.0], [0.0, 0.0]], [[2.0, 0.0], [0.5, -0.5]], [[0.0, 0.0], [0.0, 0.0]],
                    [[0.0, 0.0], [0.0, 0.0]]], dtype=np.float32)
    r.accumulate(pos, act, episode=[1, 2, 1, 1], explore_until=1, map_idx=[0, 1, 2, 0], sel=[1, 1, 1, 0])
    assert r.cnt.tolist() == [[2, 0, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0], [2, 2, 1, 0]]
    assert r.pos.sum() == 2 and r.pos[0, 0, 0] == 1 and r.pos[0, 3, 2] == 1
    assert r.act[0].tolist() == [[0, 1], [0, 1]] and r.act[1].tolist() == [[0, 0], [1, 0]]


def test_struct_sizes_match_the_header():
    """The .hip static_asserts sizeof(struct) == the header's constants; the binding must agree."""
    from multi_agent_aac_amd import _native, visits
    src = open(os.path.join(ROOT, "include", "aac_visits.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (AAC_VISITS_\w+) (\d+)", src)}
    assert ctypes.sizeof(_native.VisitsState) == const["AAC_VISITS_STATE_BYTES"]
    assert ctypes.sizeof(_native.VisitsStep) == const["AAC_VISITS_STEP_BYTES"]
    hip = open(os.path.join(ROOT, "multi_agent_aac_amd", "csrc", "aac_visits.hip")).read()
    for name, typ in (("STATE", "state"), ("STEP", "step")):
        assert re.search(r"static_assert\(sizeof\(aac_visits_%s\) == AAC_VISITS_%s_BYTES" % (typ, name), hip), name
    assert (const["AAC_VISITS_MAX_A"], const["AAC_VISITS_MAX_G"], const["AAC_VISITS_CHUNK"]) == \
        (visits.MAX_A, visits.MAX_G, visits.CHUNK)
    assert const["AAC_VISITS_COUNTERS"] == len(visits.COUNTERS) == visits_ref.COUNTERS
    for lo, hi, G in AXES.values():
        assert visits.edges(lo, hi, G).tobytes() == visits_ref.edges(lo, hi, G).tobytes()
