"""Reward map, CPU side (include/aac_rmap.h; tests/rewardmap_ref.py): the equivalence the GPU tests lean
on -- at rest, a zero-action step's ``ss_reward`` rows are the map's rows at the landing positions, bit for
bit -- on the exact-threshold batches; the restatement leaves its input alone; the rows cover every mask
bit and reward kind; the ctypes struct follows the header."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

from tests import rewardmap_cases as C
from tests import rewardmap_ref as RM
from tests import terms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _landing(variant, st, occ):
    """Where a zero-action step of the restatement's env puts every agent of the batch."""
    E, N = st["pos"].shape[:2]
    out = np.zeros((E, N, 2))
    for e in range(E):
        env = R.wgru_env(st, e, occ) if variant == "wgru" else R.att_env(st, e, occ)
        env.step(np.zeros((N, 2)))
        for i in range(N):
            out[e, i] = env.all_agents[i].pos
    return out


def _equivalence(variant, st, occ, envs=None):
    """``envs``: the envs compared (None: all) -- every agent of each."""
    if envs is not None:
        st = {k: v[envs] for k, v in st.items()}
    E, N = st["pos"].shape[:2]
    rest = C.at_rest(st, _landing(variant, st, occ))
    ei, ai = C.all_rows(E, N)
    got = RM.rows(variant, rest, occ, rest["pos"].reshape(-1, 2), ei, ai)
    for e in range(E):
        env = R.wgru_env(rest, e, occ) if variant == "wgru" else R.att_env(rest, e, occ)
        env.step(np.zeros((N, 2)))
        for i in range(N):
            ag = env.all_agents[i]
            assert np.array_equal(ag.pos, rest["pos"][e, i]) and np.array_equal(ag.pre_pos, rest["pos"][e, i]), (e, i)
        terms, own, done, masks = env.ss_reward_terms()
        sl = slice(e * N, (e + 1) * N)
        assert np.array_equal(_bits(terms), _bits(got["terms"][sl])), (variant, e)
        assert np.array_equal(_bits(own), _bits(got["reward"][sl])), (variant, e)
        assert [bool(d) for d in done] == [bool(d) for d in got["done"][sl]], (variant, e)
        assert list(masks) == got["mask"][sl].tolist(), (variant, e)
    return got


@pytest.mark.parametrize("N", C.ATT_CASES)
def test_att_step_at_rest_equals_the_map(N):
    st, occ = C.att_batch(N)
    # N = 3: every env; N = 5 (the fillers add nothing new): every second env, which keeps every family and ulp step
    got = _equivalence("att", st, occ, None if N == 3 else np.arange(0, st["pos"].shape[0], 2))
    C.coverage("att", got["mask"], got["terms"])
    assert got["bbc"][:, 0].any() and got["bbc"][:, 2].any() and got["bbc"][:, 3].any() and not got["bbc"][:, 1].any()


@pytest.mark.parametrize("N,W", [(3, 4), (3, 9), (3, 32)])
def test_wgru_step_at_rest_equals_the_map(N, W):
    st, occ = C.wgru_batch(N, W)
    np.testing.assert_array_equal(_landing("wgru", st, occ), st["post"])
    got = _equivalence("wgru", st, occ)
    C.coverage("wgru", got["mask"], got["terms"])
    assert got["bbc"][:, 0].any() and got["bbc"][:, 1].any() and not got["bbc"][:, 2:].any()


@pytest.mark.parametrize("variant", ["att", "wgru"])
def test_restatement_leaves_its_env_untouched(variant):
    st = C.moving_state(variant, 3, 9)
    occ = C.att_batch(3)[1]
    env = RM.prepare(R.wgru_env(st, 0, occ) if variant == "wgru" else R.att_env(st, 0, occ))
    before = copy.deepcopy(env)
    wp = st["wp"][0, 0, 0]
    a = RM.row(env, 0, wp, pre=(wp[0] - 1.0, wp[1]), rmin=3.0 if variant == "wgru" else None)
    b = RM.row(env, 0, wp, pre=(wp[0] - 1.0, wp[1]), rmin=3.0 if variant == "wgru" else None)
    assert a[3] & 16, "the point is on a waypoint: the search finds it (and, on the copy, pops it)"
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1:4] == b[1:4]
    for i in range(3):
        x, y = env.all_agents[i], before.all_agents[i]
        assert np.array_equal(x.pos, y.pos) and np.array_equal(x.pre_pos, y.pre_pos)
        assert x.goal == y.goal and x.waypoints == y.waypoints and x.reach_target == y.reach_target
        assert x.collide_wall_count == y.collide_wall_count and x.removed_goal == y.removed_goal
        assert np.array_equal(np.asarray(x.observableSpace), np.asarray(y.observableSpace))
    if variant == "wgru":
        assert a[0][11] == 3.0


def test_ctypes_struct_follows_the_header():
    from multi_agent_aac_amd import _native
    src = open(os.path.join(ROOT, "include", "aac_rmap.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} aac_rmap_out;", src, re.S).group(1)
    fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert fields == [n for n, _ in _native.RmapOut._fields_] == ["reward", "terms", "mask", "done", "bbc"]
    size = int(re.search(r"#define AAC_RMAP_OUT_BYTES (\d+)", src).group(1))
    assert ctypes.sizeof(_native.RmapOut) == size == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert "aac_env_reward_map" in _native.EXPORTS
    proto = re.search(r"int aac_env_reward_map\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(_native.lib().aac_env_reward_map.argtypes) if os.path.exists(_native.LIB_PATH) \
        else len(proto.split(",")) == 9
