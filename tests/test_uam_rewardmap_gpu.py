"""UAM reward map on the GPU (include/aac_uam_rmap.h, ``rewardmap.UamRewardMap``, ``aac_uam_reward_map``).

  1 replay    the map at (pos, pre_pos, pre-step top2) of every aircraft after a step, pushed through
              ``rewardmap.uam_step_rows``, is the step's terms, reward, done and mask bit for bit; the OR of an
              env's bbc rows is its bbc; ``rays`` is the step's radar and slot 11 its minimum.  Threshold batches
              at N = 3, 5, 16, the seeded random batch (E = 64) and N = 17 (the step's sequential walk)
  2 displaced seeded points aimed at features against tests/uam_rewardmap_ref.py: integers exact, floats 1e-9
  3 grid      the default 50 x 50 grid for env 0 and the last env of an E = 3 handle against the restatement
  4 rmin / prev2
  5 shapes    M = 1 and around one and two workgroups' rows into canary arenas; last env, last aircraft;
              ``terms`` / ``rays`` left out
  6 read-only state untouched; a stepped env stays bit-identical to a twin without map launches; graph replay
  7 errors    of the C entry
  8 facade    ``ss_reward_Mar_changeskin(xy=...)``
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import uam_rewardmap_ref as M
from tests import uam_thresholds as T
from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("pos", "vel", "pre_pos", "pre_vel", "goal", "start", "heading", "reach", "clouds", "cloud_kind", "cloud_tgt",
         "step", "top2")
KEYS = M.KEYS
FLOATS = ("reward", "terms", "rays")
ROWS = 14           # AAC_UAM_RMAP_ROWS: rows per workgroup


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(a.view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))
    return np.array_equal(a, b)


def _np_state(env):
    return {k: _np(v) for k, v in env.get_state().items()}


def _env_from(st, N, **kw):
    from multi_agent_aac_amd import uam
    env = uam.BatchedUAM(st["pos"].shape[0], N, **kw)
    env.reset(st["pos"], st["goal"], st["cloud_kind"])
    env.set_state(**{k: st[k] for k in STATE})
    return env


def _rmap(env):
    from multi_agent_aac_amd.rewardmap import UamRewardMap
    return UamRewardMap.for_uam(env)


def _all_rows(E, N):
    return np.repeat(np.arange(E, dtype=np.int32), N), np.tile(np.arange(N, dtype=np.int32), E)


# ------------------------------------------------------------------ 1: replay identity
def _replay(pre, N, act):
    """One step from ``pre`` with a terms buffer, then the map over every (e, i): asserts the identity and
    returns the per-env blocks (rows, flags, mask) of map rows."""
    from multi_agent_aac_amd.rewardmap import uam_step_rows
    env = _env_from(pre, N)
    E = env.E
    top2 = _np(env.get_state()["top2"])
    assert np.array_equal(top2, pre["top2"])
    terms = env.use_terms_buffer(torch.full((E, N, 12), float("nan"), dtype=torch.float64, device=DEV))
    env.step(torch.as_tensor(act, dtype=torch.float64, device=DEV))
    post, b = _np_state(env), env.bufs
    rm = _rmap(env)
    ei, ai = _all_rows(E, N)
    rm.at(post["pos"].reshape(-1, 2), env=ei, agent=ai, pre=post["pre_pos"].reshape(-1, 2), prev2=top2.reshape(-1, 2))
    got = {k: v.reshape(E, N, *v.shape[1:]) for k, v in rm.read().items()}
    want_t, want_r = _np(terms), _np(b.reward)
    assert not np.isnan(want_t).any()
    blocks = []
    for e in range(E):
        rows, reward = uam_step_rows(got["terms"][e], got["flags"][e], got["mask"][e])
        assert _bits(rows, want_t[e]), (e, rows - want_t[e])
        assert _bits(reward, want_r[e]), (e, reward, want_r[e])
        blocks.append((got["terms"][e], got["flags"][e], got["mask"][e]))
    assert np.array_equal(got["done"], _np(b.done)) and np.array_equal(got["mask"], _np(b.mask))
    assert np.array_equal(got["bbc"].max(axis=1), _np(b.bbc))
    assert _bits(got["rays"], _np(b.radar))
    assert _bits(got["terms"][..., 11], _np(b.radar).min(axis=-1))
    return got, blocks


@pytest.mark.parametrize("N", [3, 5, 16])
def test_replay_identity_on_thresholds(native_lib, N):
    pre = T.build(N).state()
    got, _ = _replay(pre, N, np.zeros((len(pre["pos"]), N, 2)))
    assert set(np.unique(M.kinds(got["mask"]))) == {0, 1, 2, 3, 4}
    assert (got["flags"] & M.CRASH_DBL).any() and (got["flags"] & M.BAND_DBL).any()


def test_replay_identity_on_random_batch(native_lib):
    pre, act = M.random_batch(64, 5)
    got, blocks = _replay(pre, 5, act)
    M.assert_coverage(got["mask"], got["flags"], blocks)


def test_replay_identity_n17(native_lib):
    pre, act = M.random_batch(4, 17)
    _replay(pre, 17, act)


# ------------------------------------------------------------------ 2, 3: against the restatement
def _cmp(got, want, tag):
    for k in KEYS:
        if k in FLOATS:
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=T.RTOL_FLOAT, err_msg=f"{tag} {k}")
        else:
            assert np.array_equal(got[k], want[k]), (tag, k, np.argwhere(got[k] != want[k])[:5])


@functools.lru_cache(maxsize=None)
def _displaced_ref():
    N = 5
    st, _ = M.random_batch(20, N, seed=1)
    pts, ei, ai, pre = M.feature_points(st, N, seed=3, per=1)
    return st, N, pts, ei, ai, pre, M.rows(st, N, pts, env=ei, agent=ai, pre=pre)


def test_displaced_points_against_restatement(native_lib):
    st, N, pts, ei, ai, pre, want = _displaced_ref()
    M.assert_coverage(want["mask"], want["flags"])
    rm = _rmap(_env_from(st, N))
    got = rm.read(rm.at(pts, env=ei, agent=ai, pre=pre))
    _cmp(got, want, "displaced")
    M.assert_coverage(got["mask"], got["flags"])
    # pre="live" is the subject's live position: the bound rows were built with it
    live = rm.read(rm.at(pts, env=ei, agent=ai, pre="live"))
    same = (pre == st["pos"][ei, ai]).all(axis=1)
    assert same.any() and not same.all()
    for k in KEYS:
        assert _bits(live[k][same], got[k][same]), k


def test_default_grid_against_restatement(native_lib):
    N = 3
    st, _ = M.random_batch(3, N, seed=2)
    rm = _rmap(_env_from(st, N))
    for e in (0, 2):
        X, Y, out = rm.grid(env=e)
        assert X.shape == Y.shape == (50, 50) and out["terms"].shape == (50, 50, 12) and out["rays"].shape == (50, 50, 18)
        assert X[0, 0] == 0.0 and X[0, -1] == 40.0 and Y[-1, 0] == 40.0
        got = {k: v.reshape(2500, *v.shape[2:]) for k, v in rm.read(out).items()}
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
        _cmp(got, M.rows(st, N, pts, env=e), f"grid env {e}")
        assert len(np.unique(M.kinds(got["mask"]))) >= 3


# ------------------------------------------------------------------ 4: rmin / prev2
def _collision_state():
    """N = 3 in open space: aircraft 1 sits 0.6 m right of the test point (9, 20), aircraft 2 far away."""
    st, _ = M.random_batch(1, 3, seed=5)
    st = {k: v.copy() for k, v in st.items()}
    st["pos"][0] = [(12.0, 24.0), (9.6, 20.0), (30.0, 33.0)]
    st["goal"][0] = [(38.0, 3.0), (38.0, 3.0), (3.0, 37.0)]
    st["start"][0] = st["pos"][0] - 1.0
    st["reach"][0] = 0
    st["clouds"][0] = [(35.0, 30.0), (35.0, 5.0)]
    st["top2"][0] = [(1, 2), (0, 2), (0, 1)]
    return st


def test_given_rmin_and_prev2(native_lib):
    st = _collision_state()
    rm = _rmap(_env_from(st, 3))
    pts = np.array([[9.0, 20.0], [9.0, 26.0], [30.0, 30.0]])
    rmin = np.array([0.75, 3.0000000000000004, 7.5])
    out = rm._alloc(3)
    out["rays"].view(torch.int64).fill_(0x7FF8A5A5A5A5A5A5)
    got = rm.read(rm.at(pts, rmin=rmin, out=out))
    assert (_np(out["rays"]).view(np.int64) == 0x7FF8A5A5A5A5A5A5).all()          # a given rmin: rays unwritten
    assert _bits(got["terms"][:, 11], rmin)
    want = M.rows(st, 3, pts, rmin=rmin)
    for k in KEYS[:-1]:
        (np.testing.assert_allclose(got[k], want[k], rtol=0, atol=T.RTOL_FLOAT) if k in FLOATS
         else np.testing.assert_array_equal(got[k], want[k]))
    assert got["terms"][1, 5] < 0 and got["terms"][2, 5] == 0          # the penalty follows the given minimum
    # the hand-built collision row: live top2 names the collider; so does (1, 255); (2, 255) does not
    assert got["mask"][0] & 4 and got["mask"][0] & 32 and got["bbc"][0].tolist() == [0, 0, 1, 1]
    p = pts[:1]
    named = rm.read(rm.at(p, prev2=np.array([[1, 255]], np.uint8)))
    other = rm.read(rm.at(p, prev2=np.array([[2, 255]], np.uint8)))
    assert named["mask"][0] & 32 and named["bbc"][0, 3] == 1 and named["flags"][0] & M.PREV_TWO
    assert not other["mask"][0] & 32 and other["bbc"][0, 3] == 0 and not other["flags"][0] & M.PREV_TWO
    assert int(other["mask"][0]) == int(named["mask"][0]) & ~32 and _bits(other["terms"], named["terms"])


# ------------------------------------------------------------------ 5: shapes and bounds
class ByteArena:
    """tests/arena.py's idea for uint8 outputs: one allocation of 0xA5 (no output value has it), regions with
    gaps and guards; ``check`` wants every region byte written and every other byte untouched."""
    CANARY, GAP = 0xA5, 64

    def __init__(self, sizes):
        self.off, n = {}, 4096
        for k, s in sizes.items():
            self.off[k] = (n, s)
            n += s + self.GAP
        self.buf = torch.full((n + 4096,), self.CANARY, dtype=torch.uint8, device=DEV)

    def ptr(self, k):
        return self.buf.data_ptr() + self.off[k][0]

    def get(self, k):
        o, s = self.off[k]
        return _np(self.buf[o:o + s])

    def check(self):
        cur = _np(self.buf)
        inside = np.zeros(len(cur), bool)
        for k, (o, s) in self.off.items():
            inside[o:o + s] = True
            assert (cur[o:o + s] != self.CANARY).all(), (k, int((cur[o:o + s] == self.CANARY).sum()))
        assert (cur[~inside] == self.CANARY).all(), np.flatnonzero((cur != self.CANARY) & ~inside)[:5]


@pytest.mark.parametrize("Mrows", [1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS - 1, 2 * ROWS, 2 * ROWS + 1])
def test_shapes_into_canary_arenas(native_lib, Mrows):
    from multi_agent_aac_amd import _native, uam
    N = 5
    st, _ = M.random_batch(20, N, seed=1)
    env = _env_from(st, N)
    rm = _rmap(env)
    rng = np.random.default_rng(Mrows)
    # the last env and the last aircraft in every launch; the rest seeded
    ei = rng.integers(0, env.E, Mrows).astype(np.int32)
    ai = rng.integers(0, N, Mrows).astype(np.int32)
    ei[-1], ai[-1] = env.E - 1, N - 1
    pts = st["pos"][ei, (ai + 1) % N] + rng.uniform(-3, 3, (Mrows, 2))
    want = rm.read(rm.at(pts, env=ei, agent=ai))
    want = {k: v.copy() for k, v in want.items()}
    ar = Arena(64 * Mrows + 4096, torch.float64, DEV, max_ld=32)
    P = ar.take(Mrows, 2, data=torch.from_numpy(pts))
    rew, terms, rays = ar.take(Mrows, 1), ar.take(Mrows, 12), ar.take(Mrows, 18)
    by = ByteArena(dict(mask=Mrows, done=Mrows, bbc=4 * Mrows, flags=Mrows))
    idx = torch.as_tensor(np.concatenate([ei, ai]), device=DEV)
    vp = ctypes.c_void_p

    def launch(t, r):
        o = _native.UamRmapOut(rew.ptr, t, by.ptr("mask"), by.ptr("done"), by.ptr("bbc"), by.ptr("flags"), r)
        uam._chk(uam.lib().aac_uam_reward_map(env._h, vp(P.ptr), None, vp(idx.data_ptr()), vp(idx.data_ptr() + 4 * Mrows),
                                              None, None, Mrows, ctypes.byref(o), None), "map")
        torch.cuda.synchronize()

    launch(terms.ptr, rays.ptr)
    ar.check(writable=[rew, terms, rays])
    by.check()
    got = dict(reward=rew.get().numpy()[:, 0], terms=terms.get().numpy(), rays=rays.get().numpy(),
               mask=by.get("mask"), done=by.get("done"), bbc=by.get("bbc").reshape(-1, 4), flags=by.get("flags"))
    for k in KEYS:
        assert _bits(got[k], want[k]), k
    # terms and rays left out: the other outputs do not change, nothing else is written
    ar.freeze([terms, rays])
    rew.view.view(torch.int64).fill_(ar.canary)
    by.buf.fill_(by.CANARY)
    launch(None, None)
    ar.check(writable=[rew])
    by.check()
    assert _bits(rew.get().numpy()[:, 0], want["reward"]) and np.array_equal(by.get("mask"), want["mask"])


# ------------------------------------------------------------------ 6: read-only, capturable
def test_read_only_and_capturable(native_lib):
    from multi_agent_aac_amd import graphs
    N = 5
    st, act = M.random_batch(64, N)
    env, twin = _env_from(st, N, tdcpa=True), _env_from(st, N, tdcpa=True)
    from multi_agent_aac_amd import uam
    for h in (env, twin):       # envs that finish are replaced: the map must not disturb the resets either
        h.set_bank(uam.build_bank(128, N, seed=11), seed=4)
    rm = _rmap(env)
    ei, ai = _all_rows(env.E, N)
    d = lambda a: torch.as_tensor(a, device=DEV)          # noqa: E731
    pd, ed, ad = d(st["pos"].reshape(-1, 2) + 0.25), d(ei), d(ai)
    before = _np_state(env)
    out = rm.at(pd, env=ed, agent=ad, pre="live")
    eager = {k: v.copy() for k, v in rm.read().items()}
    after = _np_state(env)
    for k in before:
        assert _bits(before[k], after[k]), k
    rng = np.random.default_rng(8)
    for s in range(4):
        a = d(act if s == 0 else rng.uniform(-1, 1, act.shape))
        rm.at(pd, env=ed, agent=ad)
        oa, ob = env.step(a), twin.step(a)
        rm.at(pd, env=ed, agent=ad, pre="live")
        for k, v in vars(oa).items():
            if torch.is_tensor(v):
                assert _bits(_np(v), _np(getattr(ob, k))), (s, k)
        sa, sb = _np_state(env), _np_state(twin)
        for k in sa:
            assert _bits(sa[k], sb[k]), (s, k)
        if s == 1:
            env.auto_reset(oa.env_done)
            twin.auto_reset(ob.env_done)
    # a captured launch, replayed after a further step, gives the rows of the new state
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        rm.at(pd, env=ed, agent=ad)
    env.step(d(rng.uniform(-1, 1, act.shape)))
    fresh = {k: v.copy() for k, v in rm.read(rm.at(pd, env=ed, agent=ad, out=rm._alloc(len(ei)))).items()}
    assert not _bits(fresh["terms"], eager["terms"])
    for t in out.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    replay = rm.read(out)
    for k in KEYS:
        assert _bits(replay[k], fresh[k]), k


# ------------------------------------------------------------------ 7: error returns
def test_error_returns(native_lib):
    from multi_agent_aac_amd import _native, uam
    st = _collision_state()
    env = _env_from(st, 3)
    rm = _rmap(env)
    with pytest.raises(ValueError):
        rm.at(np.zeros((0, 2)))
    with pytest.raises(ValueError):
        rm.at(np.zeros((4, 2)), env=1)
    with pytest.raises(ValueError):
        rm.at(np.zeros((4, 2)), prev2=np.zeros((3, 2), np.uint8))
    with pytest.raises(TypeError):
        _rmap(object())
    o = rm._alloc(4)
    L = uam.lib()
    pts = torch.zeros(5, 2, dtype=torch.float64, device=DEV)
    P = _native.UamRmapOut(*[o[k].data_ptr() for k in KEYS])
    p = ctypes.c_void_p(pts.data_ptr())
    off = ctypes.c_void_p(pts.data_ptr() + 4)
    assert L.aac_uam_reward_map(env._h, p, None, None, None, None, None, 0, ctypes.byref(P), None) == -1
    assert b"M out of range" in L.aac_uam_last_error()
    assert L.aac_uam_reward_map(env._h, None, None, None, None, None, None, 4, ctypes.byref(P), None) == -1
    assert L.aac_uam_reward_map(None, p, None, None, None, None, None, 4, ctypes.byref(P), None) == -1
    assert L.aac_uam_reward_map(env._h, p, None, None, None, None, None, 4, None, None) == -1
    for args in ((off, None, None), (p, off, None), (p, None, off)):        # points, pre, rmin
        assert L.aac_uam_reward_map(env._h, args[0], args[1], None, None, args[2], None, 4, ctypes.byref(P), None) == -1
        assert b"8-byte aligned" in L.aac_uam_last_error()
    for k in ("reward", "terms", "rays"):
        Q = _native.UamRmapOut(*[o[j].data_ptr() + (4 if j == k else 0) for j in KEYS])
        assert L.aac_uam_reward_map(env._h, p, None, None, None, None, None, 4, ctypes.byref(Q), None) == -1, k
    for k in ("reward", "mask", "done", "bbc", "flags"):
        Q = _native.UamRmapOut(*[None if j == k else o[j].data_ptr() for j in KEYS])
        assert L.aac_uam_reward_map(env._h, p, None, None, None, None, None, 4, ctypes.byref(Q), None) == -1, k
        assert b"required" in L.aac_uam_last_error()
    torch.cuda.synchronize()
    assert all(not _np(v).any() for v in o.values())           # no failed call launched anything


# ------------------------------------------------------------------ 8: facade
def test_facade_map_mode(native_lib):
    from multi_agent_aac_amd import uam
    N = 4
    sim = uam.env_simulator(seed=3)
    sim.create_world(N, 2, 0.95, 0.01, 10, 1, 0.1, 1, 40, 1.0, (-0.5, 0.5))
    sim.reset_world_change_skin(N)
    rng = np.random.default_rng(2)
    for _ in range(3):
        sim.step(rng.uniform(-1, 1, (N, 2)))
    usual = sim.ss_reward_Mar_changeskin(0, [None] * N, [[] for _ in range(N)])
    pos0 = sim.all_agents[0].pos.copy()
    before = _np_state(sim._env)
    held = float(_np(sim._env.bufs.radar)[0, 0].min())
    other = before["pos"][0, 1]
    for xy in ((float(other[0]) - 0.7, float(other[1])), (20.0, 20.0), (5.0, 33.0)):
        rec = [None] * N
        reward, done, check_goal, rec_out, hold, coll, bbc = sim.ss_reward_Mar_changeskin(0, rec, None, xy=xy)
        rm = _rmap(sim._env)
        row = rm.read(rm.at(np.array([xy]), rmin=held))
        assert len(reward) == 1 and len(done) == 1 and len(check_goal) == N and len(bbc) == 4
        assert _bits(np.float64(reward[0]), row["reward"][0]) and done[0] == bool(row["done"][0])
        assert check_goal == [bool(row["mask"][0] & 16)] + [False] * (N - 1)
        assert bbc == [bool(v) for v in row["bbc"][0]] and rec_out[0] == [0, float(row["reward"][0])]
        assert _bits(sim.last_map_row["terms"], row["terms"][0]) and sim.last_map_row["terms"][11] == held
    assert np.array_equal(sim.all_agents[0].pos, pos0)
    after = _np_state(sim._env)
    for k in before:
        assert _bits(before[k], after[k]), k
    again = sim.ss_reward_Mar_changeskin(0, [None] * N, [[] for _ in range(N)], xy=(None, None))
    assert repr(again) == repr(usual)
