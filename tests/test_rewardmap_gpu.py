"""Reward map on the GPU (include/aac_rmap.h, ``rewardmap.RewardMap``, ``aac_env_reward_map``).

  1 step      at rest on the exact-threshold landing positions the map's rows are the following zero-action
              step's rows bit for bit (terms, mask, done; bbc as the OR over the env's agents; reward == the
              slot sum) -- the rows the WGRU fix-up rewrites included, which pins the in-kernel exact radar
  2 motion    seeded random states with non-zero velocities against tests/rewardmap_ref.py (1e-12)
  3 grid      the reference's 50 x 50 grid on two envs of a two-map stack
  4 edges     M = 1, 255, 256, 257 into a canary arena; the last env, the last agent, no terms
  5 read-only state untouched; a stepped env stays bit-identical to a twin without map launches; graph replay
  6 rmin      NULL: slot 11 is the probe's exact minimum; a given value comes back unchanged
  7 facade    ``ss_reward(xy=...)``
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import rewardmap_cases as C
from tests import rewardmap_ref as RM
from tests import terms_ref as R
from tests import thresholds as T
from tests.arena import Arena

pytestmark = pytest.mark.gpu
ATOL = 1e-12          # the bar tests/test_terms_env_gpu.py holds the same slots to against the same restatement
KEYS = ("reward", "terms", "mask", "done", "bbc")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _env(variant, st, occ, W, map_idx=None, team=None):
    """A BatchedEnv holding a state dict (keys of tests/rewardmap_cases.py)."""
    from multi_agent_aac_amd.env import BatchedEnv
    E, N = st["pos"].shape[:2]
    kw = dict(variant="wgru") if variant == "wgru" else dict(team_reward=bool(team))
    env = BatchedEnv(E, N, occ, max_wp=W, **kw)
    env.set_state(pos=st["pos"], pre_pos=st["pre_pos"], vel=st["vel"], pre_vel=st["vel"], goal=st["goal"],
                  wp=st["wp"][:, :, :W], wp_cur=st["wp_cur"], wp_cnt=st["cnt"], reach=np.zeros((E, N), np.uint8),
                  wall=np.zeros((E, N), np.int32), step=np.zeros(E, np.int32),
                  map_idx=np.zeros(E, np.int32) if map_idx is None else map_idx, start=st["start"])
    return env


def _rmap(env):
    from multi_agent_aac_amd.rewardmap import RewardMap
    return RewardMap.for_env(env)


def _batch(variant, N, W):
    return C.wgru_batch(N, W) if variant == "wgru" else C.att_batch(N)


def _zero_step(env):
    out = env.alloc_buffers()
    env.step(torch.zeros(env.E, env.N, 2, device="cuda"), out=out)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1: against the step kernel
@pytest.mark.parametrize("variant,N,W", [("att", N, 32) for N in C.ATT_CASES] + [("wgru", N, W) for N, W in C.WGRU_CASES])
def test_map_rows_are_the_steps_rows(native_lib, variant, N, W):
    st, occ = _batch(variant, N, W)
    E = st["pos"].shape[0]
    scratch = _env(variant, st, occ, W)
    _zero_step(scratch)
    landing = _np(scratch.get_state()["pos"])
    if variant == "wgru":
        assert np.array_equal(landing, st["post"])
    rest = C.at_rest(st, landing)
    env = _env(variant, rest, occ, W)
    terms = env.use_terms_buffer()
    ei, ai = C.all_rows(E, N)
    rm = _rmap(env)
    rm.at(landing.reshape(-1, 2), env=ei, agent=ai)
    got = rm.read()
    out = _zero_step(env)
    assert np.array_equal(_np(env.get_state()["pos"]), landing) and np.array_equal(_np(env.get_state()["pre_pos"]), landing)
    t = _np(terms).reshape(E * N, 12)
    assert _same_bits(got["terms"], t), np.argwhere(_bits(got["terms"]) != _bits(t))[:4].tolist()
    assert _same_bits(got["mask"], _np(out.mask).reshape(-1))
    assert _same_bits(got["done"], _np(out.done).reshape(-1))
    assert _same_bits(got["bbc"].reshape(E, N, 4).max(axis=1), _np(out.bbc))
    assert np.array_equal(got["reward"], R.slot_sum(got["terms"]))
    assert np.array_equal(got["reward"].astype(np.float32), _np(out.reward).reshape(-1))      # per-agent rewards
    assert np.all(got["terms"][:, 7] == 0)
    C.coverage(variant, got["mask"], got["terms"])
    if variant == "wgru":
        most, cap = env.band_max()
        assert 40 <= most <= cap, (most, cap)          # rows the fix-up rewrote were among the compared ones


# ------------------------------------------------------------------ 2: against the restatement, in motion
def _motion_rows(variant, st, seed):
    E, N = st["pos"].shape[:2]
    rng = np.random.default_rng(seed)
    pts, ei, ai = [], [], []
    for e in range(E):
        for i in range(N):
            p = C.sample_points(st, e, i, rng, n_each=2)
            pts.append(p)
            ei += [e] * len(p)
            ai += [i] * len(p)
    return np.concatenate(pts), np.array(ei, np.int32), np.array(ai, np.int32)


def _against_ref(got, want, where):
    for k in ("mask", "done", "bbc"):
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(got[k] != want[k])[:4].tolist())
    err = np.abs(got["terms"] - want["terms"]).max(axis=0)
    print(where, "max |terms - ref| per slot:", " ".join(f"{R.NAMES[k]}={err[k]:.3g}" for k in range(12)),
          f"reward={np.abs(got['reward'] - want['reward']).max():.3g}")
    assert np.all(err <= ATOL), (where, err)
    assert np.all(np.abs(got["reward"] - want["reward"]) <= ATOL), where
    assert np.array_equal(got["reward"], R.slot_sum(got["terms"])), where


@pytest.mark.parametrize("variant,N", [("att", 3), ("att", 5), ("att", 8), ("wgru", 3), ("wgru", 5), ("wgru", 8)])
def test_map_follows_the_restatement_in_motion(native_lib, variant, N):
    W = 9
    st = C.moving_state(variant, N, W, E=3)
    occ = T.threshold_map()
    env = _env(variant, st, occ, W)
    rm = _rmap(env)
    pts, ei, ai = _motion_rows(variant, st, 7 * N)
    M = len(pts)
    half = np.arange(M) % 2 == 0
    live = st["pos"][ei, ai]
    # pre = point (the reference's map mode) on the even rows, pre = "live" on the odd ones
    a = rm.read(rm.at(pts[half], env=ei[half], agent=ai[half]))
    _against_ref(a, RM.rows(variant, st, occ, pts[half], ei[half], ai[half]), f"{variant} N={N} pre=point")
    b = rm.read(rm.at(pts[~half], env=ei[~half], agent=ai[~half], pre="live"))
    _against_ref(b, RM.rows(variant, st, occ, pts[~half], ei[~half], ai[~half], pre=live[~half]), f"{variant} N={N} pre=live")
    if variant == "att":
        assert np.all(a["terms"][:, 3] == 0) and np.any(b["terms"][:, 3] != 0)      # progress needs a pre_pos
    for name, m in (("bound", 1), ("drone", 2), ("building", 8), ("wp", 16)):
        both = np.concatenate([a["mask"], b["mask"]]) & m
        assert both.any() and not both.all(), name
    # given radar minima (every third row, straddling the penalty band [2.5, 5])
    third = np.arange(M) % 3 == 0
    rmin = np.random.default_rng(N).uniform(1.0, 7.0, int(third.sum()))
    c = rm.read(rm.at(pts[third], env=ei[third], agent=ai[third], pre=live[third], rmin=rmin))
    _against_ref(c, RM.rows(variant, st, occ, pts[third], ei[third], ai[third], pre=live[third], rmin=rmin),
                 f"{variant} N={N} rmin given")
    if variant == "wgru":
        assert np.array_equal(c["terms"][:, 11], rmin) and (c["terms"][:, 5] != 0).any()


# ------------------------------------------------------------------ 3: the reference's grid
@pytest.mark.parametrize("variant", ["att", "wgru"])
def test_reference_grid_on_two_maps(native_lib, occ, variant):
    N, W = 3, 9
    stack = np.stack([T.threshold_map(), np.asarray(occ, np.uint8)])
    st = C.moving_state(variant, N, W, E=2, seed=3)
    env = _env(variant, st, stack, W, map_idx=np.array([0, 1], np.int32))
    rm = _rmap(env)
    bx = np.linspace(env.cfg.bound[0], env.cfg.bound[1], 50)        # ATT/main:287-289
    by = np.linspace(env.cfg.bound[2], env.cfg.bound[3], 50)
    X0, Y0 = np.meshgrid(bx, by)
    pick = np.arange(0, 2500, 7)
    for e in range(2):
        X, Y, out = rm.grid(env=e, agent=e)
        assert _same_bits(X, X0) and _same_bits(Y, Y0)
        assert tuple(out["reward"].shape) == (50, 50) and tuple(out["terms"].shape) == (50, 50, 12)
        assert tuple(out["bbc"].shape) == (50, 50, 4) and tuple(out["mask"].shape) == (50, 50)
        got = {k: v.reshape((2500,) + v.shape[2:]) for k, v in rm.read(out).items()}
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], 1)
        assert got["bbc"][:, 0].any() and (got["mask"] & 8).any()           # the bound's edge rows; cells
        one = {k: v[e:e + 1] for k, v in st.items()}
        want = RM.rows(variant, one, stack[e], pts[pick], None, np.full(len(pick), e))
        _against_ref({k: v[pick] for k, v in got.items()}, want, f"{variant} grid env {e}")


# ------------------------------------------------------------------ 4: edges
def _carve(ar, M):
    reg = {"reward": ar.take(1, M), "terms": ar.take(M, 12), "mask": ar.take(1, (M + 7) // 8),
           "done": ar.take(1, (M + 7) // 8), "bbc": ar.take(1, (4 * M + 7) // 8)}
    out = {k: reg[k].view.reshape(-1) if k == "reward" else reg[k].view for k in ("reward", "terms")}
    for k, n in (("mask", M), ("done", M), ("bbc", 4 * M)):
        out[k] = reg[k].view.view(torch.uint8).reshape(-1)[:n]
    out["bbc"] = out["bbc"].view(M, 4)
    return reg, out


@pytest.mark.parametrize("M", [1, 255, 256, 257])
@pytest.mark.parametrize("variant", ["att", "wgru"])
def test_edges_in_a_canary_arena(native_lib, variant, M):
    N, W, E = 5, 9, 3
    st = C.moving_state(variant, N, W, E=E, seed=1)
    occ = T.threshold_map()
    env = _env(variant, st, occ, W)
    rm = _rmap(env)
    rng = np.random.default_rng(M)
    pts = np.stack([rng.uniform(450, 685, M), rng.uniform(250, 390, M)], 1)
    # the last env and the last agent
    full = rm.read(rm.at(pts, env=E - 1, agent=N - 1))
    ar = Arena(16 * M + 1024, torch.float64, "cuda", max_ld=16)
    reg, out = _carve(ar, M)
    snap = {k: _np(reg[k].view).copy() for k in reg}
    rm.at(pts, env=E - 1, agent=N - 1, out=out)
    torch.cuda.synchronize()
    ar.check(writable=list(reg.values()), all_written=False)
    got = rm.read(out)
    for k in KEYS:
        assert _same_bits(got[k], full[k]), k
    canary = np.uint64(0x7FF8A5A5A5A5A5A5)
    assert not (_bits(got["reward"]) == canary).any() and not (_bits(got["terms"]) == canary).any()   # every row written
    for k, n in (("mask", M), ("done", M), ("bbc", 4 * M)):
        a, b = _np(reg[k].view).view(np.uint8).reshape(-1), snap[k].view(np.uint8).reshape(-1)
        assert np.array_equal(a[n:], b[n:]), k + ": bytes past the payload"
        assert np.all(a[:n] <= 63), k + ": a row still holds the canary's bytes"
    # per-row env / agent arrays equal the scalar form; values outside the range are clamped into it
    ei, ai = np.full(M, E - 1, np.int32), np.full(M, N - 1, np.int32)
    same = rm.read(rm.at(pts, env=ei, agent=ai))
    assert all(_same_bits(same[k], full[k]) for k in KEYS)
    o = rm._alloc(M)
    d = lambda a: torch.as_tensor(a, device="cuda")          # noqa: E731
    pd, ed, ad = d(pts), d(ei + 7), d(ai + 100)
    P = rm._native.RmapOut(o["reward"].data_ptr(), None, o["mask"].data_ptr(), o["done"].data_ptr(), o["bbc"].data_ptr())
    L = rm._native.lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())              # noqa: E731
    rm._native.check(L.aac_env_reward_map(env._h, vp(pd), None, vp(ed), vp(ad), None, M, ctypes.byref(P), None), "map")
    torch.cuda.synchronize()
    for k in ("reward", "mask", "done", "bbc"):               # terms = NULL: the other outputs do not change
        assert _same_bits(_np(o[k]), full[k]), k
    assert not _np(o["terms"]).any()
    # agent 0 of env 0 is another subject
    other = rm.read(rm.at(pts))
    assert M == 1 or not _same_bits(other["reward"], full["reward"])


def test_argument_errors(native_lib):
    st = C.moving_state("att", 3, 9, E=2)
    env = _env("att", st, T.threshold_map(), 9)
    rm = _rmap(env)
    with pytest.raises(ValueError):
        rm.at(np.zeros((4, 3)))
    with pytest.raises(ValueError):
        rm.at(np.zeros((4, 2)), env=2)
    with pytest.raises(ValueError):
        rm.at(np.zeros((4, 2)), agent=np.zeros(3, np.int32))
    with pytest.raises(ValueError):
        rm.at(np.zeros((4, 2)), pre="held")
    o = rm._alloc(4)
    L, N_ = rm._native.lib(), rm._native
    pts = torch.zeros(5, 2, dtype=torch.float64, device="cuda")
    P = N_.RmapOut(*[o[k].data_ptr() for k in KEYS])
    p = ctypes.c_void_p(pts.data_ptr())
    assert L.aac_env_reward_map(env._h, p, None, None, None, None, 0, ctypes.byref(P), None) == -1
    assert b"M out of range" in L.aac_last_error()
    assert L.aac_env_reward_map(env._h, None, None, None, None, None, 4, ctypes.byref(P), None) == -1
    assert L.aac_env_reward_map(env._h, ctypes.c_void_p(pts.data_ptr() + 4), None, None, None, None, 4, ctypes.byref(P), None) == -1
    assert b"8-byte aligned" in L.aac_last_error()
    for k in ("reward", "mask", "done", "bbc"):
        Q = N_.RmapOut(*[None if j == k else o[j].data_ptr() for j in KEYS])
        assert L.aac_env_reward_map(env._h, p, None, None, None, None, 4, ctypes.byref(Q), None) == -1, k


def test_uam_env_has_no_reward_map_yet(native_lib):
    from multi_agent_aac_amd.rewardmap import RewardMap

    class NotAnEnv:
        pass
    with pytest.raises(TypeError, match="UAM env has no reward map yet"):
        RewardMap.for_env(NotAnEnv())


# ------------------------------------------------------------------ 5: read-only, capturable
@pytest.mark.parametrize("variant", ["att", "wgru"])
def test_read_only_and_capturable(native_lib, variant):
    from multi_agent_aac_amd import graphs
    N, W = 3, 9
    st, occ = _batch(variant, N, W)           # the threshold batch: its steps fill the band / fix-up lists
    E = st["pos"].shape[0]
    env, twin = _env(variant, st, occ, W), _env(variant, st, occ, W)
    rm = _rmap(env)
    ei, ai = C.all_rows(E, N)
    pts = st["post"].reshape(-1, 2) if variant == "wgru" else st["pos"].reshape(-1, 2)
    d = lambda a: torch.as_tensor(a, device="cuda")          # noqa: E731
    pd, ed, ad = d(np.ascontiguousarray(pts)), d(ei), d(ai)
    torch.cuda.synchronize()
    state0 = {k: _np(v).copy() for k, v in env.get_state().items()}
    rm.at(pd, env=ed, agent=ad)
    eager = {k: v.copy() for k, v in rm.read().items()}
    for k, v in env.get_state().items():
        assert _same_bits(_np(v), state0[k]), k
    assert env.band_max()[0] == 0             # no band or fix-up list entry either
    rng = np.random.default_rng(5)
    for s in range(5):
        # step 0 holds still: the batch lands on its threshold positions, whose rays fill the band list
        a = torch.from_numpy((rng.uniform(-1, 1, (E, N, 2)) * (s > 0)).astype(np.float32)).cuda()
        oa, ob = env.alloc_buffers(), twin.alloc_buffers()
        rm.at(pd, env=ed, agent=ad)
        env.step(a, out=oa)
        rm.at(pd, env=ed, agent=ad, pre="live")
        twin.step(a, out=ob)
        torch.cuda.synchronize()
        for k, v in vars(oa).items():
            if torch.is_tensor(v):
                assert _same_bits(_np(v), _np(getattr(ob, k))), (s, k)
        sa, sb = env.get_state(), twin.get_state()
        for k in sa:
            assert _same_bits(_np(sa[k]), _np(sb[k])), (s, k)
        assert env.band_max() == twin.band_max(), s
    assert env.band_max()[0] > 0
    # a captured launch replays equal to eager (on the state the five steps left)
    out = rm.at(pd, env=ed, agent=ad)
    eager2 = {k: v.copy() for k, v in rm.read().items()}
    assert not _same_bits(eager2["terms"], eager["terms"])
    for t in out.values():
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        rm.at(pd, env=ed, agent=ad)
    for t in out.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    replay = rm.read(out)
    for k in KEYS:
        assert _same_bits(replay[k], eager2[k]), k


# ------------------------------------------------------------------ 6: the WGRU radar minimum
def test_wgru_radar_minimum(native_lib):
    from multi_agent_aac_amd.probe import RadarProbe
    N, W = 3, 4
    st, occ = C.wgru_batch(N, W)
    E = st["pos"].shape[0]
    env = _env("wgru", C.at_rest(st, st["post"]), occ, W)
    rm = _rmap(env)
    ei, ai = C.all_rows(E, N)
    pts = st["post"].reshape(-1, 2)
    got = rm.read(rm.at(pts, env=ei, agent=ai))
    probe = RadarProbe.for_env(env)
    dist = probe.read(probe.at(st["post"]))["dist"]              # [E][N][18] double, band rays decided exactly
    want = dist.min(axis=2).reshape(-1)
    assert _same_bits(got["terms"][:, 11], want)
    band = (want >= 2.5) & (want <= 5)
    assert band.any() and not band.all()
    nbp = 3 * (((0 - 1) / (5 - 2.5)) * want + 2)
    crash_or_normal = (got["mask"] & 9) != 0
    normal = (got["mask"] & 13) == 0
    sel = band & (crash_or_normal | normal)
    assert sel.any() and np.array_equal(got["terms"][sel, 5], -nbp[sel])
    assert np.all(got["terms"][~band, 5] == 0)
    # given minima come back unchanged, -0.0, inf and a denormal included
    given = np.random.default_rng(0).uniform(0.0, 16.0, E * N)
    given[:4] = (-0.0, np.inf, 5e-324, 2.5)
    back = rm.read(rm.at(pts, env=ei, agent=ai, rmin=given))
    assert _same_bits(back["terms"][:, 11], given)


# ------------------------------------------------------------------ 7: the facade
def test_facade_ss_reward_at_xy(native_lib, occ):
    from multi_agent_aac_amd.env import env_simulator
    from multi_agent_aac_amd.rewardmap import RewardMap

    def make():
        sim = env_simulator(np.asarray(occ, np.uint8), seed=3, reward_terms=True)
        sim.create_world(3, 2, 0.95, 0.01, 10, 2, 0.1, 1.0, 300, 5.0, [-8, 8])
        sim.reset_world(3)
        sim.step(np.full((3, 2), 0.3))
        return sim
    sim, twin = make(), make()
    N = 3
    rec, rec_t = [[0.0, None]] * N, [[0.0, None]] * N
    hold, coll = [None] * N, [[] for _ in range(N)]
    sim.ss_reward(0, rec, hold, coll)
    twin.ss_reward(0, rec_t, [None] * N, [[] for _ in range(N)])
    pos0 = sim.all_agents[0].pos.copy()
    state0 = {k: _np(v).copy() for k, v in sim._env.get_state().items()}
    g = sim.all_agents[0].goal[-1]
    seen_goal = False
    for xy in ((pos0[0] + 1.0, pos0[1] - 2.0), (float(g[0]), float(g[1])), (sim.bound[0] + 1.0, sim.bound[2] + 40.0)):
        reward, done, check_goal, rec2, hold2, coll2, bbc = sim.ss_reward(0, rec, hold, coll, xy=xy)
        row = RewardMap.for_env(sim._env).read(RewardMap.for_env(sim._env).at(np.array([xy])))
        assert len(reward) == 1 and len(done) == 1 and len(check_goal) == N and len(bbc) == 4
        assert isinstance(reward[0], np.float64) and _same_bits(np.array(reward), row["reward"])
        assert done == [bool(row["done"][0])] and check_goal == [bool(row["mask"][0] & 32), False, False]
        assert bbc == [bool(v) for v in row["bbc"][0]]
        assert rec2 is rec and rec[0] == [0.0, float(row["terms"][0, 3])] and hold2 is hold and coll2 is coll
        seen_goal |= check_goal[0]
        assert np.array_equal(sim.all_agents[0].pos, pos0)
    assert seen_goal and done == [True]              # the goal itself; the point 1 m inside the bound line
    for k, v in sim._env.get_state().items():
        assert _same_bits(_np(v), state0[k]), k
    # xy=(None, None) is the plain path; a following step equals the twin's that never asked
    a = sim.ss_reward(0, [[0.0, None]] * N, [None] * N, [[] for _ in range(N)], xy=(None, None))
    b = twin.ss_reward(0, [[0.0, None]] * N, [None] * N, [[] for _ in range(N)])
    assert repr(a) == repr(b)
    act = np.full((3, 2), -0.2)
    sa, sb = sim.step(act), twin.step(act)
    for k in ("reward", "done", "mask", "bbc", "terms"):
        assert _same_bits(sim._last[k], twin._last[k]), k
    for k in ("own", "radar", "nei"):
        assert _same_bits(_np(getattr(sim._env.bufs, k)), _np(getattr(twin._env.bufs, k))), k
    ga, gb = sim._env.get_state(), twin._env.get_state()
    for k in ga:
        assert _same_bits(_np(ga[k]), _np(gb[k])), k
