"""The HIP env kernel's WGRU reward (config 4; ``wgru_reward``, the step kernel's waypoint cache and the
reward fix-up in csrc/aac_env.hip) on the exact-threshold states of tests/wgru_thresholds.py: waypoint
distances on 5 m, prefix minima and ties, the deciding waypoint at chosen list indices either side of the
8-entry LDS cache with removal masks up to bit 31, cross-track distances on 2.5 m from every placement,
later and tied nearest segments, degenerate segments, 1 000 random polylines, and a flagged radar ray in
each reward branch -- with waypoint lists of W = 4, 8, 9 and 32 slots (W below, at and above the cache).

Every launch is compared with the C oracle from the same injected state (masks, done, bbc, env_done, the
fp32 radar, wp_cur, goal, reach, wall and the post-step position bit for bit; own, nei and reward within
1e-5, the parity bar of DESIGN section 2); then ``wgru_thresholds.check`` states every non-random
subject's outcome from rationals, and both outcomes of every boolean threshold must occur.
tests/test_wgru_thresholds_cpu.py holds the same checks for the oracle alone."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle.consts import X_SCALE, Y_SCALE
from tests import thresholds as T
from tests import wgru_thresholds as WT

pytestmark = pytest.mark.gpu
ATOL = 1e-5


def _np(t):
    return t.detach().cpu().numpy()


def _env(E, N, W, occ):
    from multi_agent_aac_amd.env import BatchedEnv
    return BatchedEnv(E, N, occ, max_wp=W, variant="wgru")


def _install(env, st):
    E, N = st["pos"].shape[:2]
    env.set_state(pos=st["pos"], pre_pos=st["pre_pos"], vel=st["vel"], pre_vel=st["vel"], goal=st["goal"],
                  wp=st["wp"], wp_cur=st["wp_cur"], wp_cnt=st["cnt"], reach=np.zeros((E, N), np.uint8),
                  wall=np.zeros((E, N), np.int32), step=np.zeros(E, np.int32), map_idx=np.zeros(E, np.int32),
                  start=st["start"])


def _listed(fam, var):
    """The fix_kind subjects with a ray through a cell corner: each is listed for the reward fix-up."""
    n = sum(1 for f, v in zip(fam, var) if f == "fix_kind" and v[0].startswith("corner"))
    assert n >= 40
    return n


def _cmp_oracle(env, b, co, where):
    """Outputs b and the env's state against the oracle's.  Returns the state as numpy arrays."""
    for f in ("mask", "done", "bbc", "env_done"):
        assert np.array_equal(_np(getattr(b, f)), getattr(co, f)), where + " " + f
    assert np.array_equal(_np(b.radar), co.radar), where + " radar (fp32 bit-exact)"
    s = {k: _np(v) for k, v in env.get_state().items()}
    for f in ("wp_cur", "goal", "reach", "wall", "pos"):
        bad = np.argwhere(s[f] != getattr(co, f))
        assert bad.size == 0, (where, f, bad[:4].tolist())
    for f in ("own", "nei", "reward"):
        np.testing.assert_allclose(_np(getattr(b, f)), getattr(co, f), rtol=0, atol=ATOL, err_msg=where + " " + f)
    return s


@pytest.mark.parametrize("W", [4, 8, 9, 32])
@pytest.mark.parametrize("N", [3, 5, 8])
def test_step_kernel_on_wgru_thresholds(native_lib, N, W):
    """aac_env_step, one launch.  fix_kind: the subjects with a ray through a cell corner are listed for the
    reward fix-up in each of its kinds (no crash, goal reached, building contact: band_max counts them) and
    their rewards equal the oracle's, which takes the exact radar minimum."""
    occ = T.threshold_map()
    fam, var, st = WT.build(N, W)
    E = len(fam)
    env = _env(E, N, W, occ)
    co = c_oracle.BatchedOracle(E, N, occ, W=W, variant="wgru")
    _install(env, st)
    WT.oracle_state(co, st)
    act = np.zeros((E, N, 2), np.float32)
    env.step(torch.from_numpy(act).cuda())
    co.step(act)
    torch.cuda.synchronize()
    where = f"step N{N} W{W}"
    s = _cmp_oracle(env, env.bufs, co, where)
    assert np.array_equal(s["pos"], st["post"])
    seen = WT.check(fam, var, st, s, _np(env.bufs.mask), _np(env.bufs.reward), where)
    WT.both_ways(seen)
    most, cap = env.band_max()
    assert _listed(fam, var) <= most <= cap, (most, cap)


@pytest.mark.parametrize("W", [4, 32])
def test_step_tail_on_wgru_thresholds(native_lib, W):
    """aac_env_step_tail with a replay ring (the bench's launch), no auto-reset: the ring's reward column
    carries the fixed-up rewards and its n_own column the step's own rows."""
    from multi_agent_aac_amd.memory import DeviceReplay
    N = 5
    occ = T.threshold_map()
    fam, var, st = WT.build(N, W)
    E = len(fam)
    env = _env(E, N, W, occ)
    rep = DeviceReplay(2 * E, N, env.D0, seed=0)
    c, n = env.alloc_buffers(), env.alloc_buffers()
    _install(env, st)
    co = c_oracle.BatchedOracle(E, N, occ, W=W, variant="wgru")
    WT.oracle_state(co, st)
    act = np.zeros((E, N, 2), np.float32)
    a_dev = torch.from_numpy(act).cuda()
    srcs = [c.own, c.radar, c.nei, a_dev, n.reward, n.done, n.own, n.radar, n.nei]
    pos0 = rep.pos
    env.step_tail(a_dev, out=n, replay=rep, srcs=srcs, auto_reset=False)
    co.step(act)
    torch.cuda.synchronize()
    where = f"tail W{W}"
    s = _cmp_oracle(env, n, co, where)
    seen = WT.check(fam, var, st, s, _np(n.mask), _np(n.reward), where)
    WT.both_ways(seen)
    off = np.cumsum([0] + list(rep.widths))
    ring = _np(rep.ring[pos0:pos0 + E])
    k = list(rep.fields).index("rew")
    np.testing.assert_allclose(ring[:, off[k]:off[k + 1]], co.reward, rtol=0, atol=ATOL, err_msg=where + " ring reward")
    assert np.array_equal(ring[:, off[k]:off[k + 1]], _np(n.reward)), where + " ring reward = the checked output"
    k = list(rep.fields).index("n_own")
    np.testing.assert_allclose(ring[:, off[k]:off[k + 1]], co.own.reshape(E, -1), rtol=0, atol=ATOL,
                               err_msg=where + " ring n_own")
    most, cap = env.band_max()
    assert _listed(fam, var) <= most <= cap, (most, cap)


@pytest.mark.parametrize("W", [8, 32])
def test_two_steps_from_the_popped_state(native_lib, W):
    """Two zero-action steps on the wp5_*, wp_index and wp_final_pop states, the second from the kernel's
    own popped state.  The observation precedes ss_reward (WGRU/env:2131 before :1666): the first step's own
    row still carries the old goal[-1], the popped one appears at the second step."""
    N = 5
    occ = T.threshold_map()
    fam, var, st = WT.select(*WT.build(N, W), WT.TWO_STEP_FAMILIES)
    E = len(fam)
    env = _env(E, N, W, occ)
    co = c_oracle.BatchedOracle(E, N, occ, W=W, variant="wgru")
    _install(env, st)
    WT.oracle_state(co, st)
    act = np.zeros((E, N, 2), np.float32)
    a_dev = torch.from_numpy(act).cuda()
    env.step(a_dev)
    co.step(act)
    torch.cuda.synchronize()
    s1 = _cmp_oracle(env, env.bufs, co, f"two-step W{W} first")
    WT.check(fam, var, st, s1, _np(env.bufs.mask), _np(env.bufs.reward), f"two-step W{W}")
    own1 = _np(env.bufs.own).copy()
    # the second step: the oracle takes the kernel's state (popped masks and goals included)
    for k, f in (("pos", "pos"), ("vel", "vel"), ("pre_pos", "pre_pos"), ("pre_vel", "pre_vel"), ("goal", "goal"),
                 ("wp_cur", "wp_cur"), ("reach", "reach"), ("wall", "wall"), ("step_count", "step")):
        getattr(co, k)[:] = s1[f]
    env.step(a_dev)
    co.step(act)
    torch.cuda.synchronize()
    s2 = _cmp_oracle(env, env.bufs, co, f"two-step W{W} second")
    own2 = _np(env.bufs.own)
    ix, sj = np.arange(E), st["subj"]
    scale = np.array([X_SCALE, Y_SCALE])
    g0, g1 = st["goal"][ix, sj], s1["goal"][ix, sj]
    moved = np.any(g0 != g1, -1)
    assert moved.sum() >= 3 and (~moved).sum() >= 3
    assert np.abs((g1 - g0)[moved] * scale).max(-1).min() > 100 * ATOL        # the two goals differ in the row
    np.testing.assert_allclose(own1[ix, sj, 4:6], (g0 - s1["pos"][ix, sj]) * scale, rtol=0, atol=ATOL)
    np.testing.assert_allclose(own2[ix, sj, 4:6], (g1 - s2["pos"][ix, sj]) * scale, rtol=0, atol=ATOL)
