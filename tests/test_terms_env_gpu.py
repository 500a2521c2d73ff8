"""The env step kernels' reward terms (include/aac_terms.h; ``step_kernel<.., TERMS>`` and the fix-up in
csrc/aac_env.hip) through aac_env_set_terms_buffer, on injected exact-threshold states.

  sum identity   float32(sum of an agent's slots 0..6, left to right) is its reward, as a value (team
                 reward: float32 of the pairwise sum over the env's agents) -- no oracle involved; also on
                 the batch whose rewards the exact fix-up rewrites
  coverage       every reward branch occurs and every slot the variant uses is non-zero somewhere
  values         every slot against tests/terms_ref.py at 1e-12 absolute
  detached       no buffer, and a buffer attached then detached, give bit-equal outputs"""
import functools

import numpy as np
import pytest
import torch

from tests import terms_ref as R
from tests import thresholds as T
from tests import wgru_thresholds as WT

pytestmark = pytest.mark.gpu
ATOL = 1e-12          # the project's bar for fp64 env quantities on injected inputs


def _np(t):
    return t.detach().cpu().numpy()


def pairwise_sum(a):
    """numpy's pairwise summation of the N per-agent rewards (the kernel's team sum), per env."""
    return np.array([np.sum(row) for row in np.asarray(a, dtype=np.float64)])


@functools.lru_cache(maxsize=None)
def _att_batch(N):
    """tests/thresholds.py's families plus the near-band ones; the subject (agent 0) holds still, the
    others take random actions, so progress terms are non-zero in the normal branch."""
    fam, var, st, occ = T.build(N, seed=N)
    near = T.build_near(N)
    st = {k: np.concatenate([st[k], near[2][k]]) for k in st}
    E = st["pos"].shape[0]
    assert E <= 384
    act = np.random.default_rng(N).uniform(-1, 1, (E, N, 2)).astype(np.float32) * 0.5
    act[:, 0] = 0
    return st, occ, act


@functools.lru_cache(maxsize=None)
def _wgru_batch(N, W, families=None):
    fam, var, st = WT.build(N, W)
    keep = families or tuple(sorted(f for f in set(fam) if f != "xt_random"))
    fam, var, st = WT.select(fam, var, st, keep)
    E = len(fam)
    assert E <= 384
    return fam, var, st, T.threshold_map(), np.zeros((E, N, 2), np.float32)


def _sub(st, act, n):
    idx = np.linspace(0, st["pos"].shape[0] - 1, n).astype(int)
    return {k: v[idx] for k, v in st.items()}, act[idx]


def _att_env(st, occ, N, team, mode=0):
    from multi_agent_aac_amd.env import BatchedEnv
    E = st["pos"].shape[0]
    env = BatchedEnv(E, N, occ, radar_mode=mode, max_wp=32, team_reward=team)
    env.set_state(pos=st["pos"], pre_pos=st["pre_pos"], vel=st["vel"], pre_vel=st["vel"], goal=st["goal"],
                  wp=st["wp"], wp_cur=np.zeros((E, N), np.int32), wp_cnt=st["cnt"],
                  reach=np.zeros((E, N), np.uint8), wall=np.zeros((E, N), np.int32), step=np.zeros(E, np.int32),
                  map_idx=np.zeros(E, np.int32), start=st["pos"])
    return env


def _wgru_env(st, occ, N, W):
    from multi_agent_aac_amd.env import BatchedEnv
    E = st["pos"].shape[0]
    env = BatchedEnv(E, N, occ, max_wp=W, variant="wgru")
    env.set_state(pos=st["pos"], pre_pos=st["pre_pos"], vel=st["vel"], pre_vel=st["vel"], goal=st["goal"],
                  wp=st["wp"], wp_cur=st["wp_cur"], wp_cnt=st["cnt"], reach=np.zeros((E, N), np.uint8),
                  wall=np.zeros((E, N), np.int32), step=np.zeros(E, np.int32), map_idx=np.zeros(E, np.int32),
                  start=st["start"])
    return env


def _run(env, act, tail, bank=None):
    """One step (plain, or the fused tail -- with the in-launch auto-reset when a bank is given) into fresh
    buffers; returns them."""
    out = env.alloc_buffers()
    a = torch.from_numpy(act).cuda()
    if tail:
        if bank is not None:
            env.set_od_bank(bank, seed=5)
        env.step_tail(a, out=out, replay=None, auto_reset=bank is not None)
    else:
        env.step(a, out=out)
    torch.cuda.synchronize()
    return out


def _identity(terms, reward, team):
    s = R.slot_sum(terms)                       # (E, N) double
    if team:
        s = np.repeat(pairwise_sum(s)[:, None], s.shape[1], axis=1)
    got = s.astype(np.float32)
    bad = np.argwhere(got != reward)
    assert bad.size == 0, (bad[:4].tolist(), got[tuple(bad[0])], reward[tuple(bad[0])])
    assert np.all(terms[..., 7] == 0)


def _bank(occ, W):
    from multi_agent_aac_amd import world
    return world.ODBank(occ, n_pairs=256, seed=1, max_wp=W)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("team", [False, True])
@pytest.mark.parametrize("N", [3, 5])
def test_att_sum_identity(native_lib, N, team, tail):
    st, occ, act = _att_batch(N)
    st, act = _sub(st, act, 96)
    env = _att_env(st, occ, N, team)
    terms = env.use_terms_buffer()
    out = _run(env, act, tail, _bank(occ, 32) if tail else None)
    if tail:
        assert int(out.env_done.sum()) > 0        # envs were reset in the launch: their terms rows stay
    _identity(_np(terms), _np(out.reward), team)


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("W", [4, 9])
@pytest.mark.parametrize("N", [3, 8])
def test_wgru_sum_identity(native_lib, N, W, tail):
    fam, var, st, occ, act = _wgru_batch(N, W)
    st, act = _sub(st, act, 96)
    env = _wgru_env(st, occ, N, W)
    terms = env.use_terms_buffer()
    out = _run(env, act, tail, _bank(occ, W) if tail and W >= 6 else None)      # the bank's paths need 6 slots
    _identity(_np(terms), _np(out.reward), False)


@pytest.mark.parametrize("tail", [False, True])
def test_wgru_sum_identity_through_the_fixup(native_lib, tail):
    """The corner batch: a ray of each subject touches a cell corner, so its reward is listed and
    rewritten from the exact radar minimum after the launch -- slots 5 and 11 must follow."""
    N, W = 3, 4
    fam, var, st, occ, act = _wgru_batch(N, W, ("fix_kind",))
    env = _wgru_env(st, occ, N, W)
    terms = env.use_terms_buffer()
    out = _run(env, act, tail)
    listed = sum(1 for v in var if v[0].startswith("corner"))
    most, cap = env.band_max()
    assert 40 <= listed <= most <= cap, (listed, most, cap)
    t = _np(terms)
    _identity(t, _np(out.reward), False)
    # the listed subjects' penalty is the exact minimum's (tests/wgru_thresholds.fix_outcome)
    seen = 0
    for e, v in enumerate(var):
        if v[0] in ("corner", "corner_building"):
            s = int(st["subj"][e])
            rmin = float(T.exact_radar(tuple(st["post"][e, s]), [], occ, 1).min())
            nbp = 3 * ((-1 / (5 - 2.5)) * rmin + 2) if 2.5 <= rmin <= 5 else 0.0
            assert abs(t[e, s, 11] - rmin) <= 1e-9 and abs(t[e, s, 5] + nbp) <= 1e-9, (v, t[e, s], rmin, nbp)
            seen += nbp != 0.0
    assert seen > 0


@functools.lru_cache(maxsize=None)
def _att_ref(N):
    st, occ, act = _att_batch(N)
    return R.batch_terms("att", st, occ, act)


@functools.lru_cache(maxsize=None)
def _wgru_ref(N, W):
    fam, var, st, occ, act = _wgru_batch(N, W)
    return R.batch_terms("wgru", st, occ, act)


def _report(name, got, want):
    err = np.abs(got - want).max(axis=(0, 1))
    print(name, "max |terms - terms_ref| per slot:", " ".join(f"{R.NAMES[k]}={err[k]:.3g}" for k in range(R.WIDTH)))
    return err


@pytest.mark.parametrize("tail", [False, True])
def test_att_values_and_coverage(native_lib, tail):
    N = 5
    st, occ, act = _att_batch(N)
    want, own = _att_ref(N)
    env = _att_env(st, occ, N, False)
    terms = env.use_terms_buffer()
    out = _run(env, act, tail)
    t, m = _np(terms), _np(out.mask)
    err = _report(f"att tail={tail}", t, want)
    assert np.all(err <= ATOL), err
    assert np.array_equal(_np(out.reward), own.astype(np.float32))
    # coverage: bound, drone collision, goal, normal; every slot the variant uses
    bound, drone, goal = (m & 1) != 0, ((m & 1) == 0) & ((m & 2) != 0), ((m & 3) == 0) & ((m & 4) != 0)
    normal = (m & 7) == 0
    for name, sel in (("bound", bound), ("drone", drone), ("goal", goal), ("normal", normal)):
        assert sel.any(), name
    assert np.all(t[bound][:, 0] == -20) and np.all(t[bound][:, [3, 6]] == 0)
    assert np.all(t[drone][:, 0] == -20) and np.any(t[drone][:, 6] < 0) and np.all(t[drone][:, 3] == 0)
    assert np.all(t[goal][:, 0] == 20) and np.all(t[goal][:, [3, 6]] == 0)
    assert np.all(t[normal][:, 0] == 0) and np.any(t[normal][:, 3] != 0) and np.any(t[normal][:, 6] < 0)
    assert np.all(t[..., [1, 2, 4, 5, 7, 8, 11]] == 0)
    assert np.any(t[..., 9] > 0) and np.all(t[..., 10] >= 0)


@pytest.mark.parametrize("tail", [False, True])
def test_wgru_values_and_coverage(native_lib, tail):
    N, W = 3, 9
    fam, var, st, occ, act = _wgru_batch(N, W)
    want, own = _wgru_ref(N, W)
    env = _wgru_env(st, occ, N, W)
    terms = env.use_terms_buffer()
    out = _run(env, act, tail)
    t, m = _np(terms), _np(out.mask)
    err = _report(f"wgru tail={tail}", t, want)
    assert np.all(err <= ATOL), err
    np.testing.assert_allclose(_np(out.reward), own, rtol=0, atol=1e-5)
    bound, building = (m & 1) != 0, ((m & 1) == 0) & ((m & 8) != 0)
    goal, normal = ((m & 9) == 0) & ((m & 4) != 0), (m & 13) == 0
    for name, sel in (("bound", bound), ("building", building), ("goal", goal), ("normal", normal)):
        assert sel.any(), name
    for sel in (bound, building):
        assert np.all(t[sel][:, 0] == -5) and np.all(t[sel][:, 1] == 0)
    assert np.all(t[goal][:, 0] == 5) and np.all(t[goal][:, 1:7] == 0)
    assert np.all(t[normal][:, 0] == 0) and np.any(t[normal][:, 1] == 3)
    assert np.all(np.isin(t[..., 1], (0.0, 3.0)))
    for k in (0, 1, 2, 3, 4, 5, 8, 9, 10, 11):
        assert np.any(t[..., k] != 0), R.NAMES[k]
    assert np.all(t[..., 6:8] == 0)


@pytest.mark.parametrize("variant", ["att", "wgru"])
@pytest.mark.parametrize("tail", [False, True])
def test_detached_equals_today(native_lib, variant, tail):
    """No buffer, and a buffer attached (one step taken with it) then detached: the same injected state
    gives bit-equal outputs and state; the attached step's outputs are the same too."""
    N = 3
    if variant == "att":
        st, occ, act = _att_batch(N)
        st, act = _sub(st, act, 96)
        mk = lambda: _att_env(st, occ, N, True)        # noqa: E731
    else:
        fam, var, st, occ, act = _wgru_batch(N, 9)
        st, act = _sub(st, act, 96)
        mk = lambda: _wgru_env(st, occ, N, 9)          # noqa: E731
    bank = _bank(occ, 32 if variant == "att" else 9) if tail else None

    def outputs(env, o):
        d = {k: _np(v).copy() for k, v in vars(o).items() if torch.is_tensor(v)}
        d.update({"state." + k: _np(v) for k, v in env.get_state().items()})
        return d

    plain = mk()
    a = outputs(plain, _run(plain, act, tail, bank))
    env = mk()
    env.use_terms_buffer()
    b = outputs(env, _run(env, act, tail, bank))
    env2 = mk()
    env2.use_terms_buffer()
    env2.use_terms_buffer(detach=True)
    assert env2.terms is None
    c = outputs(env2, _run(env2, act, tail, bank))
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), "detached " + k
        assert a[k].tobytes() == b[k].tobytes(), "attached " + k
