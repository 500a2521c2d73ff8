"""The env kernels over the whole accepted agent count (2 <= N <= 256) against the C oracle, at the
counts tests/agent_count_cases.py lists with the branch each one takes.  Bars as in test_env_gpu:
masks / done / bbc / env_done / wp_cur / reach / wall bit-exact, fp32 outputs within 1e-5, state
within 1e-12, crowded radar bit-identical."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import agent_count_cases as C
from tests.helpers import W_DEFAULT, bank_draw_batch, steer, wgru_targets
from tests.test_env_gpu import ATOL, _cmp_out, _cmp_step, _state_to_oracle

pytestmark = pytest.mark.gpu


def _env(E, N, occ, variant="att", mode=2, **kw):
    from multi_agent_aac_amd.env import BatchedEnv
    if variant == "wgru":
        return BatchedEnv(E, N, occ, max_wp=W_DEFAULT, variant="wgru", **kw)
    return BatchedEnv(E, N, occ, radar_mode=mode, max_wp=W_DEFAULT, **kw)


def _cmp_state(env, co, where):
    s = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    np.testing.assert_allclose(s["pos"], co.pos, rtol=1e-12, atol=1e-12, err_msg=where + " pos")
    np.testing.assert_allclose(s["vel"], co.vel, rtol=1e-12, atol=1e-12, err_msg=where + " vel")
    assert np.array_equal(s["wp_cur"], co.wp_cur), where + " wp_cur"
    assert np.array_equal(s["goal"], co.goal), where + " goal"
    assert np.array_equal(s["reach"], co.reach), where + " reach"
    assert np.array_equal(s["wall"], co.wall), where + " wall"
    assert np.array_equal(s["step"], co.step_count), where + " step"


@pytest.mark.parametrize("variant,N,mode,tdcpa,team", C.PARITY,
                         ids=[f"{v}-N{N}-m{m}{'-tdcpa' if td else ''}{'' if tr or v == 'wgru' else '-own'}"
                              for v, N, m, td, tr in C.PARITY])
def test_step_reset_parity(native_lib, occ, variant, N, mode, tdcpa, team):
    """Reset, then steps from the identical injected state on both sides, with masked resets of the
    finished envs; E = 2 epb + 1 (a ragged last workgroup)."""
    E, steps = C.small_E(N), C.steps_for(N)
    assert C.epb_of(E, N) == C.epb_for(24, N) and (E % C.epb_of(E, N) or C.epb_of(E, N) == 1)
    st, wps, cnt = C.make_od(occ, E, N, seed=500 + N + 7 * mode)
    kw = {} if variant == "wgru" else dict(team_reward=team)
    env = _env(E, N, occ, variant, mode, tdcpa=tdcpa, **kw)
    co = c_oracle.BatchedOracle(E, N, occ, W=W_DEFAULT, radar_mode=mode, with_tdcpa=tdcpa, team_reward=team,
                                variant=variant)
    env.reset(st, wps, cnt)
    co.reset(st, wps, cnt)
    torch.cuda.synchronize()
    _cmp_out(env.bufs, co, "reset")
    rng = np.random.default_rng(N)
    resets = 0
    for t in range(steps):
        _state_to_oracle(env, co)
        if variant == "wgru":
            act = steer(co.pos, co.vel, wgru_targets(co.wp, co.wp_cur, co.wp_cnt), rng)
        else:
            act = rng.uniform(-1, 1, size=(E, N, 2)).astype(np.float32)
        env.step(torch.from_numpy(act).cuda())
        co.step(act)
        torch.cuda.synchronize()
        where = f"{variant} N{N} mode{mode} t{t}"
        _cmp_step(env.bufs, co, where)
        _cmp_state(env, co, where)
        if tdcpa:
            np.testing.assert_allclose(env.bufs.tcpa.cpu().numpy(), co.tcpa, rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(env.bufs.dcpa.cpu().numpy(), co.dcpa, rtol=1e-9, atol=1e-9)
            assert np.array_equal(env.bufs.conf_cur.cpu().numpy(), co.conf_cur)
            assert np.array_equal(env.bufs.conf_pre.cpu().numpy(), co.conf_pre)
        done = co.env_done.astype(np.uint8)
        if done.any() and not done.all() or t == steps // 2:
            done[-1] = 1                                  # the ragged workgroup's env resets at least once
            st2, wps2, cnt2 = C.make_od(occ, E, N, seed=1000 * t + N)
            env.reset(st2, wps2, cnt2, env_mask=done)
            co.reset(st2, wps2, cnt2, env_mask=done)
            torch.cuda.synchronize()
            _cmp_out(env.bufs, co, f"reset t{t}")
            resets += int(done.sum())
    assert resets > 0
    assert env.check_band_capacity()[0] <= C.BLOCK * 18


@pytest.mark.parametrize("N,mode", C.CROWDED)
def test_radar_crowded_bit_exact(native_lib, occ, N, mode):
    """Crowded injected states, stay put for one step: the radar bit-identical to the oracle.  Past
    64 agents the inputs are ones whose answer changes when any later block of 64 is taken away
    (checked on the CPU in test_agent_count_cases_cpu), so a skipped candidate chunk cannot pass."""
    E = 8 if N < 256 else 4
    st, wps, cnt = C.make_od(occ, E, N, seed=77)
    env = _env(E, N, occ, "att", mode)
    co = c_oracle.BatchedOracle(E, N, occ, W=W_DEFAULT, radar_mode=mode)
    env.reset(st, wps, cnt)
    co.reset(st, wps, cnt)
    pos = C.crowded_state(E, N, C.CROWDED_SEED[N])
    z = np.zeros_like(pos)
    env.set_state(pos=pos, pre_pos=pos, vel=z, pre_vel=z)
    _state_to_oracle(env, co)
    act = np.zeros((E, N, 2), np.float32)
    env.step(torch.from_numpy(act).cuda())
    co.step(act)
    torch.cuda.synchronize()
    assert np.array_equal(env.bufs.radar.cpu().numpy(), co.radar)
    assert np.array_equal(env.get_state()["pos"].cpu().numpy(), pos)
    _cmp_step(env.bufs, co, f"crowded N{N} mode{mode}")
    assert (co.radar == 0).any() and (co.radar < 15).mean() > 0.2


def _bank_pair(E, N, occ, variant, ep_len, seed=4321):
    from multi_agent_aac_amd import world
    bank = world.ODBank(occ, n_pairs=4096, seed=5, max_wp=W_DEFAULT)
    envs = []
    for _ in range(2):
        env = _env(E, N, occ, variant, 2, episode_length=ep_len)
        env.set_od_bank(bank, seed=seed)
        envs.append(env)
    return envs


def _same(ea, eb, na, nb, where):
    for f in ("own", "radar", "nei", "reward", "done", "mask", "env_done", "bbc"):
        assert torch.equal(getattr(na, f), getattr(nb, f)), (where, f)
    sa, sb = ea.get_state(), eb.get_state()
    for key in sa:
        assert torch.equal(sa[key], sb[key]), (where, key)


@pytest.mark.parametrize("variant,N", C.TAIL_RING)
def test_step_tail_with_ring_equals_separate_launches(native_lib, occ, variant, N):
    """test_step_tail_equals_separate_launches at the staged counts on either end of the range: N = 2
    (12 envs per workgroup), 9 and the widest staged rows (ATT 16, WGRU 20)."""
    from multi_agent_aac_amd.memory import DeviceReplay
    E = 4 * C.epb_for(24, N) + 1
    assert C.staged(variant, E, N)
    ea, eb = _bank_pair(E, N, occ, variant, 3)
    H = 16 if variant == "wgru" else 0
    cap = int(2.5 * E)
    ra = DeviceReplay(cap, N, ea.D0, hidden=H, seed=1)
    rb = DeviceReplay(cap, N, eb.D0, hidden=H, seed=1)
    bufs = [[e.alloc_buffers(), e.alloc_buffers()] for e in (ea, eb)]
    ea.auto_reset(None, out=bufs[0][0])
    eb.auto_reset(None, out=bufs[1][0])
    g = torch.Generator(device="cuda").manual_seed(3)
    hid = [torch.rand(E, N, H or 1, device="cuda", generator=g) for _ in range(2)]
    ha, hb = [h.clone() for h in hid], [h.clone() for h in hid]
    rng = np.random.default_rng(11)
    resets = 0
    for t in range(8):
        act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)).cuda()
        k = t % 2
        ca, na = bufs[0][k], bufs[0][1 - k]
        cb, nb = bufs[1][k], bufs[1][1 - k]
        ea.step(act, out=na)
        extra = [ha[k], ha[1 - k]] if H else []
        ra.push_batch(ca.own, ca.radar, ca.nei, act, na.reward, na.done, na.own, na.radar, na.nei, *extra)
        if H:
            ha[1 - k].mul_((na.env_done == 0).to(torch.float32)[:, None, None])
        ea.auto_reset(na.env_done, out=na)
        srcs = [cb.own, cb.radar, cb.nei, act, nb.reward, nb.done, nb.own, nb.radar, nb.nei]
        if H:
            srcs += [hb[k], hb[1 - k]]
        eb.step_tail(act, out=nb, replay=rb, srcs=srcs, zero_rows=hb[1 - k] if H else None)
        torch.cuda.synchronize()
        resets += int(na.env_done.sum())
        _same(ea, eb, na, nb, t)
        assert torch.equal(ra.meta, rb.meta) and (ra.pos, ra.size) == (rb.pos, rb.size), t
        assert torch.equal(ra.ring, rb.ring), t
        if H:
            assert torch.equal(ha[1 - k], hb[1 - k]), t
    assert resets > 0
    assert ra.size == cap and ra.pos == (8 * E) % cap


@pytest.mark.parametrize("variant,N", C.TAIL_NO_RING)
def test_step_tail_auto_reset_equals_separate_launches(native_lib, occ, variant, N):
    """Step + auto-reset in one launch, no ring, with unstaged rows: the speculative draw on (ATT 17,
    84; WGRU 21, 65) and off (85, 193), and no agent-free wave at all (193)."""
    E = 5
    ea, eb = _bank_pair(E, N, occ, variant, 2)
    for e in (ea, eb):
        e.auto_reset(None)
    rng = np.random.default_rng(N)
    resets = 0
    for t in range(6):
        act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 2)).astype(np.float32)).cuda()
        ea.step(act)
        ea.auto_reset(ea.bufs.env_done)
        eb.step_tail(act, auto_reset=True)
        torch.cuda.synchronize()
        resets += int(eb.bufs.env_done.sum())
        _same(ea, eb, ea.bufs, eb.bufs, t)
    assert resets > 0
    assert int(eb.get_state()["step"].max()) <= 2


@pytest.mark.parametrize("variant,N", C.TOO_WIDE)
def test_step_tail_refuses_ring_push_of_unstaged_rows(native_lib, occ, variant, N):
    """One agent past the staging area: own / nei as step outputs cannot be pushed.  The call returns
    AAC_E_INVALID ("too wide"), writes nothing to the ring and does not step the env."""
    from multi_agent_aac_amd import _native
    from multi_agent_aac_amd.memory import DeviceReplay
    E = 5
    assert not C.staged(variant, E, N) and C.staged(variant, E, N - 1)
    (env, _) = _bank_pair(E, N, occ, variant, 50)
    H = 16 if variant == "wgru" else 0
    rep = DeviceReplay(3 * E, N, env.D0, hidden=H, seed=1)
    cur, nxt = env.alloc_buffers(), env.alloc_buffers()
    env.auto_reset(None, out=cur)
    act = torch.full((E, N, 2), 0.5, device="cuda")
    hid = [torch.rand(E, N, H, device="cuda") for _ in range(2)] if H else []
    torch.cuda.synchronize()
    ring0, meta0 = rep.ring.clone(), rep.meta.clone()
    before = {k: v.clone() for k, v in env.get_state().items()}
    srcs = [cur.own, cur.radar, cur.nei, act, nxt.reward, nxt.done, nxt.own, nxt.radar, nxt.nei] + hid
    with pytest.raises(Exception, match="too wide"):
        env.step_tail(act, out=nxt, replay=rep, srcs=srcs)
    assert b"too wide" in _native.lib().aac_last_error()
    torch.cuda.synchronize()
    assert torch.equal(rep.ring, ring0) and torch.equal(rep.meta, meta0)
    assert (rep.pos, rep.size) == (0, 0)                  # the host mirror of the ring position stays too
    after = env.get_state()
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert int(nxt.reward.abs().sum()) == 0 and int(nxt.env_done.sum()) == 0
    # with the rows of the previous step as sources only (no step output among own / nei) the push goes through
    env.step_tail(act, out=nxt, replay=rep, srcs=[cur.own, cur.radar, cur.nei, act, nxt.reward, nxt.done,
                                                  cur.own, nxt.radar, cur.nei] + hid)
    torch.cuda.synchronize()
    assert int(env.get_state()["step"].max()) == 1 and int(rep.meta[1]) == E


BANK_SEED = 2468


def _bank_case(N):
    """(E, redrawn envs) of the bank-draw case at N.  The bank holds some 230 distinct starts: at N = 256
    the last agents find no separated start in 4096 attempts and take the last one (the rule's
    fall-back); the restatement then costs about a second per env, so fewer envs there."""
    E = C.small_E(N) + 4 if N < 256 else 2
    return E, ((E - 1,) if N == 256 else (0, E // 2, E - 1))


@functools.lru_cache(maxsize=None)
def _restated_draws(N):
    """bank_draw_batch for the case at N: episode 1 of every env, episode 2 of the redrawn ones (shared
    by the two reset forms, which must both land on it)."""
    from multi_agent_aac_amd import world
    from multi_agent_aac_amd.world import synthetic_map
    bank = world.ODBank(synthetic_map(2026), n_pairs=4096, seed=5, max_wp=W_DEFAULT)
    E, sel = _bank_case(N)
    return (bank_draw_batch(bank.start, bank.n_pairs, BANK_SEED, np.arange(E), np.ones(E, np.int64), N),
            bank_draw_batch(bank.start, bank.n_pairs, BANK_SEED, np.array(sel), np.full(len(sel), 2, np.int64), N))


@pytest.mark.parametrize("N", C.BANK_DRAW_N)
@pytest.mark.parametrize("compact", [1, 0])
def test_bank_auto_reset_draw(native_lib, occ, N, compact):
    """aac_env_auto_reset against helpers.bank_draw_batch: the pairwise-separation rule with up to
    255 earlier starts, over the packed list of done envs and over contiguous ranges, two episodes."""
    from multi_agent_aac_amd import _native, world
    (E, redrawn), seed = _bank_case(N), BANK_SEED
    bank = world.ODBank(occ, n_pairs=4096, seed=5, max_wp=W_DEFAULT)      # (occ is synthetic_map(2026))
    assert bank.n_pairs >= 4096
    env = _env(E, N, occ, "att", 0)
    env.set_od_bank(bank, seed=seed)
    lib = _native.lib()
    lib.aac_env_set_reset_compact(compact)
    try:
        env.auto_reset(None)
        torch.cuda.synchronize()
        s1 = {k: v.cpu().numpy() for k, v in env.get_state().items()}
        mask = np.zeros(E, np.uint8)
        mask[list(redrawn)] = 1
        env.auto_reset(torch.from_numpy(mask).cuda())
        torch.cuda.synchronize()
    finally:
        lib.aac_env_set_reset_compact(-1)
    s2 = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    sel = np.nonzero(mask)[0]
    idx1, redraw = _restated_draws(N)
    assert np.array_equal(s1["pos"], bank.start[idx1])
    assert np.array_equal(s1["wp"], bank.wps[idx1]) and np.array_equal(s1["wp_cnt"], bank.cnt[idx1])
    idx2 = idx1.copy()
    idx2[sel] = redraw
    assert np.array_equal(s2["pos"], bank.start[idx2]) and np.array_equal(s2["start"], bank.start[idx2])
    assert np.array_equal(s2["wp"], bank.wps[idx2]) and np.array_equal(s2["wp_cnt"], bank.cnt[idx2])
    assert (idx2[sel] != idx1[sel]).any()
    co = c_oracle.BatchedOracle(E, N, occ, W=W_DEFAULT, radar_mode=0)
    co.reset(bank.start[idx2], bank.wps[idx2], bank.cnt[idx2])
    np.testing.assert_allclose(env.bufs.radar.cpu().numpy()[sel], co.radar[sel], rtol=0, atol=ATOL)
    np.testing.assert_allclose(env.bufs.own.cpu().numpy()[sel], co.own[sel], rtol=0, atol=ATOL)


def test_epb_growth_at_two_agents(native_lib, occ):
    """E / epb_for(24) > 1024 at N = 2: the create-time loop raises epb from 12 to 13 (ragged last
    workgroup); the oracle steps a subset of 64 envs that includes the first and last workgroups."""
    E, N = C.EPB_GROWTH
    assert C.epb_of(E, N) == 13 and E % 13 != 0
    st, wps, cnt = C.make_od(occ, 64, N, seed=21)
    rep = (E + 63) // 64
    st, wps, cnt = (np.tile(a, (rep,) + (1,) * (a.ndim - 1))[:E] for a in (st, wps, cnt))
    env = _env(E, N, occ, "att", 2)
    env.reset(st, wps, cnt)
    sub = np.r_[0:16, np.random.default_rng(1).choice(np.arange(16, E - 16), 32, replace=False), E - 16:E]
    co = c_oracle.BatchedOracle(64, N, occ, W=W_DEFAULT, radar_mode=2)
    rng = np.random.default_rng(2)
    seen = 0
    for t in range(8):
        s = {k: v.cpu().numpy()[sub] for k, v in env.get_state().items()}
        co.pos[:] = s["pos"]; co.vel[:] = s["vel"]; co.pre_pos[:] = s["pre_pos"]; co.pre_vel[:] = s["pre_vel"]
        co.goal[:] = s["goal"]; co.wp[:] = s["wp"]; co.wp_cur[:] = s["wp_cur"]; co.wp_cnt[:] = s["wp_cnt"]
        co.reach[:] = s["reach"]; co.wall[:] = s["wall"]; co.step_count[:] = s["step"]; co.start[:] = s["start"]
        act = rng.uniform(-1, 1, size=(E, N, 2)).astype(np.float32)
        env.step(torch.from_numpy(act).cuda())
        co.step(act[sub])
        torch.cuda.synchronize()
        b = env.bufs
        for name in ("own", "radar", "nei", "reward"):
            np.testing.assert_allclose(getattr(b, name).cpu().numpy()[sub], getattr(co, name), rtol=0, atol=ATOL,
                                       err_msg=f"{name} t{t}")
        for name in ("mask", "done", "env_done", "bbc"):
            assert np.array_equal(getattr(b, name).cpu().numpy()[sub], getattr(co, name)), (name, t)
        np.testing.assert_allclose(env.get_state()["pos"].cpu().numpy()[sub], co.pos, rtol=1e-12, atol=1e-12)
        seen |= int(np.bitwise_or.reduce(co.mask.ravel()))
    assert seen


def _crowded_env(occ, N, mode, **kw):
    """An env standing on crowded_state(N) after a zero-action step (positions unchanged)."""
    E = 8 if N < 256 else 4
    st, wps, cnt = C.make_od(occ, E, N, seed=77)
    env = _env(E, N, occ, "att", mode, **kw)
    env.reset(st, wps, cnt)
    pos = C.crowded_state(E, N, C.CROWDED_SEED[N])
    z = np.zeros_like(pos)
    env.set_state(pos=pos, pre_pos=pos, vel=z, pre_vel=z)
    return env, pos


@pytest.mark.parametrize("N", [65, 256])
@pytest.mark.parametrize("mode", [0, 2])
def test_probe_on_crowded_states(native_lib, occ, N, mode):
    """The probe kernel's own copy of the radar past its first 64-candidate chunk: ``dist`` rounds to the
    step's fp32 radar bit for bit on every ray, and agents below 64 end rays on agents of every later
    block of 64; kind / id follow tests/probe_ref.py on the rays of up to three agents per env (the
    restatement is scalar Python, 5 to 17 ms a ray: all rays of 256 agents would take minutes), chosen
    where the records name agents >= 64, so the restatement has to confirm such records.  Rays whose
    two best candidates tie within 1e-9 (deep overlaps: several 64-gons at distance 0) are compared on
    dist only, as in test_probe_gpu."""
    from multi_agent_aac_amd.probe import RadarProbe
    from tests import probe_ref as R
    from tests.test_probe_gpu import TOL, _self_consistent
    env, pos = _crowded_env(occ, N, mode)
    E = env.E
    env.step(torch.zeros(E, N, 2, device="cuda"))
    probe = RadarProbe.for_env(env)
    probe.run()
    pr = probe.read()
    assert np.array_equal(env.get_state()["pos"].cpu().numpy(), pos)
    _self_consistent(pr, pos, env.bufs.radar.cpu().numpy(), f"crowded N{N} mode{mode}")
    drone = pr["kind"] == R.DRONE
    low = pr["id"][:, :64][drone[:, :64]]
    for b0 in range(64, N, 64):        # agents below 64 end rays on agents of every later block
        assert ((low >= b0) & (low < b0 + 64)).any(), b0
    assert (pr["id"][drone] < N).all() and (pr["id"][drone] >= 0).all()
    # per env: the first two agents below 64 with a record naming an agent >= 64, and the last agent
    full = named = rays = 0
    for m in range(E):
        hit = np.nonzero((drone[m, :64] & (pr["id"][m, :64] >= 64)).any(axis=1))[0][:2]
        for i in list(hit) + ([N - 1] if N < 256 else []):
            for r in range(18):
                ref = R.probe_ray(pos[m], i, r, occ, mode)
                rays += 1
                assert abs(pr["dist"][m, i, r] - ref["dist"]) <= TOL, (m, i, r)
                if ref["close"]:
                    continue
                full += 1
                assert (int(pr["kind"][m, i, r]), int(pr["id"][m, i, r])) == (ref["kind"], ref["id"]), (m, i, r, ref)
                named += ref["kind"] == R.DRONE and ref["id"] >= 64
    print(f"crowded N{N} mode{mode}: {rays} rays restated, {full} untied, {named} of them name an agent >= 64")
    assert rays >= 18 * E and full > 0 and named > 0, (rays, full, named)


def test_reward_map_rows_are_the_steps_rows_n65(native_lib, occ):
    """test_rewardmap_gpu.test_map_rows_are_the_steps_rows at N = 65: at rest on the crowded positions
    the map's row of every (env, agent) is the following zero-action step's row bit for bit."""
    from multi_agent_aac_amd.rewardmap import RewardMap
    from tests import terms_ref
    from tests.rewardmap_cases import all_rows
    from tests.test_rewardmap_gpu import _same_bits
    N = 65
    env, pos = _crowded_env(occ, N, 2, team_reward=False)
    E = env.E
    terms = env.use_terms_buffer()
    ei, ai = all_rows(E, N)
    rm = RewardMap.for_env(env)
    rm.at(pos.reshape(-1, 2), env=ei, agent=ai)
    got = rm.read()
    out = env.alloc_buffers()
    env.step(torch.zeros(E, N, 2, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state()["pos"].cpu().numpy(), pos)
    t = terms.cpu().numpy().reshape(E * N, 12)
    assert _same_bits(got["terms"], t), np.argwhere(got["terms"] != t)[:4].tolist()
    assert _same_bits(got["mask"], out.mask.cpu().numpy().reshape(-1))
    assert _same_bits(got["done"], out.done.cpu().numpy().reshape(-1))
    assert _same_bits(got["bbc"].reshape(E, N, 4).max(axis=1), out.bbc.cpu().numpy())
    assert np.array_equal(got["reward"], terms_ref.slot_sum(got["terms"]))
    assert np.array_equal(got["reward"].astype(np.float32), out.reward.cpu().numpy().reshape(-1))
    m = got["mask"].reshape(E, N)
    assert (m[:, 64] & 2).any() and (m & 2).any() and not (m & 2).all()      # contacts, the 65th agent's too
    assert len(np.unique(got["reward"])) > 50
