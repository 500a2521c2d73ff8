"""The UAM env kernels at the aircraft counts that leave idle lanes in the workgroup's wave or fill it
(tests/agent_count_cases.py UAM_N: 7 -> 9 envs and one idle lane, 33 and 63 -> one env and 31 / 1 idle
lanes, 64 -> the full wave) against oracle/uam_ref.py, with the bars of test_uam_gpu (masks / done / bbc
/ env_done bit-exact, float64 outputs within 1e-9, state within 1e-12).

The reference's episode draw cannot place more than some thirty starts 3 pB apart in its two start
zones (sample_episode(33) does not return; aac_uam_bank_build refuses more than 40), so from N = 33 the starts are
placed: columns 1.6 m apart beside the runway, on the zones' sides of it, goals from the reference's
end regions."""
import random

import numpy as np
import pytest
import torch

from oracle import uam_ref as U
from tests import agent_count_cases as C
from tests import test_uam_gpu as T

pytestmark = pytest.mark.gpu


def _episodes(E, N, seed):
    if N <= 16:
        return T._episodes(E, N, seed)
    py, npr = random.Random(seed), np.random.RandomState(seed)
    st, go, cl = [], [], []
    for _ in range(E):
        c0, c1 = py.choice(range(len(U.CLOUDS))), py.choice(range(len(U.GO_AC)))
        # two blocks of 4 columns x 8 rows beside the runway (x 11.2 .. 16, 24 .. 28.8; y 13.6 .. 24.8),
        # 1.6 m = 3.2 pB apart, jittered by less than 0.04 m
        cols = np.r_[11.2 + 1.6 * np.arange(4), 24.0 + 1.6 * np.arange(4)]
        grid = np.stack(np.meshgrid(cols, 13.6 + 1.6 * np.arange(8), indexing="ij"), -1).reshape(-1, 2)
        s = grid[npr.permutation(len(grid))[:N]] + npr.uniform(-0.02, 0.02, (N, 2))
        g = []
        for i in range(N):
            regs = U.end_regions(c0, s[i, 0])
            r = regs[npr.randint(0, len(regs))]
            g.append([npr.uniform(r[0], r[1]), npr.uniform(r[2], r[3])])
        st.append(s)
        go.append(g)
        cl.append((c0, c1))
    return np.array(st), np.array(go), np.array(cl, dtype=np.int32)


@pytest.mark.parametrize("N", C.UAM_N)
def test_uam_step_matches_oracle(native_lib, N):
    """test_uam_gpu._stepped_pair (every env checked against the oracle from the device's own pre-step
    state): reset + 2 steps, E = 2 epb + 1.  The states are not quiet ones: rays end below the radar
    range, and from 33 aircraft (1.6 m apart, full actions) mask bits are set."""
    from multi_agent_aac_amd import uam
    epb = 64 // N
    E = 2 * epb + 1
    eps = _episodes(E, N, 70 + N)
    masks, conf = T._stepped_pair(N, E, 70 + N, 2, episodes=eps)
    assert len(masks) == 2 and masks[0].shape == (E, N)
    env = uam.BatchedUAM(E, N)
    env.reset(*eps)
    torch.cuda.synchronize()
    assert (env.bufs.radar.cpu().numpy() < U.RADAR_DIST).mean() > 0.05       # radar returns at the start already
    if N >= 33:
        assert any(m.any() for m in masks)


def test_uam_compact_reset_bit_exact_n7(native_lib):
    _compact_reset_pair(7, 40, None)


def test_uam_compact_reset_bit_exact_n64(native_lib):
    """The full wave: a bank assembled from placed episodes (the reference's draw has no room for 64)."""
    from multi_agent_aac_amd import uam
    _compact_reset_pair(64, 5, uam.Bank(*_episodes(48, 64, 9)))


def _compact_reset_pair(N, E, bank):
    """test_uam_gpu.test_uam_compact_reset_bit_exact: the auto-reset over the compacted list of done envs
    against the one over contiguous ranges, same bank and actions, every output and state tensor."""
    from multi_agent_aac_amd import uam
    bank = bank or uam.build_bank(512, N, seed=9)
    envs = []
    for _ in range(2):
        env = uam.BatchedUAM(E, N, neighbours=True)
        env.set_bank(bank, seed=77)
        envs.append(env)
    rng = np.random.default_rng(4)
    lib = uam.lib()
    resets = 0
    try:
        for mode, env in zip((1, 0), envs):
            lib.aac_uam_set_reset_compact(mode)
            env.auto_reset()
        for k in range(8):
            act = torch.from_numpy(rng.uniform(-1, 1, (E, N, 2))).to(T.DEV)
            for mode, env in zip((1, 0), envs):
                lib.aac_uam_set_reset_compact(mode)
                env.step(act)
                env.auto_reset(env.bufs.env_done)
            torch.cuda.synchronize()
            done = envs[0].bufs.env_done.cpu().numpy().astype(bool)
            resets += int(done.sum())
            a, b = envs
            for name in a.bufs.__dict__:
                x, y = getattr(a.bufs, name), getattr(b.bufs, name)
                if isinstance(x, torch.Tensor):
                    assert torch.equal(x, y), (k, name)
            sa, sb = a.get_state(), b.get_state()
            for key in sa:
                assert torch.equal(sa[key], sb[key]), (k, key)
            if done.any():      # a reset env stands on one of the bank's episodes
                s0 = sa["start"].cpu().numpy()[done]
                assert all((bank.start == s).all(axis=(1, 2)).any() for s in s0)
    finally:
        lib.aac_uam_set_reset_compact(1)
    assert resets > 0 and not (N == 64 and resets == 8 * E)        # some envs reset, not all of them every step


def test_uam_probe_dist_is_the_steps_radar_n64(native_lib):
    """UamRadarProbe.run() ``dist`` bit for bit the radar of reset and of two steps at the full wave."""
    from multi_agent_aac_amd import uam
    from multi_agent_aac_amd.probe import UamRadarProbe
    from tests import uam_probe_ref as R
    E, N = 3, 64
    st, go, cl = _episodes(E, N, 164)
    env = uam.BatchedUAM(E, N)
    pr = UamRadarProbe.for_uam(env)
    rng = np.random.default_rng(6)
    ids = set()

    def same(out, where):
        got = pr.read(pr.run())
        radar = out.radar.cpu().numpy()
        assert got["dist"].shape == radar.shape == (E, N, 18)
        assert np.array_equal(got["dist"].view(np.int64), radar.view(np.int64)), (where, np.argwhere(got["dist"] != radar)[:5])
        ids.update(np.unique(got["id"][got["kind"] != R.NONE]).tolist())
        return int((got["kind"] != R.NONE).sum())

    hits = [same(env.reset(st, go, cl), "reset")]
    for s in range(2):
        hits.append(same(env.step(torch.as_tensor(rng.uniform(-1, 1, (E, N, 2)), device=T.DEV)), f"step {s}"))
    assert min(hits) > E * N                   # more than a ray per aircraft ends on something
    assert max(ids) >= 60 and min(ids) <= 3    # records name aircraft across the whole wave


def test_bank_build_refuses_more_aircraft_than_the_start_zones_hold(native_lib):
    """aac_uam_bank_build past 40 aircraft (aac_uam_create accepts up to 64): no more than 40 starts
    3 pB apart fit the two start zones (disc packing: 20 discs of radius 0.75 m in a 3.5 m x 11.5 m
    rectangle at density pi / sqrt(12)); the call returns an error at once, where it used to spend
    100000 draws on every aircraft it could not place.  40 is still accepted; N = 16 (config 5) builds
    separated starts as before."""
    import math
    import time
    from multi_agent_aac_amd import uam
    assert math.floor(3.5 * 11.5 * (math.pi / math.sqrt(12)) / (math.pi * 0.75 ** 2)) == 20
    for N in (41, 64):
        t0 = time.perf_counter()
        with pytest.raises(RuntimeError, match="cannot hold more than 40"):
            uam.build_bank(512, N, seed=9)
        assert time.perf_counter() - t0 < 1.0
    assert uam.build_bank(1, 40, seed=9).start.shape == (1, 40, 2)
    bk = uam.build_bank(64, 16, seed=9)
    d = np.linalg.norm(bk.start[:, :, None] - bk.start[:, None], axis=-1) + np.eye(16) * 9
    assert d.min() > 1.5
