"""Agent counts for the env kernels: which N hits which branch, and the inputs to run them with.

aac_env_create takes 2 <= N <= 256 (aac_uam_create 2 <= N <= 64) and the kernels branch on N and on
nag = epb * N, the agents of one 256-thread workgroup.  This module restates the create-time rules in
Python (``epb_of``, ``staged``, ``branches``) and lists, per branch, the counts on either side of it;
tests/test_agent_count_cases_cpu.py keeps the lists honest, tests/test_env_agent_counts_gpu.py and
tests/test_uam_agent_counts_gpu.py run them.

Branches of csrc/aac_env.hip (values at small E, where epb = epb_for(24)):
  radar_chunks   radar_ray / probe / reward map collect drone candidates per 64 agents:   64 | 65, 128 | 129, 192 | 193
  agent_waves    slots t / N packed into the first (nag + 63) / 64 waves:                 64 | 65 ... 192 | 193 (no agent-free wave)
  spec           speculative OD draw of the fused tail: nag <= 84 and agent_waves < 4:    84 | 85
  late_copy      ring copy by agent-free waves: agent_waves < 4:                          192 | 193
  prefetch_all   WGRU: the 8 cached waypoints per agent held across the radar, nag <= 64: 64 | 65
  staged         own | nei rows staged in LDS, nag (D0 + 6 K) <= 2560:   ATT 12 (no) 16 (yes) 17 (no); WGRU 20 | 21
  epb            envs per workgroup, epb_for(24): 12, 2, 2, 1 at N = 2, 9, 12, 13+; raised towards epb_for(50)
                 while E / epb > 1024 (epb_grown: E = 12 * 1024 + 5 at N = 2)
LDS bounds the kernel derives by hand (asserted for every N by the CPU test): S.idx[nag + 2 epb] and
spec_starts inside S.rmin[256] whenever spec is on; a thread's flagged-ray mask has nag * 18 / 256 <= 32 bits.
UAM (csrc/aac_uam.hip): epb = 64 / N, idle lanes 64 - epb * N: 7 (9 envs, 1 idle), 33 and 63 (1 env,
31 and 1 idle), 64 (full wave).

Inputs.  ``random_od`` (the reference's draw) up to N = 85; above that ``placed_od``: its rejection loop
needs starts 5 m apart out of a few hundred pool cells and does not terminate at N = 256.
``crowded_state`` is the construction of
test_radar_crowded_bit_exact for any N; for N > 64 it is valid only if ``second_chunk_matters``.

Measured CPU cost (this project's C oracle, one core; GPU side is milliseconds per case):
  random_od per env      N = 9 0.01 s, 25 0.02 s, 51 0.04 s, 65 0.05 s, 85 0.07 s, 129 0.11 s, 193 0.24 s, 256 never ends
  oracle reset = step    per env, combined radar: N = 25 3 ms, 51 9 ms, 65 15 ms, 85 25 ms, 129 58 ms, 193 127 ms;
                         drone radar on placed ODs: 193 125 ms, 256 220 ms (N^2); WGRU (obstacle radar) 256: 4 ms
  placed_od              under 10 ms at any N
  bank_draw_batch        E = 7: N = 64 0.03 s, 85 0.05 s; N = 256: about 1 s per env (the bank has some 230
                         distinct starts, so the last agents run all 4096 attempts)
  UAM oracle/uam_ref.py  N = 7: sample_episode, reset and step 10 ms each per env; 33: 0.1 s, 64: 0.35 s per call.
                         sample_episode(33) does not return (33 starts 3 pB apart do not fit its start zones) and
                         aac_uam_bank_build refuses more than 40 aircraft: N >= 33 uses placed starts
  tests/probe_ref.py     probe_ray on the crowded states: 5 ms a ray at N = 65, 17 ms at N = 256
so with E = 2 epb + 1 (3 envs from N = 13 up) and 6 steps + resets the N = 256 drone-radar case costs about
7 s of oracle, N = 193 about 4 s, everything else under 2 s.
"""
import numpy as np

from oracle.consts import BOUND

BLOCK, WAVE = 256, 64
OBS_STAGE_FLOATS = 2560
SPEC_MAX_AG = 84
WPC, WPI = 8, 2
N_MAX, UAM_N_MAX = 256, 64
E_CAP = 25                      # E = 2 epb + 1, capped here (N = 2: epb 12)


def epb_for(apw, N):
    return 1 if N > apw else apw // N


def epb_of(E, N):
    """Envs per workgroup as aac_env_create chooses them (no AAC_ENV_AGENTS_PER_WG)."""
    if E // epb_for(50, N) >= 1024:
        return epb_for(50, N)
    epb = epb_for(24, N)
    while epb < epb_for(50, N) and (E + epb - 1) // epb > 1024:
        epb += 1
    return epb


def row_floats(variant, N):
    K = N - 1
    return (6 if variant == "wgru" else 6 + 4 * K) + 6 * K


def staged(variant, E, N):
    """Whether the step kernel stages the workgroup's own | nei rows in LDS."""
    return epb_of(E, N) * N * row_floats(variant, N) <= OBS_STAGE_FLOATS


def branches(variant, E, N):
    epb = epb_of(E, N)
    nag = epb * N
    waves = (nag + WAVE - 1) // WAVE
    return dict(epb=epb, nag=nag, radar_chunks=(N + WAVE - 1) // WAVE, agent_waves=waves,
                spec=nag <= SPEC_MAX_AG and waves < BLOCK // WAVE, late_copy=waves < BLOCK // WAVE,
                prefetch_all=nag * WPC <= WPI * BLOCK, staged=staged(variant, E, N),
                epb_grown=epb > epb_for(24, N), ragged=E % epb != 0)


def small_E(N):
    """2 epb + 1 envs: two full workgroups and a ragged third."""
    return min(2 * epb_for(24, N) + 1, E_CAP)


# step + reset parity: (variant, N, radar mode, tdcpa, team_reward)
ATT_N = (2, 9, 12, 16, 17, 25, 51, 64, 65, 84, 85, 129, 193, 256)
WGRU_N = (2, 8, 9, 20, 21, 33, 64, 65, 129, 256)
PARITY = ([("att", N, 2, N in (2, 9, 65), True) for N in ATT_N if N <= 85] +
          [("att", N, 0, False, True) for N in ATT_N if N > 85] +          # (combined up to 85; the drone radar above)
          [("att", N, m, False, True) for N in (2, 65, 256) for m in (0, 1) if not (N == 256 and m == 0)] +
          [("att", N, 2, False, False) for N in (9, 85)] +                 # per-agent reward: the other side of team_reward
          [("wgru", N, 1, False, False) for N in WGRU_N])
CROWDED = [(N, mode) for N in (9, 64, 65, 130, 256) for mode in (0, 2)]
CROWDED_SEED = {9: 40, 64: 40, 65: 40, 130: 40, 256: 40}
TAIL_RING = [("att", 2), ("att", 9), ("att", 16), ("wgru", 2), ("wgru", 9), ("wgru", 20)]
TAIL_NO_RING = [("att", 17), ("att", 84), ("att", 85), ("att", 193), ("wgru", 21), ("wgru", 65)]
TOO_WIDE = [("att", 17), ("wgru", 21)]
BANK_DRAW_N = (2, 64, 85, 256)
EPB_GROWTH = (12 * 1024 + 5, 2)
UAM_N = (7, 33, 63, 64)

# every branch with the counts that take it each way: {branch: {value: [(variant, E, N), ...]}}
def _sides():
    cases = {(v, small_E(N), N) for v, N, *_ in PARITY} | {(v, 40, N) for v, N in TAIL_RING + TAIL_NO_RING}
    cases |= {("att", 8 if N < 256 else 4, N) for N, _ in CROWDED} | {("att", EPB_GROWTH[0], EPB_GROWTH[1])}
    out = {}
    for v, E, N in sorted(cases):
        for k, val in branches(v, E, N).items():
            out.setdefault(k, {}).setdefault(val, []).append((v, E, N))
    return out


SIDES = _sides()


def steps_for(N):
    return 6 if N >= 129 else 10


def _free_lattice(occ, pitch=5.2, margin=6.0):
    """Points of a square lattice (pitch > 2 pB, so any two are a legal pair of starts) that lie in a
    free cell, `margin` inside the bounds."""
    xs = np.arange(BOUND[0] + margin, BOUND[1] - margin, pitch)
    ys = np.arange(BOUND[2] + margin, BOUND[3] - margin, pitch)
    p = np.stack(np.meshgrid(xs, ys, indexing="ij"), -1).reshape(-1, 2)
    gx0, gy0 = np.ceil(BOUND[0] / 10.0) * 10.0, np.ceil(BOUND[2] / 10.0) * 10.0
    ci = np.floor((p[:, 0] - gx0) / 10.0 + 0.5).astype(int)
    cj = np.floor((p[:, 1] - gy0) / 10.0 + 0.5).astype(int)
    ok = (ci >= 0) & (cj >= 0) & (ci < occ.shape[0]) & (cj < occ.shape[1])
    ok[ok] &= occ[ci[ok], cj[ok]] == 0
    for di in (-1, 0, 1):                   # and more than pB (+ 0.5 m) away from every occupied cell's square
        for dj in (-1, 0, 1):
            ii, jj = np.clip(ci + di, 0, occ.shape[0] - 1), np.clip(cj + dj, 0, occ.shape[1] - 1)
            dx = np.maximum(np.abs(p[:, 0] - (gx0 + 10.0 * ii)) - 5.0, 0.0)
            dy = np.maximum(np.abs(p[:, 1] - (gy0 + 10.0 * jj)) - 5.0, 0.0)
            ok &= ~((occ[ii, jj] != 0) & (np.hypot(dx, dy) < 3.0))
    return p[ok]


def placed_od(occ, E, N, seed, W=32):
    """ODs by direct placement: distinct lattice points in free cells as starts (pairwise > 2 pB), a
    free lattice point as goal, straight lists of 1..3 waypoints (the last is the goal).  The kernels
    under test do not care how the OD was drawn; random_od cannot draw this many separated starts."""
    rng = np.random.default_rng(seed)
    lat = _free_lattice(occ)
    assert len(lat) >= N, (len(lat), N)
    st = np.zeros((E, N, 2))
    wps = np.zeros((E, N, W, 2))
    cnt = rng.integers(1, 4, size=(E, N)).astype(np.int32)
    for e in range(E):
        st[e] = lat[rng.permutation(len(lat))[:N]]
        goal = lat[rng.integers(0, len(lat), size=N)]
        for i in range(N):
            f = np.arange(1, cnt[e, i] + 1)[:, None] / cnt[e, i]
            wps[e, i, :cnt[e, i]] = st[e, i] + f * (goal[i] - st[e, i])
            wps[e, i, cnt[e, i]:] = goal[i]
    return st, wps, cnt


def make_od(occ, E, N, seed, W=32):
    from tests.helpers import random_od
    return random_od(occ, E, N, seed, W) if N <= 85 else placed_od(occ, E, N, seed, W)


def crowded_state(E, N, seed):
    """The positions of test_radar_crowded_bit_exact for any N: a centre per env, agents at
    normal(scale = 3 m), deep overlaps, agents on cell corners, cell edges and the bound lines."""
    assert E % 4 == 0
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(BOUND[0] - 5, BOUND[1] + 5, E), rng.uniform(BOUND[2] - 5, BOUND[3] + 5, E)], -1)
    pos = centre[:, None, :] + rng.normal(scale=3.0, size=(E, N, 2))
    pos[::4, 1] = pos[::4, 0] + rng.uniform(-1, 1, size=(len(pos[::4]), 2))
    edge = rng.integers(0, 22, size=(E // 4, N, 2))
    pos[1::4] = np.stack([455.0 + 10 * edge[..., 0], 255.0 + 10 * np.minimum(edge[..., 1], 13)], -1)
    pos[1::4, :, 1] += rng.integers(0, 2, size=(E // 4, N)) * rng.uniform(0, 10, size=(E // 4, N))
    pos[2::8, 0, 0] = BOUND[0]
    pos[3::8, 0, 1] = BOUND[3]
    return pos


def drone_radar(occ, pos):
    """The oracle's drone radar (mode 0) of the agents at pos (E, M, 2)."""
    from oracle import c_oracle
    E, M = pos.shape[:2]
    co = c_oracle.BatchedOracle(E, M, occ, W=1, radar_mode=0)
    co.pos[:] = pos
    co.pre_pos[:] = pos
    co.observe()
    return co.radar.copy()


def second_chunk_matters(occ, pos):
    """For N > 64: per block of 64 agents past the first, whether taking it away changes a ray of an
    agent below 64 -- the condition under which a kernel that skipped that candidate chunk would fail."""
    N = pos.shape[1]
    full = drone_radar(occ, pos)[:, :64]
    out = {}
    for b0 in range(64, N, 64):
        keep = np.r_[0:b0, min(b0 + 64, N):N]
        out[b0] = bool((drone_radar(occ, pos[:, keep])[:, :64] != full).any())
    return out
