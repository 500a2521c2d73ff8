"""The sortie statistics behind the three real envs (aac_env_sorties / aac_uam_sorties through
``SortieStats``): ATT (8 envs x 3), WGRU (6 x 3) and UAM (6 x 4), episode_length 8, 24 steps as separate
launches: env step, ``sorties.accumulate``, auto-reset.  The restatement (tests/sortie_ref.py) is fed the
positions, starts and goals of ``get_state()`` read between the step and the reset, and the step's outputs.

``set_state`` scripts the first episode of every env by its role (env index mod 5):
  0  every aircraft 3.6 step lengths short of its goal, flying at it            -> reached
  1  aircraft 1 moved to 0.8 pB from aircraft 0, both at rest                   -> drone
  2  left alone with small actions: the step limit ends the episode             -> idle, a timeout
  3  aircraft 0 just inside the bound, flying out                               -> bound
  4  aircraft 0 inside an occupied cell (ATT, WGRU) / flying into the runway (UAM)  -> obstacle
The restatement's own counts must show every class and a timeout before anything is compared; then
counters, collide_hist, running state and log rows are bit-equal and the double sums agree within
n * 2^-52 relative."""
import math

import numpy as np
import pytest
import torch

import sortie_ref

pytestmark = pytest.mark.gpu

EP, STEPS, LOG = 8, 24, 4096
#        kind   E  N  seed
RUNS = [("att", 8, 3, 1), ("wgru", 6, 3, 2), ("uam", 6, 4, 3)]


def _env(kind, E, N, occ):
    from multi_agent_aac_amd import uam, world
    from multi_agent_aac_amd.env import BatchedEnv
    if kind == "uam":
        env = uam.BatchedUAM(E, N, episode_length=EP)
        env.set_bank(uam.build_bank(2048, N, seed=7), seed=11)
        return env
    env = BatchedEnv(E, N, occ, radar_mode="combined" if kind == "att" else None, variant=kind, episode_length=EP)
    env.set_od_bank(world.ODBank(occ, n_pairs=4096, seed=5, max_wp=32), seed=11)
    return env


def _script(env, kind, occ):
    """The scripted first episode: returns the state tensors to inject."""
    c = env.cfg
    s = {k: v.cpu().numpy() for k, v in env.get_state().items()}
    pos, vel, goal = s["pos"].copy(), s["vel"].copy(), s["goal"]
    hop, pb, b = c.vmax * c.dt, c.pB, tuple(c.bound)
    for e in range(env.E):
        role = e % 5
        if role == 0:
            d = goal[e] - pos[e]
            u = d / np.linalg.norm(d, axis=-1, keepdims=True)
            pos[e], vel[e] = goal[e] - 3.6 * hop * u, c.vmax * u
        elif role == 1:
            pos[e, 1], vel[e, :2] = pos[e, 0] + [0.8 * pb, 0.0], 0.0
        elif role == 3:
            pos[e, 0], vel[e, 0] = [b[0] + pb + 0.3 * hop, 0.5 * (b[2] + b[3])], [-c.vmax, 0.0]
        elif role == 4 and kind == "uam":
            pos[e, 0], vel[e, 0] = [18.0 - pb - 0.3 * hop, 20.0], [c.vmax, 0.0]      # the runway's x0 edge
        elif role == 4:
            gx0, gy0 = math.ceil(b[0] / c.cell) * c.cell, math.ceil(b[2] / c.cell) * c.cell
            ii, jj = next((i, j) for i in range(3, occ.shape[0] - 3) for j in range(3, occ.shape[1] - 3) if occ[i, j])
            pos[e, 0], vel[e, 0] = [gx0 + c.cell * ii, gy0 + c.cell * jj], 0.0
    return dict(pos=pos, pre_pos=pos, vel=vel, pre_vel=vel)


def _actions(env, kind, g, adt):
    E, N = env.E, env.N
    s = env.get_state()
    d = s["goal"] - s["pos"]
    act = (torch.rand(E, N, 2, device="cuda", generator=g, dtype=torch.float64) * 2 - 1) * 0.02
    for e in range(E):
        if e % 5 == 0:
            act[e] = d[e] / d[e].norm(dim=-1, keepdim=True).clamp_min(1e-9)
        elif e % 5 == 3:
            act[e, 0, 0], act[e, 0, 1] = -1.0, 0.0
        elif e % 5 == 4 and kind == "uam":
            act[e, 0, 0], act[e, 0, 1] = 1.0, 0.0
    return act.to(adt).contiguous()


@pytest.mark.parametrize("kind,E,N,seed", RUNS)
def test_sorties_follow_the_env(native_lib, occ, kind, E, N, seed):
    from multi_agent_aac_amd.sorties import COUNTERS, DOUBLES, SortieStats
    uam = kind == "uam"
    env = _env(kind, E, N, occ)
    ss = (SortieStats.for_uam if uam else SortieStats.for_env)(env, log=LOG)
    assert ss.reach_margin == (5.0 if uam else 0.0) and (ss.E, ss.N, ss.episode_length) == (E, N, EP)
    ref = sortie_ref.SortieRef(E, N, EP, ss.reach_margin, **(sortie_ref.BITS_UAM if uam else sortie_ref.BITS_ENV))
    counter = env.use_episode_buffer(torch.zeros(E, dtype=torch.int32, device="cuda"))
    bufs = [env.alloc_buffers(), env.alloc_buffers()]
    env.auto_reset(None, out=bufs[0])
    env.set_state(**_script(env, kind, occ))
    g = torch.Generator(device="cuda").manual_seed(seed)
    adt = torch.float64 if uam else torch.float32
    timeouts = 0
    for t in range(STEPS):
        n = bufs[1 - (t & 1)]
        env.step(_actions(env, kind, g, adt), out=n)
        ss.accumulate(n)
        s = env.get_state()
        ed = n.env_done.cpu().numpy()
        timeouts += int(((ref.run_len + 1 > EP) & (ed != 0)).sum())
        ref.accumulate(s["pos"].cpu().numpy(), s["start"].cpu().numpy(), s["goal"].cpu().numpy(), n.done.cpu().numpy(),
                       n.mask.cpu().numpy(), ed, None, counter.cpu().numpy())
        env.auto_reset(n.env_done, out=n)
    print(kind, ref.cnt, "timeouts", timeouts, "collide_hist", ref.collide_hist.tolist(), "ratios", ref.ratios)
    # the run exercises what it is for, by the restatement's own counts
    assert all(ref.cnt[k] > 0 for k in sortie_ref.CLASSES), ref.cnt
    assert timeouts > 0 and ref.collide_hist.sum() > 0 and len(ref.ratios) > 0
    assert ref.cnt["episodes"] >= 2 * E and ref.cnt["sorties"] == N * ref.cnt["episodes"]

    rows = ss.log_rows()
    want_rows = ref.log_rows()
    assert rows.dtype == want_rows.dtype and rows.tobytes() == want_rows.tobytes()
    got_t = {k: v.cpu().numpy() for k, v in ss.tensors().items()}
    for k, v in ref.running().items():
        assert got_t[k].tobytes() == v.astype(got_t[k].dtype).tobytes(), k
    out = ss.read()
    assert {k: out[k] for k in COUNTERS} == ref.cnt
    assert np.array_equal(out["collide_hist"], ref.collide_hist)
    want, cnt = ref.sums()
    for k in DOUBLES:
        print(f"{k}: got {out[k]!r} want {want[k]!r} n {cnt}")
        if k in ("ratio_min", "ratio_max"):
            assert out[k] == want[k], k
        else:
            assert abs(out[k] - want[k]) <= cnt * 2.0 ** -52 * abs(want[k]), (k, out[k], want[k])
    r = np.array(ref.ratios)
    assert abs(out["ratio_mean"] - r.mean()) <= 4 * cnt * 2.0 ** -52 * r.mean()
    # the std comes from sum and sum of squares: its absolute error is that of the mean square
    assert abs(out["ratio_std"] ** 2 - r.std() ** 2) <= 8 * cnt * 2.0 ** -52 * float((r * r).mean())
    assert out["mean_reach_step"] == ref.cnt["reach_step_sum"] / ref.cnt["reached"]
    # read(clear=True) empties totals and histogram; the episode counts stay
    again = ss.read(clear=True)
    assert again["sorties"] == out["sorties"] and np.array_equal(again["collide_hist"], out["collide_hist"])
    empty = ss.read()
    assert empty["sorties"] == 0 and empty["collide_hist"].sum() == 0 and math.isnan(empty["ratio_mean"])
    assert int(ss.ep_count.sum()) == ref.cnt["episodes"]


def test_wrong_buffers_are_refused(native_lib, occ):
    from multi_agent_aac_amd.sorties import SortieStats
    env = _env("att", 8, 3, occ)
    ss = SortieStats.for_env(env)
    other = _env("att", 4, 3, occ)
    with pytest.raises(ValueError, match="done"):
        ss.accumulate(other.alloc_buffers())
    with pytest.raises(ValueError, match="quota"):
        ss.accumulate(env.alloc_buffers(), quota=torch.zeros(7, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        SortieStats.for_uam(env)
    with pytest.raises(ValueError):
        SortieStats.for_env(env, reach_margin=float("nan"))
    assert ss.read()["sorties"] == 0 and ss.log_rows().shape == (0,)
