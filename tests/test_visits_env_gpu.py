"""The exploration maps behind the three real envs (aac_env_visits / aac_uam_visits through
``VisitMap``): ATT (E = 96, N = 3), WGRU on a 2-map stack (E = 96, N = 3) and UAM (E = 64, N = 5), 20
steps of seeded random actions with auto-reset, episode_length 6 (an episode lasts at most 7 steps, so
every env finishes at least two) and ``explore_until = 1`` (the first episode of an env is "explore",
the later ones "exploit").

Each step: act, ``visits.accumulate(act)``, env step (the fused tail with its auto-reset for ATT / WGRU;
step + auto-reset for UAM).  The restatement (tests/visits_ref.py) is fed the positions and map indices
of ``get_state()`` and the episode buffer, read before each step; the tables must be bit-equal."""
import numpy as np
import pytest
import torch

import visits_ref

pytestmark = pytest.mark.gpu

EP, STEPS = 6, 20
#        kind   E   N  maps  grid      A   seed
RUNS = [("att", 96, 3, 1, (50, 50), 20, 1), ("wgru", 96, 3, 2, (50, 50), 20, 2), ("uam", 64, 5, 1, (50, 50), 20, 3),
        ("att", 96, 3, 1, (7, 3), 32, 4)]


def _env(kind, E, N, maps, occ):
    from multi_agent_aac_amd import uam, world
    from multi_agent_aac_amd.env import BatchedEnv
    if kind == "uam":
        env = uam.BatchedUAM(E, N, episode_length=EP)
        env.set_bank(uam.build_bank(2048, N, seed=7), seed=11)
        return env
    if maps > 1:
        stack = world.map_stack(range(2026, 2026 + maps))
        env = BatchedEnv(E, N, stack, radar_mode=None, variant=kind, episode_length=EP)
        env.set_od_bank(world.MapBanks(stack, n_pairs=512, seed=7, max_wp=32), seed=11)
        return env
    env = BatchedEnv(E, N, occ, radar_mode="combined" if kind == "att" else None, variant=kind, episode_length=EP)
    env.set_od_bank(world.ODBank(occ, n_pairs=4096, seed=5, max_wp=32), seed=11)
    return env


@pytest.mark.parametrize("kind,E,N,maps,grid,A,seed", RUNS)
def test_maps_follow_the_env(native_lib, occ, kind, E, N, maps, grid, A, seed):
    from multi_agent_aac_amd.visits import VisitMap
    uam = kind == "uam"
    env = _env(kind, E, N, maps, occ)
    vm = (VisitMap.for_uam if uam else VisitMap.for_env)(env, grid=grid, act_bins=A, explore_until=1)
    assert (vm.n_maps, vm.E, vm.N) == (maps, E, N)
    assert VisitMap(env).explore_until == (10000 if uam else 8000)
    b = vm.bound
    ref = visits_ref.VisitsRef(maps, grid[0], grid[1], A, b[:2], b[2:])
    counter = env.use_episode_buffer(torch.zeros(E, dtype=torch.int32, device="cuda"))
    bufs = [env.alloc_buffers(), env.alloc_buffers()]
    env.auto_reset(None, out=bufs[0])
    g = torch.Generator(device="cuda").manual_seed(seed)
    adt = torch.float64 if uam else torch.float32
    # even envs: full-scale random accelerations (crashes, flights out of the bound); odd envs: 2 % of
    # them (the step limit).  A few actions are pushed past +-1: the map counts what it is given
    scale = torch.where(torch.arange(E, device="cuda") % 2 == 0, 1.0, 0.02).to(adt).view(E, 1, 1)
    done = 0
    for t in range(STEPS):
        n = bufs[1 - (t & 1)]
        act = (torch.rand(E, N, 2, device="cuda", generator=g, dtype=adt) * 2 - 1) * scale
        act[t % E, 0, 0] = 1.0
        act[(t + 1) % E, 0, 1] = -1.0
        act[(t + 2) % E, 0, 1] = 1.5
        s = env.get_state()
        mp = None if uam else s["map_idx"].cpu().numpy()
        ref.accumulate(s["pos"].cpu().numpy(), act.cpu().numpy(), counter.cpu().numpy(), 1, mp)
        vm.accumulate(act)
        if uam:
            env.step(act, out=n)
            done += int(n.env_done.sum())
            env.auto_reset(n.env_done, out=n)
        else:
            env.step_tail(act, out=n, replay=None)
            done += int(n.env_done.sum())
    out = vm.read()
    assert np.array_equal(out["pos"].reshape(ref.pos.shape), ref.pos)
    assert np.array_equal(out["act"], ref.act)
    for k, name in enumerate(("samples", "pos_outside", "act_outside")):
        assert np.array_equal(out[name].reshape(-1), ref.cnt[:, k]), name
    assert out["bad_map"] == 0 and out["explore_until"] == 1
    print(kind, "episodes finished", done, "samples", out["samples"].tolist(), "pos_outside", out["pos_outside"].tolist())
    assert done >= E and int(counter.min()) >= 2
    per_period = out["samples"].sum(axis=0)
    assert per_period[0] > 0 and per_period[1] > 0 and per_period.sum() == STEPS * E * N
    assert (out["samples"].sum(axis=1) > 0).all()                 # every map of the stack is flown
    assert out["act_outside"].sum() == STEPS and out["pos"].sum() + out["pos_outside"].sum() == STEPS * E * N
    assert np.array_equal(out["x_edges"], ref.ex) and np.array_equal(out["act_edges"], ref.ea)
    # read(clear=True) empties the tables; a second object's tensors are its own
    assert vm.read(clear=True)["pos"].sum() == out["pos"].sum() and vm.read()["samples"].sum() == 0
    assert set(vm.tensors()) == {"pos_hist", "act_hist", "counters"}


def test_wrong_action_tensor_is_refused(native_lib, occ):
    from multi_agent_aac_amd.visits import VisitMap
    env = _env("att", 8, 3, 1, occ)
    vm = VisitMap.for_env(env)
    with pytest.raises(ValueError, match="act"):
        vm.accumulate(torch.zeros(8, 3, 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="act"):
        vm.accumulate(torch.zeros(8, 2, 2, device="cuda"))
    with pytest.raises(ValueError, match="sel"):
        vm.accumulate(torch.zeros(8, 3, 2, device="cuda"), sel=torch.zeros(7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(TypeError):
        VisitMap.for_uam(env)
    with pytest.raises(ValueError):
        VisitMap.for_env(env, act_bins=33)
    assert vm.read()["samples"].sum() == 0
