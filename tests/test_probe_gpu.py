"""Radar probes on the GPU (include/aac_probe.h, ``probe.RadarProbe``): the probe's double distance
rounds to the step / reset / band-fix launches' fp32 radar bit for bit (threshold-band rays included),
its hit point lies at exactly that distance, kind / id follow the restatement of tests/probe_ref.py and
the hand-built ties; ``at()`` shapes, row selection and a canary arena; read-only; graph replay;
``for_trajectories``."""
import numpy as np
import pytest
import torch

from tests import probe_cases as C
from tests import probe_ref as R
from tests import thresholds as T
from tests.arena import Arena

pytestmark = pytest.mark.gpu
TOL = 1e-9          # the project's fp64 parity bar
FIELDS = ("dist", "point", "end", "kind", "id")


def _np(t):
    return t.detach().cpu().numpy()


def _env(E, N, occ, mode, variant="att", **kw):
    from multi_agent_aac_amd.env import BatchedEnv
    return BatchedEnv(E, N, occ, radar_mode=mode, max_wp=32, variant=variant, **kw)


def _probe(env):
    from multi_agent_aac_amd.probe import RadarProbe
    return RadarProbe.for_env(env)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ends(pos):
    """thresholds.ray_end of every (row, agent, ray)."""
    M, N = pos.shape[:2]
    return np.array([[[T.ray_end((float(pos[m, i, 0]), float(pos[m, i, 1])), r) for r in range(18)]
                      for i in range(N)] for m in range(M)])


def _self_consistent(pr, pos, radar, where):
    """The three bitwise identities of every ray against the env's own outputs and positions."""
    assert _same_bits(pr["dist"].astype(np.float32), radar), where + ": float32(dist) != radar"
    assert _same_bits(pr["end"], _ends(pos)), where + ": end"
    dx, dy = pr["point"][..., 0] - pos[:, :, None, 0], pr["point"][..., 1] - pos[:, :, None, 1]
    assert _same_bits(np.sqrt(dx * dx + dy * dy), pr["dist"]), where + ": |point - pos| != dist"
    assert np.array_equal(pr["kind"] == 0, pr["id"] == -1), where
    none = pr["kind"] == 0
    assert _same_bits(pr["point"][none], pr["end"][none]), where + ": a none record's point is the ray end"


def _against_ref(pr, pos, stack, mode, map_idx, where, excuse=True):
    """kind / id equal and dist / point / end within TOL of tests/probe_ref.py; rays whose two best
    candidates lie within 1e-9 there are compared on dist only (at most 1 % of the case's rays)."""
    ref = R.probe_rows(pos, stack, mode, map_idx)
    np.testing.assert_allclose(pr["dist"], ref["dist"], rtol=0, atol=TOL, err_msg=where + " dist")
    np.testing.assert_allclose(pr["end"], ref["end"], rtol=0, atol=TOL, err_msg=where + " end")
    full = ~ref["close"] if excuse else np.ones_like(ref["close"])
    excused = int((~full).sum())
    print(f"{where}: {excused} of {full.size} rays excused; kinds {np.bincount(pr['kind'].ravel(), minlength=4)}")
    assert excused <= 0.01 * full.size, (where, excused)
    assert np.array_equal(pr["kind"][full], ref["kind"][full]), where + " kind"
    assert np.array_equal(pr["id"][full], ref["id"][full]), where + " id"
    np.testing.assert_allclose(pr["point"][full], ref["point"][full], rtol=0, atol=TOL, err_msg=where + " point")
    return ref


# ------------------------------------------------------------------ 1 + 3: the env's own states
@pytest.mark.parametrize("name", list(C.CASES))
def test_probe_follows_reset_step_autoreset(native_lib, occ, name):
    from multi_agent_aac_amd import world
    mode, N, variant = C.CASES[name]
    st, wps, cnt, stack, mi = C.reset_state(occ, name)
    env = _env(C.E, N, stack, mode, variant)
    if stack.ndim == 3:
        env.set_od_bank(world.MapBanks(stack, n_pairs=512, seed=7, max_wp=32), seed=11)
    else:
        env.set_od_bank(world.ODBank(stack, n_pairs=512, seed=5, max_wp=32), seed=11)
    probe = _probe(env)
    seen = np.zeros(4, np.int64)

    def check(where):
        probe.run()
        pr = probe.read()
        s = env.get_state()
        pos, midx = _np(s["pos"]), _np(s["map_idx"])
        _self_consistent(pr, pos, _np(env.bufs.radar), where)
        _against_ref(pr, pos, stack, mode, midx if stack.ndim == 3 else None, where)
        assert sum(probe.summary().values()) == pr["kind"].size
        assert [probe.summary()[k] for k in probe.KINDS] == np.bincount(pr["kind"].ravel(), minlength=4).tolist()
        seen[:] += np.bincount(pr["kind"].ravel(), minlength=4)

    env.reset(st, wps, cnt, map_idx=mi)
    check(f"{name} reset")
    for a in C.actions(name):
        env.step(torch.from_numpy(a).cuda())
    check(f"{name} step 3")
    half = torch.from_numpy((np.arange(C.E) % 2).astype(np.uint8)).cuda()
    env.auto_reset(half)
    check(f"{name} auto_reset")
    want = {0: (0, 1), 1: (0, 2, 3), 2: (0, 1, 2, 3)}[mode]
    # (drone hits need two agents within 17.5 m: the clustered rows of the at() test have them)
    assert all(seen[k] > 0 for k in want if k != 1) and seen[[k for k in range(4) if k not in want]].sum() == 0, seen


def test_isolated_agents_see_nothing(native_lib, occ):
    """The drone radar with nobody in reach: every record is none.  (N = 1 itself cannot be built:
    aac_env_create refuses a handle with fewer than two agents.)"""
    env = _env(4, 2, occ, 0)
    probe = _probe(env)
    pos = np.array([[(500.0 + 7 * e, 300.0 + 3 * e), (500.0 + 7 * e, 340.0 + 3 * e)] for e in range(4)])   # 40 m apart
    probe.at(pos)
    pr = probe.read()
    assert (pr["kind"] == 0).all() and (pr["id"] == -1).all()
    assert _same_bits(pr["point"], pr["end"]) and _same_bits(pr["end"], _ends(pos))
    assert probe.summary() == {"none": 4 * 2 * 18, "drone": 0, "cell": 0, "bound": 0}


# ------------------------------------------------------------------ 2: threshold states (flagged rays)
def _install(env, st):
    E, N = st["pos"].shape[:2]
    env.set_state(pos=st["pos"], pre_pos=st["pre_pos"], vel=st["vel"], pre_vel=st["vel"], goal=st["goal"],
                  wp=st["wp"], wp_cur=np.zeros((E, N), np.int32), wp_cnt=st["cnt"],
                  reach=np.zeros((E, N), np.uint8), wall=np.zeros((E, N), np.int32), step=np.zeros(E, np.int32),
                  map_idx=np.zeros(E, np.int32), start=st["pos"])


@pytest.mark.parametrize("N,variant,mode", [(3, "att", 0), (3, "att", 1), (3, "att", 2), (5, "att", 2), (5, "wgru", 1)])
def test_probe_on_threshold_states(native_lib, N, variant, mode):
    """The rays the step launch flags for the exact fix-up: the probe decides them itself and lands on the
    band fix's value; kind / id of the subject's rays (the threshold ray among them) follow the restatement;
    the handle's band list is not touched."""
    fam, var, st, occ = T.build(N, seed=N)
    E = len(fam)
    env = _env(E, N, occ, mode, variant)
    _install(env, st)
    env.step(torch.zeros(E, N, 2, device="cuda"))
    before = env.band_max()
    assert mode == 1 or before[0] > 0          # (the cell families flag too; the drone ones always)
    probe = _probe(env)
    probe.run()
    pr = probe.read()
    assert env.band_max() == before
    pos = _np(env.get_state()["pos"])
    _self_consistent(pr, pos, _np(env.bufs.radar), f"thresholds N{N} {variant} mode{mode}")
    checked = 0
    for e, f in enumerate(fam):
        if f not in T.RADAR_FAMILIES:
            continue
        for r in range(18):
            ref = R.probe_ray(pos[e], 0, r, occ, mode)
            assert (int(pr["kind"][e, 0, r]), int(pr["id"][e, 0, r])) == (ref["kind"], ref["id"]), (f, var[e], e, r, ref)
            assert abs(pr["dist"][e, 0, r] - ref["dist"]) <= TOL
            checked += 1
    assert checked > 100 * 18


# ------------------------------------------------------------------ 4: hand-built ties
def test_hand_built_ties(native_lib):
    occ = C.hand_map()
    env = _env(4, 2, occ, 2)
    probe = _probe(env)
    probe.at(C.HAND_ROWS)
    pr = probe.read()
    for (m, i, r), (kind, idx, dist, point) in C.HAND_WANT.items():
        got = (int(pr["kind"][m, i, r]), int(pr["id"][m, i, r]), float(pr["dist"][m, i, r]), tuple(pr["point"][m, i, r]))
        assert got == (kind, idx, dist, point), (m, i, r, got)
    assert tuple(pr["end"][2, 0, 0]) == (555.0, 310.0)            # d == len: the hit point is the ray end
    # every ray of the rows in full, nothing excused
    _against_ref(pr, C.HAND_ROWS, occ, 2, None, "hand-built", excuse=False)
    dx, dy = pr["point"][..., 0] - C.HAND_ROWS[:, :, None, 0], pr["point"][..., 1] - C.HAND_ROWS[:, :, None, 1]
    assert _same_bits(np.sqrt(dx * dx + dy * dy), pr["dist"])


# ------------------------------------------------------------------ 5: at() shapes, selection, arena
def _carve(ar, M, N):
    n = M * N * 18
    reg = {"dist": ar.take(M, N * 18), "point": ar.take(M, N * 36), "end": ar.take(M, N * 36),
           "kind": ar.take(1, (n + 7) // 8), "id": ar.take(1, (4 * n + 7) // 8)}
    out = {k: reg[k].view for k in ("dist", "point", "end")}
    out["kind"] = reg["kind"].view.view(torch.uint8).reshape(-1)[:n]
    out["id"] = reg["id"].view.view(torch.int32).reshape(-1)[:n]
    return reg, out


@pytest.mark.parametrize("M", [1, 65, 300])
def test_at_shapes_selection_and_arena(native_lib, occ, M):
    """M rows of 90 work items (N = 5), no multiple of a workgroup's 256, so workgroups start and end inside
    rows; alternating ``sel``: the unselected
    outputs keep the canary, the selected equal the unselected launch (M = 65: ``run()`` on the same
    positions as live state) bit for bit; nothing outside the payload changes."""
    N, E = 5, 65
    env = _env(E, N, occ, 2)
    probe = _probe(env)
    pos = C.random_rows(M, N, seed=50 + M)
    if M == E:
        z = np.zeros_like(pos)
        env.set_state(pos=pos, pre_pos=pos, vel=z, pre_vel=z, map_idx=np.zeros(E, np.int32))
        probe.run()
        full = probe.read()
    else:
        full = probe.read(probe.at(pos))
    assert full["dist"].shape == (M, N, 18) and full["point"].shape == (M, N, 18, 2)
    assert M == 1 or all((full["kind"] == k).any() for k in range(4))
    sel = (np.arange(M) % 2 == 0).astype(np.uint8)
    ar = Arena(6 * M * N * 18 + 1024, torch.float64, "cuda", max_ld=N * 36)
    reg, out = _carve(ar, M, N)
    snap = {k: _np(reg[k].view).copy() for k in reg}
    probe.at(pos, sel=sel, out=out)
    torch.cuda.synchronize()
    ar.check(writable=list(reg.values()), all_written=False)
    got = probe.read(out)
    on = sel.astype(bool)
    for k in FIELDS:
        assert _same_bits(got[k][on], full[k][on]), k
    n = M * N * 18
    after = {k: _np(reg[k].view) for k in reg}
    for k in ("dist", "point", "end"):
        assert _same_bits(after[k][~on], snap[k][~on]), k + ": an unselected row was written"
    for k, size in (("kind", 1), ("id", 4)):
        a, b = after[k].view(np.uint8).reshape(-1), snap[k].view(np.uint8).reshape(-1)
        assert np.array_equal(a[n * size:], b[n * size:]), k + ": bytes past the payload"
        keep = np.repeat(~on, N * 18 * size)
        assert np.array_equal(a[:n * size][keep], b[:n * size][keep]), k + ": an unselected row was written"
    # without ``end``: the other outputs do not change
    o2 = probe._alloc(M)
    P = probe._native.ProbeOut(o2["dist"].data_ptr(), o2["point"].data_ptr(), None, o2["kind"].data_ptr(), o2["id"].data_ptr())
    import ctypes
    pd = torch.as_tensor(pos, device="cuda")
    probe._native.check(probe._native.lib().aac_env_probe(env._h, ctypes.c_void_p(pd.data_ptr()), None, M, None,
                                                          ctypes.byref(P), None), "aac_env_probe")
    torch.cuda.synchronize()
    for k in ("dist", "point", "kind", "id"):
        assert _same_bits(_np(o2[k]), full[k]), k
    assert not _np(o2["end"]).any()


def test_probe_argument_errors(native_lib, occ):
    env = _env(4, 3, occ, 2)
    probe = _probe(env)
    with pytest.raises(ValueError):
        probe.at(np.zeros((2, 4, 2)))                     # another N
    with pytest.raises(ValueError):
        probe.run(sel=torch.zeros(5, dtype=torch.uint8, device="cuda"))
    import ctypes
    o = probe._live
    P = probe._native.ProbeOut(*[o[k].data_ptr() for k in FIELDS])
    L = probe._native.lib()
    assert L.aac_env_probe(env._h, None, None, 3, None, ctypes.byref(P), None) == -1      # live state: M must be E
    assert b"E rows" in L.aac_last_error()
    P.dist = None
    assert L.aac_env_probe(env._h, None, None, 4, None, ctypes.byref(P), None) == -1


# ------------------------------------------------------------------ 6 + 7: read-only, graph
def test_run_is_read_only_and_replays_in_a_graph(native_lib, occ):
    from multi_agent_aac_amd import graphs
    name = "combined5"
    mode, N, variant = C.CASES[name]
    st, wps, cnt, stack, mi = C.reset_state(occ, name)
    env = _env(C.E, N, stack, mode)
    env.reset(st, wps, cnt)
    env.step(torch.full((C.E, N, 2), 0.25, device="cuda"))
    probe = _probe(env)
    torch.cuda.synchronize()
    state0 = {k: _np(v).copy() for k, v in env.get_state().items()}
    bufs0 = {k: _np(v).copy() for k, v in vars(env.bufs).items() if v is not None}
    probe.run()
    eager = probe.read()
    for k, v in env.get_state().items():
        assert _same_bits(_np(v), state0[k]), k
    for k, v in vars(env.bufs).items():
        if v is not None:
            assert _same_bits(_np(v), bufs0[k]), k
    for t in probe._live.values():
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        probe.run()
    for t in probe._live.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    replay = probe.read()
    for k in FIELDS:
        assert _same_bits(replay[k], eager[k]), k
    assert (eager["kind"] != 0).any()


# ------------------------------------------------------------------ 8: trajectories
def test_for_trajectories(native_lib):
    from multi_agent_aac_amd import probe as P
    from multi_agent_aac_amd import trainer
    from multi_agent_aac_amd.evaluate import Evaluator
    tr = trainer.Trainer(16, 3, 16, 1024, "combined", seed=1, model="att")
    ev = Evaluator(tr, E=8, seed=0)
    stats, tj = ev.record(1)
    out = P.for_trajectories(ev.env, tj)
    T_, S = tj.rows["pos"].shape[:2]
    assert out["valid"].shape == (T_, S) and np.array_equal(out["valid"].sum(1), tj.cursor) and tj.cursor.min() > 1
    assert np.array_equal(out["valid"], np.arange(S)[None] < tj.cursor[:, None])
    assert out["dist"].shape == (T_, S, 3, 18) and out["point"].shape == (T_, S, 3, 18, 2)
    rows = [(k, r) for k in range(T_) for r in range(int(tj.cursor[k]))]
    pr = P.RadarProbe.for_env(ev.env)
    pos = np.stack([tj.rows["pos"][k, r] for k, r in rows])
    midx = np.array([tj.rows["header"][k, r, 3] for k, r in rows], np.int32)
    one = pr.read(pr.at(pos, map_idx=midx))
    for f in FIELDS:
        assert _same_bits(np.stack([out[f][k, r] for k, r in rows]), one[f]), f
        assert not out[f][~out["valid"]].any(), f + ": rows past the cursor are not written"
    assert (one["kind"] != 0).any()
