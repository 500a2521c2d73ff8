"""The flight recorder behind the three real envs (aac_env_record / aac_uam_record through
``FlightRecorder``): E = 32, seeded random actions, episode_length 6, 20 steps of step / record /
auto-reset / record.  An episode lasts at most episode_length + 1 = 7 steps, so every track finishes
at least 2 episodes in 20 steps by construction.

After every eager call the whole recording is downloaded and compared with the numpy restatement
(tests/record_ref.py) fed from ``get_state()`` and the step buffers: the terminal rows are checked
before the reset overwrites the state, the t = 0 rows after it.  The att run leaves the episode
counter inside the handle (the expected count is kept here: one per reset of the env); the others
move it to a caller's buffer with ``use_episode_buffer``."""
import numpy as np
import pytest
import torch

import record_ref
from test_stats_env_gpu import _make_env

pytestmark = pytest.mark.gpu

E, EP, STEPS = 32, 6, 20
SUBSET = [31, 4, 0, 17, 9, 22, 30]
#        kind  N   env_ids  episodes  action seed
RUNS = [("att", 5, None, 2, 1),("wgru", 8, SUBSET, 2, 2), ("uam", 5, SUBSET, 2, 3), ("uam", 16, None, 2, 4)]


def _np(d, keys):
    return {k: d[k].cpu().numpy() for k in keys}


def _download(rec):
    return {"rows": _np(rec.rows, rec.rows), "track": _np(rec.track, rec.track),
            "summaries": rec.summaries.cpu().numpy().view(record_ref.EPISODE)[..., 0]}


@pytest.mark.parametrize("kind,N,ids,episodes,seed", RUNS)
def test_recording_follows_the_env(native_lib, occ, kind, N, ids, episodes, seed):
    from multi_agent_aac_amd.record import FlightRecorder
    uam = kind == "uam"
    env = _make_env(kind, E, N, EP, occ)
    S = episodes * (EP + 2)
    rec = FlightRecorder.for_env(env, ids, steps=S, episodes=episodes)
    assert (rec.T, rec.S, rec.P) == (E if ids is None else len(ids), S, episodes)
    assert rec.return_mode == {"att": 1, "wgru": 0, "uam": 0}[kind]
    ref = record_ref.RecordRef(np.arange(E) if ids is None else ids, S, episodes, N, rec.return_mode, episodes,
                               heading=uam, clouds=uam)
    counter = None
    if kind != "att":
        counter = env.use_episode_buffer(torch.zeros(E, dtype=torch.int32, device="cuda"))
    host_count = np.zeros(E, dtype=np.int32)
    keys = ("pos", "vel", "goal") + (("heading", "clouds") if uam else ("map_idx",))

    def state():
        s = _np(env.get_state(), keys)
        s["episode"] = counter.cpu().numpy() if counter is not None else host_count.copy()
        if counter is not None:
            assert np.array_equal(s["episode"], host_count)
        return s
    bufs = [env.alloc_buffers(), env.alloc_buffers()]
    env.auto_reset(None, out=bufs[0])
    host_count += 1
    rec.after_reset(None)
    ref.reset_phase(state())
    worst = record_ref.check(_download(rec), ref, "first reset")
    g = torch.Generator(device="cuda").manual_seed(seed)
    adt = torch.float64 if uam else torch.float32
    # even envs: full-scale random accelerations (crashes); odd envs: 2 % of them (the step limit)
    scale = torch.where(torch.arange(E, device="cuda") % 2 == 0, 1.0, 0.02).to(adt).view(E, 1, 1)
    for t in range(STEPS):
        n = bufs[1 - (t & 1)]
        act = (torch.rand(E, N, 2, device="cuda", generator=g, dtype=adt) * 2 - 1) * scale
        env.step(act, out=n)
        rec.after_step(n, act)
        s = state()
        s.update(_np({k: getattr(n, k) for k in ("reward", "done", "mask", "env_done")},
                     ("reward", "done", "mask", "env_done")), act=act.cpu().numpy())
        ref.step_phase(s)
        worst = max(worst, record_ref.check(_download(rec), ref, ("step", t)))
        env.auto_reset(n.env_done, out=n)
        host_count += s["env_done"] != 0
        rec.after_reset(n.env_done)
        ref.reset_phase(state(), sel=s["env_done"])
        worst = max(worst, record_ref.check(_download(rec), ref, ("reset", t)))
    tj = rec.read()
    print(kind, N, "worst ulp", worst, "episodes", int(tj.ep_seen.sum()), "min separation", tj.min_separation().min())
    assert (tj.ep_seen == episodes).all() and not tj.dropped.any()
    assert tj == ref.trajectories() or worst == 1
    eps = tj.episodes()
    assert len(eps) == rec.T * episodes
    for e in eps:
        assert e["rows"] == e["len"] + 1 <= EP + 2 and not e["truncated"]
        assert e["row_flags"][0] == 2 and e["row_flags"][-1] == 1 and not e["row_flags"][1:-1].any()
        assert list(e["t"]) == list(range(e["rows"])) and e["env"] == tj.tracks[e["track"]]
        assert (e["map_idx"] == 0).all()
    print("episode lengths", sorted({e["len"] for e in eps}))
