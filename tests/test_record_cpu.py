"""Flight recorder without a GPU: ``Trajectories`` (pure numpy) on arrays produced by the numpy
restatement (tests/record_ref.py), the recorder kernel's compile-time resources, and the ctypes
structs against the header's sizes."""
import ctypes
import os
import re
import shutil

import numpy as np
import pytest

import record_ref
from test_stats_resources_cpu import HIPCC, _usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _synthetic(S, seed=3, E=6, N=4, steps=11, heading=False):
    """A RecordRef driven with random states: env e finishes an episode every 3 + e % 3 steps."""
    rng = np.random.default_rng(seed)
    ids = [4, 0, 5]
    ref = record_ref.RecordRef(ids, S, 3, N, return_mode=0, max_episodes=3, heading=heading, clouds=heading)
    episode = np.zeros(E, dtype=np.int32)

    def state():
        s = {"pos": rng.normal(size=(E, N, 2)) * 10, "vel": rng.normal(size=(E, N, 2)),
             "goal": rng.normal(size=(E, N, 2)), "episode": episode.copy(), "map_idx": np.arange(E, dtype=np.int32) % 2}
        if heading:
            s["heading"], s["clouds"] = rng.normal(size=(E, N)), rng.normal(size=(E, 2, 2))
        return s
    ref.reset_phase(state())
    age = np.zeros(E, dtype=np.int32)
    for _ in range(steps):
        age += 1
        s = state()
        s["act"] = rng.uniform(-1, 1, size=(E, N, 2)).astype(np.float32)
        s["reward"] = rng.normal(size=(E, N)).astype(np.float32)
        s["env_done"] = (age >= 3 + np.arange(E) % 3).astype(np.uint8)
        s["done"] = (rng.random((E, N)) < 0.2).astype(np.uint8) * s["env_done"][:, None]
        s["mask"] = rng.integers(0, 64, size=(E, N)).astype(np.uint8)
        ref.step_phase(s)
        episode += s["env_done"]
        age[s["env_done"] != 0] = 0
        ref.reset_phase(dict(state(), episode=episode.copy()), sel=s["env_done"])
    return ref


def test_episode_slicing_and_min_separation():
    ref = _synthetic(S=64)
    tj = ref.trajectories()
    assert list(tj.tracks) == [4, 0, 5] and not tj.dropped.any()
    eps = tj.episodes()
    # env 4 ends every 4 steps, env 0 every 3, env 5 every 5: 2, 3 and 2 episodes in 11 steps
    assert [(e["track"], e["env"]) for e in eps] == [(0, 4)] * 2 + [(1, 0)] * 3 + [(2, 5)] * 2
    assert [e["len"] for e in eps] == [4, 4, 3, 3, 3, 5, 5]
    assert [e["episode"] for e in eps] == [0, 1, 0, 1, 2, 0, 1]
    for e in eps:
        assert not e["truncated"] and e["rows"] == e["len"] + 1
        assert list(e["t"]) == list(range(e["len"] + 1))
        assert e["row_flags"][0] == 2 and e["row_flags"][-1] == 1 and not e["row_flags"][1:-1].any()
        assert e["pos"].shape == (e["rows"], 4, 2) and e["act"].dtype == np.float32
        assert not e["act"][0].any() and not e["reward"][0].any()
        # the summary restates its rows: closest approach, the first step that attains it, the return
        k, r0 = e["track"], e["row0"]
        seps = tj.rows["min_sep"][k, r0:r0 + e["rows"]]
        assert np.array_equal(e["min_sep_row"], seps)
        assert e["min_sep"] == seps.min() and e["min_sep_t"] == int(np.argmin(seps))
        assert np.array_equal(e["nearest"].min(axis=1), seps)
        ret = np.float64(0)
        for row in e["reward"][1:]:
            for v in row:
                ret = ret + v
        assert e["ret"] == ret
    assert [e["track"] for e in tj.episodes(track=1)] == [1, 1, 1]
    ms = tj.min_separation()
    assert ms.dtype == np.float64 and ms.shape == (7,)
    assert np.array_equal(ms, [tj.summaries[e["track"]]["min_sep"][i] for e, i in zip(eps, [0, 1, 0, 1, 2, 0, 1])])


def test_truncated_episodes_keep_their_summaries():
    full, cut = _synthetic(S=64).trajectories(), _synthetic(S=6).trajectories()
    assert list(cut.cursor) == [6, 6, 6]
    assert list(cut.dropped) == [c - 6 for c in full.cursor]
    for a, b in zip(full.episodes(), cut.episodes()):
        for f in ("ret", "min_sep", "min_sep_t", "len", "episode", "env", "any_done"):
            assert a[f] == b[f], f
        assert b["row0"] == min(6, a["row0"])
        assert b["truncated"] == (a["row0"] + a["rows"] > 6)
        assert b["rows"] == max(0, min(6, a["row0"] + a["rows"]) - min(6, a["row0"]))
        assert len(b["pos"]) == b["rows"]
        assert np.array_equal(b["pos"], a["pos"][:b["rows"]])


@pytest.mark.parametrize("heading", [False, True])
def test_npz_round_trip(tmp_path, heading):
    tj = _synthetic(S=16, heading=heading).trajectories()
    path = str(tmp_path / "traj.npz")
    tj.save(path)
    back = type(tj).load(path)
    assert back == tj
    assert set(back.rows) == set(tj.rows) and ("heading" in back.rows) == heading
    for k in tj.rows:
        assert record_ref.same_bits(back.rows[k], tj.rows[k]), k
    for f in tj.summaries.dtype.names:
        assert record_ref.same_bits(back.summaries[f], tj.summaries[f]), f
    for f in ("tracks", "cursor", "ep_seen", "dropped"):
        assert record_ref.same_bits(getattr(back, f), getattr(tj, f)), f
    other = _synthetic(S=16, heading=heading, seed=4).trajectories()
    assert other != tj


def test_separation_ties_and_single_agent():
    # agent 0 at the origin, three agents on 3-4-5 triangles around it, one coincident pair
    pos = np.array([[0, 0], [3, 4], [-4, 3], [0, -5], [100, 100], [100, 100]], dtype=np.float64)
    near, idx, sep = record_ref.separation(pos)
    assert list(idx) == [1, 0, 0, 0, 5, 4] and list(near) == [5, 5, 5, 5, 0, 0] and sep == 0
    near, idx, sep = record_ref.separation(np.zeros((1, 2)))
    assert np.isinf(near[0]) and idx[0] == -1 and np.isinf(sep)


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_record_kernels_have_no_scratch():
    ks = _usage("aac_record.hip")
    assert any("record_kernel" in k for k in ks), sorted(ks)
    for name, u in ks.items():
        assert "ScratchSize" in u, (name, u)
        assert u["ScratchSize"] == 0, (name, u)


def test_struct_sizes_match_the_header():
    """The .hip static_asserts sizeof(struct) == the header's constants; the binding must agree."""
    from multi_agent_aac_amd import _native, record
    src = open(os.path.join(ROOT, "include", "aac_record.h")).read()
    const = {k: int(v) for k, v in re.findall(r"#define (AAC_RECORD_\w+) (\d+)", src)}
    assert ctypes.sizeof(_native.RecordEpisode) == const["AAC_RECORD_EPISODE_BYTES"] == record.EPISODE.itemsize
    assert ctypes.sizeof(_native.RecordState) == const["AAC_RECORD_STATE_BYTES"]
    assert ctypes.sizeof(_native.RecordStep) == const["AAC_RECORD_STEP_BYTES"]
    hip = open(os.path.join(ROOT, "multi_agent_aac_amd", "csrc", "aac_record.hip")).read()
    for name, typ in (("EPISODE", "episode"), ("STATE", "state"), ("STEP", "step")):
        assert re.search(r"static_assert\(sizeof\(aac_record_%s\) == AAC_RECORD_%s_BYTES" % (typ, name), hip), name
    assert (const["AAC_RECORD_RESET"], const["AAC_RECORD_STEP"]) == (record.PHASE_RESET, record.PHASE_STEP)
    assert const["AAC_RECORD_MAX_AGENTS"] == record.MAX_AGENTS
    assert [f for f, _ in _native.RecordEpisode._fields_] == list(record.EPISODE.names)
