"""bench.py's ``--dump-outputs`` writer and the plain / ``--full`` switch, on the CPU: the writer
is given a stand-in trainer with host tensors (the files' names, dtypes and values, and the seeded
env sample when the rows pass the byte budget)."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _trainer(E=12, N=3):
    g = torch.Generator().manual_seed(5)
    cur = types.SimpleNamespace(own=torch.rand(E, N, 7, generator=g, dtype=torch.float64),
                                radar=torch.rand(E, N, 18, generator=g),
                                done=(torch.rand(E, N, generator=g) > 0.5).to(torch.uint8),
                                env_done=(torch.rand(E, generator=g) > 0.5).to(torch.uint8),
                                conf=torch.arange(E * N, dtype=torch.int32).view(E, N), nei6=None)
    torch.manual_seed(6)
    model = types.SimpleNamespace(actors=torch.nn.Linear(7, 4), critics=torch.nn.Linear(5, 3).double(),
                                  actors_target=torch.nn.Linear(7, 4), critics_target=torch.nn.Linear(5, 3).double())
    return types.SimpleNamespace(E=E, N=N, cur=cur, model=model)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_buffer_as_float(tmp_path):
    tr = _trainer()
    bench.dump_outputs(tr, str(tmp_path / "out"))
    got = _load(str(tmp_path / "out"))
    f64 = ("env_own", "learner_critics", "learner_critics_target")
    assert sorted(got) == ["env_conf", "env_done", "env_env_done", "env_own", "env_radar", "learner_actors",
                           "learner_actors_target", "learner_critics", "learner_critics_target"]
    assert all(got[k].dtype == (np.float64 if k in f64 else np.float32) for k in got)
    for k, t in vars(tr.cur).items():
        if t is not None:
            assert got["env_" + k].shape == tuple(t.shape) and np.array_equal(got["env_" + k], t.numpy())
    for n in ("actors", "critics", "actors_target", "critics_target"):
        net = getattr(tr.model, n)
        want = np.concatenate([net.weight.detach().numpy().ravel(), net.bias.detach().numpy().ravel()])
        assert np.array_equal(got["learner_" + n], want)


def test_dump_samples_envs_within_the_budget(tmp_path, monkeypatch):
    tr = _trainer(E=64)
    per_env = 3 * (7 * 8 + 18 * 4 + 4 + 4) + 4
    learner = 2 * (7 * 4 + 4) * 4 + 2 * (5 * 3 + 3) * 8
    monkeypatch.setattr(bench, "DUMP_BUDGET", learner + 10 * per_env + per_env // 2)
    bench.dump_outputs(tr, str(tmp_path / "a"))
    bench.dump_outputs(tr, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET
    assert all(a[k].shape[0] == 10 for k in a if k.startswith("env_"))
    assert all(np.array_equal(a[k], b[k]) for k in a)                  # the same sample every run
    # the sampled rows are whole envs of the full buffers, in ascending env order, the same for every field
    conf = tr.cur.conf.numpy()
    rows = [int(np.flatnonzero((conf == r).all(axis=1))[0]) for r in a["env_conf"]]
    assert rows == sorted(set(rows))
    assert np.array_equal(a["env_own"], tr.cur.own.numpy()[rows])
    assert np.array_equal(a["env_env_done"], tr.cur.env_done.numpy()[rows])


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (4, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
