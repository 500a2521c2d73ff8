"""One plain ``bench.py`` run at a tiny size on the GPU: the result line of a plain run (the headline
fields, none of the ``--full`` measurements), ``--steps`` as the number of timed steps, and the
``--dump-outputs`` files of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, N, B, STEPS = 64, 3, 64, 6


@pytest.mark.gpu
def test_plain_run_line_and_dump(native_lib, tmp_path):
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "2", "--envs", str(E), "--agents", str(N), "--batch", str(B), "--memory", "4096",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == 2 and d["unit"] == "agent-env-steps/s" and d["higher_is_better"]
    assert d["ms_per_step"] > 0 and d["dtype"] == "f64 env state / f32 obs+learner"
    # value and ms_per_step are the same measurement: E x N agent-env-steps per timed step
    assert abs(d["value"] - E * N / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    for k in ("cpu_baseline", "roofline", "env_roofline", "attn_roofline", "env_microbench", "world_schedule"):
        assert k not in d, k
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    D0 = 6 + 4 * (N - 1)
    shapes = {"env_own": (E, N, D0), "env_radar": (E, N, 18), "env_nei": (E, N, N - 1, 6), "env_reward": (E, N),
              "env_done": (E, N), "env_mask": (E, N), "env_env_done": (E,), "env_bbc": (E, 4)}
    for k, s in shapes.items():
        assert got[k].shape == s and got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
    nets = ("learner_actors", "learner_critics", "learner_actors_target", "learner_critics_target")
    assert sorted(got) == sorted(list(shapes) + list(nets))
    for a, t in (nets[0::2], nets[1::2]):
        assert got[a].shape == got[t].shape and got[a].ndim == 1 and np.isfinite(got[a]).all()
        # the updates moved the online network, and the Polyak target (tau = 0.01) lags behind it
        assert 0 < np.abs(got[a] - got[t]).max() < 1.0
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
