"""The C oracle over every agent count the env ABI accepts (2..256).

oc_step used to keep its per-agent arrays at 64 entries: N = 65 wrote past them silently and N = 85
smashed the stack.  They are sized by N now, so: the stand-alone driver (oracle/wide_driver.c, N = 65
and 256 under ASan / UBSan) exits clean, the N = 64 outputs are bit-identical to the ones recorded from
the oracle before the change (tests/golden/oracle_n64.npz: inputs and the oracle's own outputs), and
BatchedOracle refuses N outside 2..256.

``python -m tests.test_oracle_wide_cpu OUT.npz`` re-records the fixture from whatever oracle is built.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import c_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "oracle_n64.npz")
N, E, W, STEPS = 64, 1, 32, 3
PER_STEP = ("radar", "reward", "done", "mask", "env_done", "bbc", "pos", "vel", "wp_cur", "reach", "wall")
LAST = ("own", "nei", "conf_cur", "tcpa")


def _inputs(occ):
    """Starts on free ground near each other (the penalty, contact and radar loops all do work)."""
    from tests.helpers import random_od
    rng = np.random.default_rng(64)
    inp = {}
    for v in ("att", "wgru"):
        st, wps, cnt = random_od(occ, E, N, seed=640 + len(v), W=W)
        inp[v + "_st"], inp[v + "_wps"], inp[v + "_cnt"] = st, wps, cnt
        inp[v + "_act"] = rng.uniform(-1, 1, size=(STEPS, E, N, 2)).astype(np.float32)
        inp[v + "_crowd"] = np.array([560.0, 322.0]) + rng.normal(scale=9.0, size=(E, N, 2))
    return inp


def _trace(occ, inp):
    """Reset, one random step, a crowded injected state stepped with zero actions, one more step."""
    out = {}
    for v in ("att", "wgru"):
        co = c_oracle.BatchedOracle(E, N, occ, W=W, radar_mode=2, with_tdcpa=True, team_reward=True, variant=v)
        co.reset(inp[v + "_st"], inp[v + "_wps"], inp[v + "_cnt"])
        out[f"{v}_reset_radar"] = co.radar.copy()
        out[f"{v}_reset_own"] = co.own.copy()
        for t in range(STEPS):
            act = inp[v + "_act"][t]
            if t == 1:
                co.pos[:] = inp[v + "_crowd"]
                co.pre_pos[:] = inp[v + "_crowd"]
                co.vel[:] = 0
                co.pre_vel[:] = 0
                act = np.zeros_like(act)
            co.step(act)
            for name in PER_STEP + (LAST if t == STEPS - 1 else ()):
                a = co.step_count if name == "step" else getattr(co, name)
                out[f"{v}_t{t}_{name}"] = a.copy()
    return out


@pytest.mark.skipif(not shutil.which("gcc") or not shutil.which("make"), reason="no host toolchain")
def test_wide_driver_is_asan_ubsan_clean():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "wide"], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "oracle", "_build", "wide_driver")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "wide oracle run ok" in r.stdout


def test_n64_outputs_unchanged_bit_for_bit(occ):
    gold = np.load(GOLD)
    inp = {k: gold[k] for k in gold.files if k.split("_")[1] in ("st", "wps", "cnt", "act", "crowd")}
    got = _trace(occ, inp)
    want = sorted(k for k in gold.files if k not in inp)
    assert want == sorted(got) and len(want) > 60
    for k in want:
        assert got[k].dtype == gold[k].dtype and got[k].tobytes() == gold[k].tobytes(), k
    # the recorded trace is not a quiet one: contacts, penalties and radar returns all occur
    assert (gold["att_t1_mask"] & 2).any() and (gold["att_t1_radar"] < 15).any()
    assert (gold["wgru_t1_mask"] & 2).any() and len(np.unique(gold["wgru_t1_reward"])) > 8


@pytest.mark.parametrize("n", [1, 257, 300])
@pytest.mark.parametrize("variant", ["att", "wgru"])
def test_agent_count_outside_abi_range_refused(occ, n, variant):
    with pytest.raises(ValueError, match="outside 2..256"):
        c_oracle.BatchedOracle(2, n, occ, variant=variant)


@pytest.mark.parametrize("n", [2, 65, 85, 256])
def test_wide_counts_step(occ, n):
    """Through ctypes too: the counts that used to overrun step and give finite, in-range outputs."""
    from tests.helpers import W_DEFAULT
    rng = np.random.default_rng(n)
    co = c_oracle.BatchedOracle(1, n, occ, W=W_DEFAULT, radar_mode=2)
    st = np.array([470.0, 262.0]) + 6.0 * np.stack([np.arange(n) % 16, np.arange(n) // 16], -1)[None].astype(float)
    wps = np.repeat((st + 30.0)[:, :, None, :], W_DEFAULT, 2)
    co.reset(st, wps, np.full((1, n), 1, np.int32))
    for _ in range(2):
        co.step(rng.uniform(-1, 1, size=(1, n, 2)).astype(np.float32))
    assert np.isfinite(co.reward).all() and np.isfinite(co.own).all()
    assert (co.radar >= 0).all() and (co.radar <= 15).all() and (co.radar < 15).any()
    assert len(np.unique(co.reward)) == 1          # team reward: one sum over all n agents


if __name__ == "__main__":
    from multi_agent_aac_amd import world
    occ_ = world.synthetic_map(2026)
    inp_ = _inputs(occ_)
    np.savez_compressed(sys.argv[1], **inp_, **_trace(occ_, inp_))
    print("recorded", sys.argv[1], os.path.getsize(sys.argv[1]), "bytes")
