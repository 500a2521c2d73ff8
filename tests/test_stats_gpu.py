"""Episode statistics kernel (include/aac_stats.h) against the numpy restatement (tests/stats_ref.py)
on synthetic step outputs: totals, running state and log rows; quota; run-to-run and eager-to-graph
bit-identity.

Shapes: E = 5 (one partial workgroup), EPW + 7 (a full and a partial one), 3 EPW + 1 (a one-env
workgroup), N = 2 (agent 0's reward) and 5 (sum over agents) in float32, and one float64 case with
N = 33 (three LDS passes of 16 + 16 + 1 agents, reach bits past 32).  40 steps, episode_length 6, so
that every end reason, crash subtype and reach bin 0 / 1 / N occurs (asserted on the restatement).
The log holds 64 rows: at the larger E one step finishes more episodes than that."""
import functools
import types

import numpy as np
import pytest
import torch

import stats_ref

EPW = 256
T, EP_LEN, LOG = 40, 6, 64
#        E            N   f64    seed
CASES = {"e5_n2": (5, 2, False, 0), "e5_n5": (5, 5, False, 2),
         "e263_n2": (EPW + 7, 2, False, 0), "e263_n5": (EPW + 7, 5, False, 0),
         "e769_n2": (3 * EPW + 1, 2, False, 0), "e769_n5": (3 * EPW + 1, 5, False, 0),
         "e263_n33_f64": (EPW + 7, 33, True, 0)}


def gen_inputs(E, N, f64, seed):
    """Seeded random step outputs [T][...]: an env ends with probability 1/4 per step (lengths on both
    sides of episode_length 6); per (step, env) no agent, one agent or all agents take the goal
    branch; done and bbc flags are independent coin flips."""
    rng = np.random.default_rng([seed, E, N])
    reward = rng.normal(0.0, 3.0, size=(T, E, N)).astype(np.float64 if f64 else np.float32)
    done = (rng.random((T, E, N)) < 0.2).astype(np.uint8)
    env_done = (rng.random((T, E)) < 0.25).astype(np.uint8)
    bbc = (rng.random((T, E, 4)) < 0.4).astype(np.uint8)
    goal_bit = 4 if f64 else 5
    mask = rng.integers(0, 256, size=(T, E, N)).astype(np.uint8) & np.uint8(~(1 << goal_bit) & 0xFF)
    mode = rng.choice(3, size=(T, E), p=[0.6, 0.25, 0.15])
    who = rng.integers(0, N, size=(T, E))
    goal = (mode[..., None] == 2) | ((mode[..., None] == 1) & (np.arange(N) == who[..., None]))
    mask |= (goal.astype(np.uint8) << goal_bit).astype(np.uint8)
    return dict(reward=reward, done=done, mask=mask, env_done=env_done, bbc=bbc)


def params(name):
    E, N, f64, seed = CASES[name]
    return dict(E=E, N=N, f64=f64, seed=seed, goal_bit=4 if f64 else 5, return_mode=1 if N == 2 else 0)


@functools.lru_cache(maxsize=None)
def reference(name, quota=None, extra=0):
    """(inputs, restatement after T steps [+ ``extra`` repeated ones]); computed once per case."""
    p = params(name)
    x = gen_inputs(p["E"], p["N"], p["f64"], p["seed"])
    ref = stats_ref.StatsRef(p["E"], p["N"], EP_LEN, p["goal_bit"], p["return_mode"], log=LOG)
    q = None if quota is None else np.full(p["E"], quota, dtype=np.int32)
    for t in list(range(T)) + list(range(extra)):
        ref.accumulate(x["reward"][t], x["done"][t], x["mask"][t], x["env_done"][t], x["bbc"][t], quota=q)
    return x, ref


def covered(ref, N):
    c = ref.c
    return all(c[k] > 0 for k in ("timeout", "crash", "goal", "collision_count", "crash_bound", "crash_building",
                                  "crash_drone", "crash_nearest", "all_steps_used")) and \
        all(ref.reach_hist[k] > 0 for k in (0, 1, N))


def make_stats(name, log=LOG):
    from multi_agent_aac_amd.stats import EpisodeStats
    p = params(name)
    return EpisodeStats(p["E"], p["N"], EP_LEN, torch.float64 if p["f64"] else torch.float32, goal_bit=p["goal_bit"],
                        return_mode=p["return_mode"], log=log)


def upload(x):
    """Per-step buffer sets (views of one [T][...] device tensor per field)."""
    dev = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    return [types.SimpleNamespace(**{k: v[t] for k, v in dev.items()}) for t in range(T)]


def raw_state(st):
    """Everything the kernels wrote, as bytes-comparable arrays."""
    d = {k: v.cpu().numpy() for k, v in st.tensors().items()}
    d["totals"] = st._reduce().copy()
    return d


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_totals_state_log(native_lib, name):
    x, ref = reference(name)
    assert covered(ref, params(name)["N"]), (ref.c, ref.reach_hist)
    st = make_stats(name)
    steps = upload(x)
    for b in steps:
        st.accumulate(b)
    got = st.read()
    stats_ref.check_totals(got, ref)
    assert got["under_quota"] == params(name)["E"]
    stats_ref.check_state(st, ref)
    stats_ref.check_log(st, ref)
    assert got["return_mean"] == got["return_sum"] / got["episodes"]
    assert got["length_mean"] == got["steps"] / got["episodes"]
    first = raw_state(st)
    # a second run of the same sequence: bit-identical
    st.reset()
    for b in steps:
        st.accumulate(b)
    second = raw_state(st)
    for k in first:
        assert np.array_equal(first[k], second[k]), k
    # the 40 launches captured in one graph and replayed: bit-identical
    st.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for b in steps:
            st.accumulate(b)
    st.reset()
    g.replay()
    third = raw_state(st)
    for k in first:
        assert np.array_equal(first[k], third[k]), k


@pytest.mark.parametrize("name", ["e5_n5", "e769_n2", "e263_n33_f64"])
def test_quota(native_lib, name):
    E = params(name)["E"]
    x, ref = reference(name, quota=2)
    assert ref.c["episodes"] == 2 * E          # every env finishes two episodes within the 40 steps
    st = make_stats(name)
    steps = upload(x)
    quota = torch.full((E,), 2, dtype=torch.int32, device="cuda")
    for b in steps:
        st.accumulate(b, quota=quota)
    got = st.read()
    assert got["episodes"] == 2 * E and got["under_quota"] == 0 and st.under_quota() == 0
    stats_ref.check_totals(got, ref)
    stats_ref.check_state(st, ref)
    stats_ref.check_log(st, ref)
    before = raw_state(st)
    for b in steps[:8]:                        # further steps change nothing
        st.accumulate(b, quota=quota)
    after = raw_state(st)
    for k in before:
        if k != "log_meta":                    # its call counter goes on
            assert np.array_equal(before[k], after[k]), k
    assert int(after["log_meta"][0]) == int(before["log_meta"][0])


def test_clear_and_window(native_lib):
    """read(clear=True) empties the totals and keeps running episodes: two windows add up."""
    name = "e263_n5"
    x, ref = reference(name)
    st = make_stats(name)
    steps = upload(x)
    for b in steps[:17]:
        st.accumulate(b)
    a = st.read(clear=True)
    assert st.read()["episodes"] == 0
    for b in steps[17:]:
        st.accumulate(b)
    b2 = st.read()
    for k in stats_ref.COUNTERS:
        assert a[k] + b2[k] == ref.c[k], k
    assert [p + q for p, q in zip(a["reach_hist"], b2["reach_hist"])] == ref.reach_hist
    assert min(a["return_min"], b2["return_min"]) == min(ref.returns)
    stats_ref.check_state(st, ref)


def test_bad_arguments(native_lib):
    from multi_agent_aac_amd.stats import EpisodeStats
    with pytest.raises(ValueError):
        EpisodeStats(4, 65, 10)
    st = EpisodeStats(4, 2, 10)
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device="cuda")   # noqa: E731
    bad = types.SimpleNamespace(reward=z(4, 3, dt=torch.float32), done=z(4, 2), mask=z(4, 2), env_done=z(4), bbc=z(4, 4))
    with pytest.raises(ValueError):
        st.accumulate(bad)
