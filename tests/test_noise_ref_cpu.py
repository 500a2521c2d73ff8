"""The checker behind the act-path noise tests, pinned without a GPU: tests/noise_ref.py against a
scalar restatement on Python integers and ``math``, and the block arithmetic of
tests/test_act_rows_gpu.py (which rows of a weights-stationary launch take the inline noise)."""
import math

import numpy as np
import pytest

from tests import noise_ref


def test_mix64_matches_scalar_integers():
    xs = [0, 1, 2, 0x9E3779B97F4A7C15, (1 << 64) - 1, (1 << 63), 123456789012345678]
    got = noise_ref.mix64(np.array(xs, dtype=np.uint64))
    assert [int(v) for v in got] == [noise_ref.mix64_int(x) for x in xs]
    # SplitMix64's first output for state 0 (the published test vector of the generator)
    assert noise_ref.mix64_int(0) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("N", [1, 5, 8])
def test_row_to_episode_mapping_matches_scalar_loop(N):
    E = 37
    rng = np.random.default_rng(N)
    episode = rng.integers(1, 9000, size=E).astype(np.int32)
    rows = np.arange(E * N)
    got = noise_ref.row_episode(rows, N, episode)
    for r in rows:
        assert got[r] == float(episode[r // N]), r
    assert (noise_ref.row_episode(rows, N, None) == 1.0).all()
    # a sub-list of rows (the sampled form) maps the same way
    sub = rows[::7].astype(np.uint64)
    assert np.array_equal(noise_ref.row_episode(sub, N, episode), got[::7])


def _scalar_noise(seed, epoch, row, N, episode, eps_end, ns, ne):
    ep = int(episode[row // N]) if episode is not None else 1
    var = ns + (ne - ns) / (eps_end - 1) * (ep - 1) if ep <= eps_end else ne
    h1 = noise_ref.mix64_int(noise_ref.mix64_int(noise_ref.mix64_int(seed) ^ epoch) ^ (2 * row))
    h2 = noise_ref.mix64_int(h1 ^ 0xD1B54A32D192ED03)
    u1 = (float(h1 >> 11) + 1.0) * (1.0 / 9007199254740992.0)
    u2 = float(h2 >> 11) * (1.0 / 9007199254740992.0)
    rr = math.sqrt(-2.0 * math.log(u1))
    return rr * math.cos(noise_ref.TWO_PI * u2) * var, rr * math.sin(noise_ref.TWO_PI * u2) * var


@pytest.mark.parametrize("N", [1, 5, 8])
def test_noise_matches_scalar_restatement(N):
    E, eps_end, seed = 23, 8000, 7919 * 6 + 3
    rng = np.random.default_rng(N + 10)
    episode = rng.integers(1, 9000, size=E).astype(np.int32)
    episode[0], episode[1], episode[2] = 1, eps_end, eps_end + 1       # both ends of the schedule and past it
    rows = np.arange(E * N)
    for epoch in (0, 41, (1 << 32) - 1):
        got = noise_ref.noise64(seed, epoch, rows, N, episode, eps_end, 1.0, 0.03)
        for r in rows:
            w0, w1 = _scalar_noise(seed, epoch, int(r), N, episode, eps_end, 1.0, 0.03)
            # numpy's and math's log / cos / sin may differ in the last place
            assert abs(got[r, 0] - w0) <= 1e-15 * max(1.0, abs(w0)) and abs(got[r, 1] - w1) <= 1e-15 * max(1.0, abs(w1))
    assert not np.array_equal(noise_ref.noise64(seed, 0, rows, N, episode, eps_end, 1.0, 0.03),
                              noise_ref.noise64(seed, 1, rows, N, episode, eps_end, 1.0, 0.03))


def test_schedule_ends_and_float32_form():
    ep = np.array([1, 2, 7999, 8000, 8001, 20000])
    v = noise_ref.var_schedule(ep, 8000, 1.0, 0.05)
    assert v[0] == 1.0 and abs(v[3] - 0.05) < 1e-15 and v[4] == 0.05 and v[5] == 0.05 and v[1] < 1.0
    # noise32: the schedule ends are the float32 values the launch receives, one rounding at the end
    rows = np.arange(40)
    ns, ne = float(np.float32(1.0)), float(np.float32(0.05))
    want = noise_ref.noise64(3, 2, rows, 5, None, 8000, ns, ne).astype(np.float32)
    got = noise_ref.noise32(3, 2, rows, 5, None, 8000, 1.0, 0.05)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert ne != 0.05                                                   # the distinction is real


def test_block_arithmetic_of_the_act_rows_cases():
    """The (inline-noise rows, largest block index, workgroups reaching it, partial last block)
    tables of test_act_rows_gpu.py follow from the launchers' grid formulas; a scalar walk of the
    kernels' loop (workgroup wg runs blocks wg, wg + grid, ...) counts the same rows."""
    from tests import test_act_rows_gpu as T

    def walk(rows, rpb, grid):
        nblk = (rows + rpb - 1) // rpb
        fb, max_kb, at_max = 0, 0, 0
        for wg in range(grid):
            kb = 0
            for blk in range(wg, nblk, grid):
                n = min(rpb, rows - blk * rpb)
                assert n > 0
                if kb >= T.NB:
                    fb += n
                if kb > max_kb:
                    max_kb, at_max = kb, 0
                if kb == max_kb:
                    at_max += 1
                kb += 1
        return fb, max_kb, at_max, rows % rpb != 0

    for (R, N), want in T.HEAD_CASES.items():
        grid = min((R + 15) // 16, 256)
        p = T.paths(R, 16, grid)
        assert walk(R, 16, grid) == want == (p["fallback_rows"], p["max_kb"], p["wgs_at_max"], p["partial"]), (R, N)
    for (E, N), want in T.GRU_CASES.items():
        G = max(1, min((E + 31) // 32, 256 // N))
        p = T.paths(E, 32, G)
        assert walk(E, 32, G) == want == (p["fallback_rows"], p["max_kb"], p["wgs_at_max"], p["partial"]), (E, N)
    for (R, N), want in T.UAM_CASES.items():
        p = T.paths(R, 16, 256)
        assert walk(R, 16, 256) == want == (p["fallback_rows"], p["max_kb"], p["wgs_at_max"], p["partial"]), (R, N)
    # every boolean in both directions within each kernel's set of cases
    for cases in (T.HEAD_CASES, T.GRU_CASES, T.UAM_CASES):
        vals = list(cases.values())
        assert any(v[0] > 0 for v in vals) and any(v[0] == 0 for v in vals)          # inline / up-front noise
        assert any(v[3] for v in vals) and any(not v[3] for v in vals)               # partial / full last block
    assert any(v[1] > 0 for v in T.HEAD_CASES.values()) and any(v[1] == 0 for v in T.HEAD_CASES.values())
    assert any(v[1] > 0 for v in T.GRU_CASES.values()) and any(v[1] == 0 for v in T.GRU_CASES.values())


def test_row_checks_catch_a_wrong_inline_branch():
    """What the GPU tests' assertions do with an inline-noise branch that is wrong, made by hand on
    numpy arrays (no wrong kernel runs on the GPU): the noise of the rows past the up-front window
    taken for the block's first row (``row`` replaced by ``blk * 16``), with epoch 0, or not added.
    Shape: the ATT head's R = 36 905, N = 5 case (4137 rows past the window)."""
    from tests import test_act_rows_gpu as T
    R, N, seed, epoch = 36905, 5, 99, T.C0
    _, kb = T.window(R, 16, 256)
    inline = kb >= T.NB
    assert int(inline.sum()) == 4137
    rng = np.random.default_rng(0)
    episode = rng.integers(1, 9000, size=R // N).astype(np.int32)
    rows = np.arange(R)
    plain = rng.uniform(-1, 1, size=(R, 2)).astype(np.float32)
    want = noise_ref.noise32(seed, epoch, rows, N, episode, 8000, 1.0, 0.05)
    act = np.clip(plain + want, np.float32(-1), np.float32(1))
    T._check_noisy32(plain, act, want, want)                      # the right kernel passes

    def mutant(noise_rows, noise_epoch, add=True):
        nz = want.copy()
        bad = noise_ref.noise32(seed, noise_epoch, noise_rows, N, episode, 8000, 1.0, 0.05)
        nz[inline] = bad[inline]
        a = np.clip(plain + nz, np.float32(-1), np.float32(1)) if add else act.copy()
        return a, nz

    for a, nz in (mutant((rows // 16) * 16, epoch), mutant(rows, 0), mutant(rows, epoch + 1)):
        with pytest.raises(AssertionError):                       # noise_out against the restatement, 1 ulp
            T._check_noisy32(plain, a, nz, want)
    # the noise right in noise_out but not in the action of the inline rows
    a = act.copy()
    a[inline] = plain[inline]
    with pytest.raises(AssertionError):
        T._check_noisy32(plain, a, want, want)
    # R = 32 769: the one inline row is the first of its block, so `blk * 16` is its own row there (that
    # case catches a wrong epoch; the 36 905 / 9307 / 36 907 / 147 643 cases catch a wrong row)
    _, kb1 = T.window(32769, 16, 256)
    only = np.flatnonzero(kb1 >= T.NB)
    assert list(only) == [32768] and only[0] % 16 == 0
    # float64 form (UAM, 1e-12): the same mutants are far outside the tolerance
    w64 = noise_ref.noise64(seed, epoch, rows, N, episode, 10000, 1.0, 0.0)
    for bad in (noise_ref.noise64(seed, epoch, (rows // 16) * 16, N, episode, 10000, 1.0, 0.0),
                noise_ref.noise64(seed, 0, rows, N, episode, 10000, 1.0, 0.0)):
        d = np.abs(np.clip(plain + w64, -1, 1) - np.clip(plain + bad, -1, 1))[inline]
        assert (d > 1e-12).sum() > 0.9 * inline.sum()
