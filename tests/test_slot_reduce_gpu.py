"""The slot reduce shared by the three slot-based tallies (csrc/aac_slots.h: stats_reduce_kernel,
terms_reduce_kernel, sortie_reduce_kernel), pinned directly: no env and no accumulate launch.

Each wrapper is built at E giving G = 1, 257 and 258 slots (at 257 thread 0 folds two slots, at 258
threads 0 and 1 do), its ``slots`` tensor is filled by hand -- seeded random int64 counters, doubles of
mixed sign and magnitude so that the order of the additions matters, +-inf in some min / max slots -- and
the totals of ``aac_*_reduce`` are compared bit for bit with a numpy fold in the kernel's stated order:
lane t over the slots g = t, t + 256, ... ascending, then entry j with j + 128, 64, ... 1.  With
``clear`` every slot is left at its identity (0, +inf, -inf by kind), except the stats record's
``under_quota`` column, which the accumulate launch rewrites whole; the sortie histogram is zeroed."""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ISUM, IKEEP, DSUM, DMIN, DMAX = range(5)      # int sum, int sum kept on clear, double sum / min / max
GS = (1, 257, 258)


def _kinds(which):
    if which == "stats":        # 11 counters, under_quota, return sum / sqsum / min / max, reach_hist[65]
        return [ISUM] * 11 + [IKEEP, DSUM, DSUM, DMIN, DMAX] + [ISUM] * 65
    if which == "terms":        # episodes, then sum / sqsum / min / max of the 8 slots
        return [ISUM] + [DSUM] * 16 + [DMIN] * 8 + [DMAX] * 8
    return [ISUM] * 9 + [DSUM, DSUM, DMIN, DMAX, DSUM, DSUM]      # sortie


def _make(which, G):
    """The wrapper with exactly G slots at its smallest N, and its reduce entry point."""
    from multi_agent_aac_amd import _native
    lib = _native.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    if which == "stats":
        from multi_agent_aac_amd.stats import EPW, EpisodeStats
        E = (G - 1) * EPW + 1
        return EpisodeStats(E, 1, 8, device=dev), E, lib.aac_stats_reduce
    env = types.SimpleNamespace(N=1, device=dev, terms=None, cfg=types.SimpleNamespace(episode_length=8))
    if which == "terms":
        from multi_agent_aac_amd.terms import EPW, RewardLedger
        env.E = E = (G - 1) * EPW + 1
        return RewardLedger(env), E, lib.aac_terms_reduce
    from multi_agent_aac_amd.sorties import EPW, SortieStats
    env.E = E = (G - 1) * EPW + 1
    return SortieStats(env), E, lib.aac_sortie_reduce


def _fill(kinds, G, seed):
    """int64 [G][F] slot words: counters, or the bits of doubles."""
    rng = np.random.default_rng([seed, G, len(kinds)])
    raw = np.zeros((G, len(kinds)), dtype=np.int64)
    d = raw.view(np.float64)
    for f, k in enumerate(kinds):
        if k in (ISUM, IKEEP):
            raw[:, f] = rng.integers(-2 ** 40, 2 ** 40, size=G)
        else:
            v = rng.choice([-1.0, 1.0], size=G) * rng.random(G) * 10.0 ** rng.integers(-8, 13, size=G)
            if k != DSUM:       # slots no episode reached keep their identity; the other infinity is a value too
                v[rng.random(G) < 0.25] = np.inf
                v[rng.random(G) < 0.25] = -np.inf
            d[:, f] = v
    return raw


def _fold(col, kind):
    """One field's total: lane t takes slots t, t + 256, ... in order, then the 128 ... 1 tree."""
    if kind in (ISUM, IKEEP):
        acc, op = np.zeros(256, dtype=np.int64), np.add
    else:
        col = col.view(np.float64)
        acc = np.full(256, {DSUM: 0.0, DMIN: np.inf, DMAX: -np.inf}[kind])
        op = {DSUM: np.add, DMIN: np.fmin, DMAX: np.fmax}[kind]
    for g0 in range(0, len(col), 256):
        c = col[g0:g0 + 256]
        acc[:len(c)] = op(acc[:len(c)], c)
    s = 128
    while s:
        acc[:s] = op(acc[:s], acc[s:2 * s])
        s >>= 1
    return acc[:1].view(np.int64)[0]


def _identity(kinds, G):
    raw = np.zeros((G, len(kinds)), dtype=np.int64)
    d = raw.view(np.float64)
    for f, k in enumerate(kinds):
        if k in (DMIN, DMAX):
            d[:, f] = np.inf if k == DMIN else -np.inf
    return raw


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("which", ["stats", "terms", "sortie"])
def test_reduce_order_and_clear(native_lib, which, G):
    kinds = _kinds(which)
    w, E, reduce = _make(which, G)
    assert tuple(w.slots.shape) == (G, len(kinds)) and w.slots.dtype == torch.int64
    raw = _fill(kinds, G, seed=7)
    want = np.array([_fold(np.ascontiguousarray(raw[:, f]), k) for f, k in enumerate(kinds)], dtype=np.int64)
    w.slots.copy_(torch.from_numpy(raw))
    if which == "sortie":
        w.collide_hist.fill_(3)

    def run(clear):
        w.totals.fill_(-1)
        rc = reduce(ctypes.byref(w._st), E, ctypes.c_void_p(w.totals.data_ptr()), int(clear),
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        return w.totals.cpu().numpy().copy(), w.slots.cpu().numpy().copy()

    tot, slots = run(False)
    assert np.array_equal(tot, want), np.flatnonzero(tot != want)
    assert np.array_equal(slots, raw)
    if which == "sortie":
        assert bool((w.collide_hist == 3).all())

    tot, slots = run(True)
    assert np.array_equal(tot, want), np.flatnonzero(tot != want)
    ident = _identity(kinds, G)
    keep = [f for f, k in enumerate(kinds) if k == IKEEP]
    assert keep == ([11] if which == "stats" else [])
    ident[:, keep] = raw[:, keep]
    assert np.array_equal(slots, ident), np.argwhere(slots != ident)[:8]
    if which == "sortie":
        assert bool((w.collide_hist == 0).all())

    # the cleared slots fold to the identities (and the kept column to its sum again)
    tot, _ = run(False)
    want0 = np.array([_fold(np.ascontiguousarray(ident[:, f]), k) for f, k in enumerate(kinds)], dtype=np.int64)
    assert np.array_equal(tot, want0)
