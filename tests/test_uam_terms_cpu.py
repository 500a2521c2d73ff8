"""tests/uam_terms_ref.py against oracle/uam_ref.py on the exact-threshold batches (tests/uam_thresholds.py):
the restated ``ss_reward`` gives the oracle's reward, done, mask and bbc bit for bit, the left-to-right sum
of every row's slots 0..6 is the reward with ``==``, and every reward branch, the crash doubling and the
near-drone band with and without its doubling occur.  No GPU."""
import numpy as np
import pytest

from oracle import uam_ref as U
from tests import uam_terms_ref as R
from tests import uam_thresholds as T


@pytest.mark.parametrize("N", [3, 5])
def test_restatement_equals_oracle(N):
    B = T.build(N)
    st = B.state()
    kinds = np.zeros(5, int)
    band = band_dbl = crash_dbl = minus100 = 0
    used = np.zeros(R.WIDTH, bool)
    for e in range(len(B)):
        o = U.env_from_state(st, e, N)
        _, r, d, cg, bbc, mk, over = o.full_step(np.zeros((N, 2)))
        x = R.uam_env(st, e, N)
        t, r2, d2, cg2, bbc2, mk2, over2 = x.full_step_terms(np.zeros((N, 2)))
        tag = (B.fam[e], B.var[e], e)
        assert np.array_equal(r, r2) and r.dtype == r2.dtype == np.float64, tag
        assert np.array_equal(d, d2) and np.array_equal(cg, cg2) and np.array_equal(bbc, bbc2), tag
        assert np.array_equal(mk, mk2) and over == over2, tag
        assert np.array_equal(R.slot_sum(t), r), (tag, t, r)
        ev = x.events
        for i in range(N):
            k = ev["kind"][i]
            kinds[k] += 1
            # a branch fills only its own contribution slots
            want = {0: (0,), 1: (0,), 2: (0,), 3: (0,), 4: (3, 5, 6)}[k]
            assert all(t[i, s] == 0 for s in range(R.SLOTS) if s not in want), (tag, i, t[i])
            assert (t[i, 0] == 0.0) if k == 4 else (t[i, 0] == U.REACH) if k == 3 else (t[i, 0] <= -U.CRASH), (tag, i)
        band += sum(ev["band"])
        band_dbl += sum(ev["band_dbl"])
        crash_dbl += sum(ev["crash_dbl"])
        minus100 += int(np.sum(r == -100.0))
        used |= (t != 0).any(axis=0)
    assert kinds.min() > 0, dict(zip(R.KINDS, kinds))
    assert band > band_dbl > 0 and crash_dbl > 0 and minus100 > 0, (band, band_dbl, crash_dbl, minus100)
    assert set(np.flatnonzero(used)) == set(R.USED), np.flatnonzero(used)
    if N == 5:      # the batch's census (417 envs)
        assert len(B) == 417
        assert tuple(kinds[:4]) == (27, 60, 86, 28), kinds
        assert (minus100, band, band_dbl) == (52, 60, 12), (minus100, band, band_dbl)
