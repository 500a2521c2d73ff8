"""The UAM oracle (oracle/uam_ref.py) on the exact-threshold states of tests/uam_thresholds.py, without a
GPU: ``full_step`` from the builder's states against the exact checkers (rational predicates on the GEOS
float vertices, float norms where the reference compares floats).  Inside ``geos.BAND`` the oracle's
closed forms hand the decision to the exact tests; without that hand-over the predicate families
(goal_*, cloud_*, rw_corner, go_target) and rw_graze fail here."""
import numpy as np
import pytest

from oracle import geos
from oracle import uam_ref as U
from tests import uam_thresholds as T

N = 3


@pytest.fixture(scope="module")
def stepped():
    """The oracle's one step from every env of the N = 3 batch, in the layout ``T.check`` reads."""
    B = T.build(N)
    pre = B.state()
    E = len(B)
    out = dict(mask=np.zeros((E, N), np.uint8), reward=np.zeros((E, N)), radar=np.zeros((E, N, U.N_RAYS)),
               conf_cur=np.zeros((E, N), np.int32), cloud_tgt=np.zeros(E, np.int32), clouds=np.zeros((E, 2, 2)),
               pos=np.zeros((E, N, 2)))
    for e in range(E):
        o = U.env_from_state(pre, e, N)
        obs, r, d, cg, bbc, mk, over = o.full_step(np.zeros((N, 2)))
        s = U.state_of(o)
        out["mask"][e], out["reward"][e], out["radar"][e] = mk, r, obs[2]
        out["conf_cur"][e] = o.tdcpa_out[2]
        out["cloud_tgt"][e], out["clouds"][e], out["pos"][e] = s["cloud_tgt"], s["clouds"], s["pos"]
    return B, out


def test_oracle_on_thresholds(stepped):
    B, out = stepped
    seen, count = T.check(B, out, where="oracle")
    T.both_ways(seen)
    assert set(count) == set(T.BOOL_FAMILIES) | set(T.RADAR_FAMILIES)


def test_builder_positions_exact(stepped):
    """The subject's post-step position is the builder's, bit for bit (stationary or dyadic moves)."""
    B, out = stepped
    for e in range(len(B)):
        assert np.array_equal(out["pos"][e], B.rows[e]["post"]), (B.fam[e], e)


def test_bound_band_inputs():
    """A condition on the inputs: the capsule band holds both outcomes in fair shares, by the
    reference's full vertex loop alone."""
    B = T.build(N)
    hits = [geos.bound_crash(B.rows[e]["pos"][B.subj[e]], B.rows[e]["post"][B.subj[e]], U.BOUND, U.PB)
            for e, f in enumerate(B.fam) if f == "bound"]
    assert len(hits) >= 32 and 0.05 < np.mean(hits) < 0.95, np.mean(hits)


def test_radar_families_hold_both_outcomes():
    """The threshold ray itself decides between a hit well inside its length and none."""
    B = T.build(N)
    for f in ("tangent", "rw_corner_ray", "rw_graze"):
        vals = [B.exp[e]["radar"][B.exp[e]["ray"]] for e in range(len(B)) if B.fam[e] == f and "ray" in B.exp[e]]
        assert min(vals) < U.RADAR_DIST - 0.1 and max(vals) > U.RADAR_DIST - 1e-6, (f, min(vals), max(vals))
