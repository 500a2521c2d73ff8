"""The UAM kernels on exact-threshold states (tests/uam_thresholds.py): goals, clouds, the go-around
aircraft and its target switch on the Minkowski 64-gon's apothems and vertices, 64-gons touching the
runway's edges and corners, the bound capsule band, contact / near-band / bearing / tdCPA float
compares, radar rays through a vertex or a runway corner, along a runway edge and an ulp beside it --
each on the threshold and +-1, +-2 ulp off it.

Through the C ABI in three forms: aac_uam_step with few aircraft (N = 3, 5: one env per 16-lane row,
many envs per workgroup), aac_uam_step at N = 16 (4 envs per workgroup, the subject in different
lanes) and the radar phase of aac_uam_reset.  Each is checked
  * against oracle/uam_ref.py from the identical pre-step state: mask, done, bbc, env_done, reach,
    cloud_tgt, conf_cur, conf_pre bit-equal, floats within 1e-9, state within 1e-12;
  * independently of the oracle, every subject row against the exact checkers (rational predicates
    on the GEOS float vertices; float norms / atan2 where the reference compares floats);
  * with both outcomes of every boolean family occurring."""
import numpy as np
import pytest
import torch

from oracle import uam_ref as U
from tests import uam_thresholds as T

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _np_state(env):
    return {k: v.cpu().numpy() for k, v in env.get_state().items()}


def _step(B, N):
    """One zero-action step of the batch on the device: (pre-step state, post-step state, outputs)."""
    from multi_agent_aac_amd import uam
    st = B.state()
    E = len(B)
    env = uam.BatchedUAM(E, N, p3=True, tdcpa=True)
    env.reset(st["pos"], st["goal"], st["cloud_kind"])
    env.set_state(**st)
    pre = _np_state(env)
    for k, v in st.items():
        assert np.array_equal(pre[k], v), k
    env.step(torch.zeros(E, N, 2, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    post = _np_state(env)
    b = env.bufs
    out = {f.name: getattr(b, f.name).cpu().numpy() for f in b.__dataclass_fields__.values()
           if getattr(b, f.name) is not None}
    out["cloud_tgt"], out["clouds"] = post["cloud_tgt"], post["clouds"]
    return pre, post, out


def _cmp_oracle(pre, post, out, e, N, tag):
    o = U.env_from_state(pre, e, N)
    (own, p2, rad, p3), r, d, cg, bbc, mk, over = o.full_step(np.zeros((N, 2)))
    tc, dc, cc, cp = o.tdcpa_out
    ref = U.state_of(o)
    for name, want in (("mask", mk), ("done", d), ("bbc", bbc), ("conf_cur", cc), ("conf_pre", cp)):
        assert np.array_equal(out[name][e].astype(want.dtype), want), (tag, name, out[name][e], want)
    assert bool(out["env_done"][e]) == bool(over), (tag, "env_done")
    assert np.array_equal(post["reach"][e], ref["reach"]), (tag, "reach")
    assert post["cloud_tgt"][e] == ref["cloud_tgt"] and post["step"][e] == ref["step"], (tag, "cloud_tgt / step")
    assert np.array_equal(post["top2"][e], ref["top2"]), (tag, "top2")
    for name, want in (("own", own), ("radar", rad), ("nei", p2), ("nei6", p3), ("reward", r), ("tcpa", tc), ("dcpa", dc)):
        np.testing.assert_allclose(out[name][e].reshape(np.shape(want)), want, rtol=0, atol=TOL, err_msg=f"{tag} {name}")
    for key in ("pos", "vel", "pre_pos", "pre_vel", "heading", "clouds"):
        np.testing.assert_allclose(post[key][e], ref[key], rtol=0, atol=1e-12, err_msg=f"{tag} {key}")


@pytest.mark.parametrize("N", [3, 5])
def test_uam_step_on_thresholds(native_lib, N):
    B = T.build(N)
    pre, post, out = _step(B, N)
    for e in range(len(B)):
        assert np.array_equal(post["pos"][e], B.rows[e]["post"]), (B.fam[e], e)
    seen, count = T.check(B, out, where=f"step N{N}")
    T.both_ways(seen)
    assert set(count) == set(T.BOOL_FAMILIES) | set(T.RADAR_FAMILIES)
    for e in range(len(B)):
        _cmp_oracle(pre, post, out, e, N, (f"step N{N}", B.fam[e], B.var[e], e))


def test_uam_step_on_thresholds_n16(native_lib):
    """4 envs per workgroup, the subject in lanes 0 / 15 of its row: every env against the exact
    checkers, one env per family against the oracle (its Python radar costs ~0.3 s per env here)."""
    N = 16
    B = T.build(N)
    pre, post, out = _step(B, N)
    seen, count = T.check(B, out, where="step N16")
    T.both_ways(seen)
    assert set(count) == set(T.BOOL_FAMILIES) | set(T.RADAR_FAMILIES)
    picks = T.one_per_family(B)
    assert len(picks) <= 24
    for e in picks:
        _cmp_oracle(pre, post, out, e, N, ("step N16", B.fam[e], B.var[e], e))


def test_uam_reset_radar_on_thresholds(native_lib):
    """The reset kernel's own radar phase (aac_uam_reset) with the radar families' positions as
    episode starts: the subject's 18 rays against the exact radar and the oracle's reset."""
    from multi_agent_aac_amd import uam
    N = 3
    B = T.build(N)
    st = B.state()
    E = len(B)
    env = uam.BatchedUAM(E, N, p3=True, tdcpa=True)
    env.reset(st["pos"], st["goal"], st["cloud_kind"])
    torch.cuda.synchronize()
    radar = env.bufs.radar.cpu().numpy()
    checked = 0
    for e, f in enumerate(B.fam):
        if f not in T.RADAR_FAMILIES:
            continue
        si = B.subj[e]
        np.testing.assert_allclose(radar[e, si], T.reset_radar(B, e), rtol=0, atol=TOL, err_msg=f"reset {f} env {e}")
        o = U.UAMEnv(N)
        obs = o.reset(st["pos"][e], st["goal"][e], int(st["cloud_kind"][e, 0]), int(st["cloud_kind"][e, 1]))
        np.testing.assert_allclose(radar[e], obs[2], rtol=0, atol=TOL, err_msg=f"reset oracle {f} env {e}")
        checked += 1
    assert checked > 80
