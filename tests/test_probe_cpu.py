"""The radar-probe restatement (tests/probe_ref.py) against the oracles it is built from, the hand-built
ties, the share of rays the GPU tests may excuse, and the ctypes binding's size.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import env_ref
from tests import probe_cases as C
from tests import probe_ref as R
from tests import thresholds as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_restatement_dist_is_scalar_env_radar(occ, mode):
    """``dist`` equals ``ScalarEnv.radar`` bit for bit on random clustered states; every kind occurs."""
    N = 4
    env = env_ref.ScalarEnv(N, occ, radar_mode=mode)
    kinds = set()
    for row in C.random_rows(12, N, seed=10 + mode):
        for i, ag in env.all_agents.items():
            ag.pos = row[i].copy()
        for i in range(N):
            want = env.radar(i)
            recs = [R.probe_ray(row, i, r, occ, mode) for r in range(18)]
            assert [x["dist"] for x in recs] == want.tolist(), (mode, i)
            for r, x in enumerate(recs):
                kinds.add(x["kind"])
                assert x["end"] == T.ray_end(tuple(row[i]), r)
                assert (x["kind"] == 0) == (x["id"] == -1)
                np.testing.assert_allclose(np.hypot(x["point"][0] - row[i, 0], x["point"][1] - row[i, 1]), x["dist"],
                                           rtol=0, atol=1e-9)
    assert kinds == {0: {0, 1}, 1: {0, 2, 3}, 2: {0, 1, 2, 3}}[mode], kinds


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_restatement_on_threshold_families(mode):
    """The subject's 18 distances on ``thresholds.build(3)``'s radar families against the rationals of
    ``thresholds.exact_radar``: the drone families in mode 0, the cell families in mode 1, every third
    (on / below / above) triple of all of them in mode 2.  1e-9: the fp64 parity bar (the exact value
    is rounded once, the restatement's a few times)."""
    fam, var, st, occ = T.build(3, seed=3)
    drone = ("tangent", "start_on")
    idx = [e for e, f in enumerate(fam) if f in T.RADAR_FAMILIES]
    if mode == 0:
        idx = [e for e in idx if fam[e] in drone]
    elif mode == 1:
        idx = [e for e in idx if fam[e] not in drone]
    else:
        idx = [e for k, e in enumerate(idx) if (k // 3) % 3 == 0]
    assert len(idx) > 30
    hits = 0
    for e in idx:
        p = st["pos"][e]
        ex = T.exact_radar(tuple(p[0]), [tuple(x) for x in p[1:]], occ, mode)
        d = np.array([R.probe_ray(p, 0, r, occ, mode)["dist"] for r in range(18)])
        np.testing.assert_allclose(d, ex, rtol=0, atol=1e-9, err_msg=f"{fam[e]} {var[e]} env {e} mode {mode}")
        hits += int((ex < 15.0 - 1e-6).any())
    assert 0 < hits


def test_hand_built_ties():
    """The tie rule on exactly representable coordinates (probe_cases.HAND_WANT says why each holds)."""
    occ = C.hand_map()
    for (m, i, r), (kind, idx, dist, point) in C.HAND_WANT.items():
        c, e, L, hits = R.candidates(C.HAND_ROWS[m], i, r, occ, 2)
        rec = R.probe_ray(C.HAND_ROWS[m], i, r, occ, 2)
        assert (rec["kind"], rec["id"], rec["dist"], tuple(rec["point"])) == (kind, idx, dist, point), (m, i, r, rec)
        tied = sorted((h[1], h[2]) for h in hits if R.eligible(h, L) and h[0] == rec["dist"])
        if (m, i, r) == (0, 0, 0):
            assert tied == [(2, 135), (2, 136)]              # both cells, bit-equal
        if (m, i, r) == (1, 0, 0):
            assert tied == [(1, 1), (2, 135)]                # drone and cell, bit-equal
        if (m, i, r) == (2, 0, 0):
            assert L == 15.0 and tied == [(2, 135)]          # d == len exactly
    # order independence: the record does not change when the rows' cells are listed the other way round
    flipped = occ[:, ::-1]
    rec = R.probe_ray(C.HAND_ROWS[0] * [1, -1] + [0, 640.0], 0, 0, flipped, 2)      # mirrored in y = 320
    assert rec["kind"] == 2 and rec["id"] == 10 * C.GH + 6 and rec["dist"] == 10.0  # cells (10, 6), (10, 7): the lower


@pytest.mark.parametrize("name", ["drones2", "drones5", "obstacles3", "obstacles8", "combined5", "twomap"])
def test_excused_share_of_the_gpu_cases(occ, name):
    """The GPU comparison excuses kind / id / point of rays whose two best candidates lie within 1e-9 in the
    restatement, at most 1 % of a case's rays: the reset states of its seeds and the states its three
    free-running steps lead to stay within that here."""
    mode, N, variant = C.CASES[name]
    st, _, _, stack, mi = C.reset_state(occ, name)
    for where, pos in (("reset", st), ("flown", C.flown(st, C.actions(name), 10.0 if variant == "wgru" else 5.0))):
        ref = R.probe_rows(pos, stack, mode, mi)
        assert ref["close"].mean() <= 0.01, (name, where, ref["close"].sum())


def test_binding_size_matches_header():
    from multi_agent_aac_amd import _native
    hdr = open(os.path.join(ROOT, "include", "aac_probe.h")).read()
    size = int(re.search(r"#define AAC_PROBE_OUT_BYTES (\d+)", hdr).group(1))
    assert ctypes.sizeof(_native.ProbeOut) == size
    fields = re.findall(r"^\s+(?:double|uint8_t|int32_t) \*(\w+);", hdr[hdr.index("typedef struct"):], re.M)
    assert [f for f, _ in _native.ProbeOut._fields_] == fields
    hip = open(os.path.join(ROOT, "multi_agent_aac_amd", "csrc", "aac_env.hip")).read()
    assert "static_assert(sizeof(aac_probe_out) == AAC_PROBE_OUT_BYTES" in hip
