"""CPU side of the UAM radar probe (include/aac_uam_probe.h, ``probe.UamRadarProbe``): the restatement of
tests/uam_probe_ref.py against the oracle's own radar, the coverage of the seeded batches the GPU tests use,
the tie rule, and the binding's constants."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from oracle import uam_ref as U
from tests import uam_probe_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = P.BATCHES
reference = P.reference
# rays per kind (none, runway, bound, cloud, aircraft) of the three batches, from the oracle's candidates
COUNTS = {(20, 3, 0): (477, 55, 52, 228, 268), (20, 5, 0): (749, 80, 84, 352, 535),
          (10, 16, 0): (524, 91, 55, 240, 1970)}


@pytest.mark.parametrize("E,N,seed", BATCHES)
def test_restatement_dist_is_the_oracle_radar(E, N, seed):
    st, ref = reference(E, N, seed)
    for e in range(E):
        env = U.env_from_state(st, e, N)
        for i in range(N):
            want = env.radar(i)
            assert np.array_equal(ref["dist"][e, i].view(np.int64), want.view(np.int64)), (e, i)


@pytest.mark.parametrize("E,N,seed", BATCHES)
def test_every_kind_occurs_and_no_near_ties(E, N, seed):
    st, ref = reference(E, N, seed)
    counts = tuple(int(c) for c in np.bincount(ref["kind"].reshape(-1), minlength=5))
    print("kinds", dict(zip(P.KINDS, counts)))
    assert counts == COUNTS[(E, N, seed)]
    assert all(c > 0 for c in counts)
    near = ref["runner_up"] - ref["dist"] <= 1e-9
    print("rays with a runner-up within 1e-9:", int(near.sum()), "of", near.size)
    assert near.size == E * N * 18 and not near.any()
    # the record's own consistency: ids in range, NONE at the ray end, |point - pos| == dist
    k, idx = ref["kind"], ref["id"]
    assert (idx[k == P.NONE] == -1).all() and (idx[k == P.RUNWAY] == 0).all()
    assert ((idx[k == P.BOUND] >= 0) & (idx[k == P.BOUND] < 4)).all()
    assert ((idx[k == P.CLOUD] >= 0) & (idx[k == P.CLOUD] < 2)).all()
    assert ((idx[k == P.AIRCRAFT] >= 0) & (idx[k == P.AIRCRAFT] < N)).all()
    assert np.array_equal(ref["point"][k == P.NONE], ref["end"][k == P.NONE])
    d = ref["point"] - st["pos"][:, :, None, :]
    assert np.array_equal(np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]), ref["dist"])


def test_tie_rule_on_a_hand_built_list():
    end, far = (5.0, 0.0), (9.0, 9.0)
    hit = lambda d: (d, (d, 0.0))          # noqa: E731
    # bit-equal distances: the first in test order, i.e. the lowest (kind, id)
    cands = [(P.RUNWAY, 0, None), (P.BOUND, 0, None), (P.BOUND, 1, hit(2.0)), (P.CLOUD, 0, hit(2.0)),
             (P.AIRCRAFT, 1, hit(2.0)), (P.AIRCRAFT, 2, hit(2.0))]
    assert P.select(5.0, end, cands) == (2.0, P.BOUND, 1, (2.0, 0.0), 2.0)
    assert P.select(5.0, end, cands[3:]) == (2.0, P.CLOUD, 0, (2.0, 0.0), 2.0)
    assert P.select(5.0, end, cands[4:]) == (2.0, P.AIRCRAFT, 1, (2.0, 0.0), 2.0)
    # a later candidate wins only when strictly nearer
    nearer = cands + [(P.AIRCRAFT, 3, hit(math.nextafter(2.0, 0.0)))]
    got = P.select(5.0, end, nearer)
    assert got[:3] == (math.nextafter(2.0, 0.0), P.AIRCRAFT, 3) and got[4] == 2.0
    # a candidate bit-equal to the ray length leaves the record NONE, the point the ray end
    assert P.select(5.0, end, [(P.BOUND, 2, (5.0, far)), (P.AIRCRAFT, 0, (5.0, far))]) == (5.0, P.NONE, -1, end, 5.0)
    assert P.select(5.0, end, []) == (5.0, P.NONE, -1, end, math.inf)
    assert P.select(5.0, end, [(P.CLOUD, 1, hit(1.0))]) == (1.0, P.CLOUD, 1, (1.0, 0.0), 5.0)


def _define(name):
    src = open(os.path.join(ROOT, "include", "aac_uam_probe.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


def test_struct_size_and_constants():
    from multi_agent_aac_amd import _native, probe
    assert _define("AAC_UAM_PROBE_OUT_BYTES") == ctypes.sizeof(_native.UamProbeOut) == 40
    assert [n for n, _ in _native.UamProbeOut._fields_] == ["dist", "point", "end", "kind", "id"]
    assert _define("AAC_UAM_PROBE_RAYS") == probe.N_RAYS == P.N_RAYS == 18
    assert _define("AAC_UAM_PROBE_PAIRS") * 18 <= 256
    assert probe.UamRadarProbe.KINDS == P.KINDS == ("none", "runway", "bound", "cloud", "aircraft")
    for code, name in enumerate(("NONE", "RUNWAY", "BOUND", "CLOUD", "AIRCRAFT")):
        assert _define("AAC_UAM_PROBE_" + name) == code == getattr(P, name)


def test_symbol_is_exported(native_lib):
    from multi_agent_aac_amd import _native, uam
    assert "aac_uam_probe" in _native.EXPORTS and "aac_uam_probe" in uam.EXPORTS
    assert hasattr(_native.lib(), "aac_uam_probe")          # exported by the built library
