"""Compile-time guard (hipcc, no GPU): every kernel of aac_clip.hip, float and double, keeps its
registers -- no scratch.  With clipping on the two launches stand at every Adam boundary of an update;
a spilled copy buffer or by-value job would cost more than the norm itself."""
import os
import shutil

import pytest

from tests.test_monitor_resources_cpu import HIPCC, _usage


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_clip_kernels_have_no_scratch():
    ks = _usage("aac_clip.hip")
    for want in ("clip_sumsq_kernelIf", "clip_sumsq_kernelId", "adam_clip_kernelIf", "adam_clip_kernelId"):
        assert any(want in k for k in ks), (want, sorted(ks))
    assert len(ks) == 4, sorted(ks)
    for name, u in ks.items():
        assert "ScratchSize" in u, (name, u)
        assert u["ScratchSize"] == 0, (name, u)
