"""Compile-time guard (hipcc, no GPU): every kernel of aac_sortie.hip keeps its registers -- no
scratch.  The accumulate launch runs once per env step between the step and the reset; a spilled log row
or set of partial sums would cost more than the tally itself."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _usage(src):
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
                          "--offload-device-only", "-c", "-o", os.devnull, "-I", os.path.join(ROOT, "include"),
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(ROOT, "multi_agent_aac_amd", "csrc", src)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_sortie_kernels_have_no_scratch():
    ks = _usage("aac_sortie.hip")
    for want in ("sortie_accum_kernel", "sortie_log_kernel", "sortie_reduce_kernel"):
        assert any(want in k for k in ks), (want, sorted(ks))
    for name, u in ks.items():
        assert "ScratchSize" in u, (name, u)
        assert u["ScratchSize"] == 0, (name, u)
        # six partial sums of 256 threads + the 2048-bin collide_hist table + the counters
        assert u.get("LDS Size", 0) <= 6 * 256 * 8 + 2048 * 4 + 64, (name, u)
