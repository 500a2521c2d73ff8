"""Compile-time guard (hipcc, no GPU): the radar probe left the env's existing kernels alone.  The
point-returning forms added to aac_geom.h (ray_square_pt, ray_vline_pt, ray_hline_pt) now carry the bodies the
step, reset and band-fix kernels inline, so their VGPR / SGPR / LDS / scratch figures must be the ones the
commit before the probe had, taken with the command of tests/test_kernel_resources_cpu.py (its ``_usage``,
here with the LDS line parsed too)."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_kernel_resources_cpu import HIPCC, ROOT

# kernel -> (VGPRs, TotalSGPRs, LDS bytes / block, scratch bytes / lane) before the probe was added
PARENT = {
    "band_fix_kernel": (128, 106, 0, 0),
    "reset_kernel": (108, 106, 37376, 0),
    "step_kernel<1, 1, true, true>": (121, 104, 36352, 0),
    "step_kernel<1, 1, false, true>": (118, 106, 36352, 0),
    "step_kernel<1, 1, true, false>": (121, 104, 36352, 0),
    "step_kernel<1, 1, false, false>": (118, 106, 36352, 0),
    "step_kernel<0, 0, true, true>": (117, 106, 36352, 0),
    "step_kernel<0, 0, false, true>": (112, 106, 36352, 0),
    "step_kernel<0, 0, true, false>": (117, 106, 36352, 0),
    "step_kernel<0, 0, false, false>": (112, 106, 36352, 0),
    "step_kernel<0, 1, true, true>": (117, 104, 36352, 0),
    "step_kernel<0, 1, false, true>": (112, 106, 36352, 0),
    "step_kernel<0, 1, true, false>": (117, 104, 36352, 0),
    "step_kernel<0, 1, false, false>": (112, 106, 36352, 0),
    "step_kernel<0, 2, true, true>": (127, 104, 36352, 0),
    "step_kernel<0, 2, false, true>": (126, 106, 36352, 0),
    "step_kernel<0, 2, true, false>": (127, 104, 36352, 0),
    "step_kernel<0, 2, false, false>": (126, 106, 36352, 0),
}


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
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/(?:lane|block)\])?: (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


def _name(mangled):
    m = re.search(r"step_kernelILi(\d)ELi(\d)ELb(\d)ELb(\d)EE", mangled)
    if m and "uam" not in mangled:
        return "step_kernel<%s, %s, %s, %s>" % (m.group(1), m.group(2), ("false", "true")[int(m.group(3))],
                                                ("false", "true")[int(m.group(4))])
    for n in ("reset_kernel", "band_fix_kernel", "radar_probe_kernel"):
        if n in mangled:
            return n
    return None


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_existing_env_kernels_keep_their_resources():
    got = {}
    for k, u in _usage("aac_env.hip").items():
        if _name(k):
            got[_name(k)] = (u["VGPRs"], u["TotalSGPRs"], u["LDS Size"], u["ScratchSize"])
    probe = got.pop("radar_probe_kernel")          # no bound on the new kernel: DESIGN records its figures
    print("radar_probe_kernel (VGPRs, SGPRs, LDS, scratch):", probe)
    assert got == PARENT
