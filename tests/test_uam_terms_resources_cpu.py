"""Resource usage of the two instantiations of ``uam_step_kernel`` (csrc/aac_uam.hip) as hipcc reports it
for gfx950, the method of tests/test_kernel_resources_cpu.py.  The kernel is built
``__launch_bounds__(256, 4)``: four workgroups share a CU's 160 KB of LDS with the 8 KB of dynamic LDS
each takes at N = 16, so the static LDS has to stay at or under 32 KB, and the 4-wave register budget is
128 VGPRs.  The plain form must report what it reported before the terms form existed."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_kernel_resources_cpu import HIPCC, ROOT

pytestmark = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
PLAIN = {"VGPRs": 128, "TotalSGPRs": 106, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 30928,
         "Occupancy [waves/SIMD]": 4}


def _usage(src):
    """{kernel: {field: value}} with every field of the remark, its unit included (the parser of
    tests/test_kernel_resources_cpu.py keeps the unit-less fields only)."""
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
        m = re.search(r"remark:\s+(\S.*?): (\d+) \[-Rpass", line)
        if m and cur:
            kernels[cur][m.group(1)] = int(m.group(2))
    return kernels


@pytest.fixture(scope="module")
def step_kernels():
    ks = {k: v for k, v in _usage("aac_uam.hip").items() if "uam_step_kernel" in k}
    # Itanium mangling of the bool template argument: ILb0E / ILb1E
    plain = [v for k, v in ks.items() if "uam_step_kernelILb0E" in k]
    terms = [v for k, v in ks.items() if "uam_step_kernelILb1E" in k]
    assert len(ks) == 2 and len(plain) == 1 and len(terms) == 1, sorted(ks)
    return plain[0], terms[0]


def test_plain_form_reports_the_parent_numbers(step_kernels):
    plain, _ = step_kernels
    assert {k: plain.get(k) for k in PLAIN} == PLAIN, plain


def test_terms_form_keeps_four_waves_and_no_scratch(step_kernels):
    _, terms = step_kernels
    assert terms["ScratchSize [bytes/lane]"] == 0, terms
    assert terms["Occupancy [waves/SIMD]"] == 4, terms
    assert terms["VGPRs"] <= 128, terms
    assert terms["LDS Size [bytes/block]"] <= 32768, terms
