"""Resource usage of csrc/aac_uam.hip's kernels with the radar-probe kernel in the file, as hipcc reports it
for gfx950 (the command of tests/test_uam_terms_resources_cpu.py).  ``uam_probe_kernel`` shares the geometry
helpers of the step's radar and of the reward map; that must leave the step, reset and reward-map kernels as
the commit before the probe reported them.  The new kernel's figures are printed (DESIGN.md section 4 records
them); its scratch size is 0, as the step's radar has it with the same helpers."""
import os
import shutil

import pytest

from tests.test_kernel_resources_cpu import HIPCC
from tests.test_uam_rewardmap_resources_cpu import RESET, TERMS
from tests.test_uam_terms_resources_cpu import PLAIN, _usage

pytestmark = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
# what the parent commit reports for uam_reward_map_kernel with the same command
RMAP = {"VGPRs": 100, "TotalSGPRs": 106, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 2016,
        "Occupancy [waves/SIMD]": 4}


@pytest.fixture(scope="module")
def kernels():
    return _usage("aac_uam.hip")


def _one(kernels, key):
    hit = [v for k, v in kernels.items() if key in k]
    assert len(hit) == 1, (key, sorted(kernels))
    return hit[0]


@pytest.mark.parametrize("key,want", [("uam_step_kernelILb0E", PLAIN), ("uam_step_kernelILb1E", TERMS),
                                      ("uam_reset_kernel", RESET), ("uam_reward_map_kernel", RMAP)])
def test_existing_kernels_report_the_parent_figures(kernels, key, want):
    got = _one(kernels, key)
    assert {k: got.get(k) for k in want} == want, got


def test_probe_kernel_figures_are_printed_and_scratch_is_zero(kernels):
    got = _one(kernels, "uam_probe_kernel")
    print("uam_probe_kernel:", {k: got.get(k) for k in PLAIN})
    assert all(k in got for k in PLAIN), got
    assert got["ScratchSize [bytes/lane]"] == 0, got
