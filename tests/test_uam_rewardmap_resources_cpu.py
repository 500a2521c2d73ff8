"""Resource usage of csrc/aac_uam.hip's kernels with the reward-map kernel in the file, as hipcc reports it for
gfx950 (the command of tests/test_uam_terms_resources_cpu.py).  ``uam_reward_map_kernel`` shares the step's
geometry helpers and its phase-5 tail (``phase5_tail``); that must leave the step and reset kernels as the
commit before the map reported them.
The new kernel's figures are printed, not bounded (DESIGN.md section 4 records them)."""
import os
import shutil

import pytest

from tests.test_kernel_resources_cpu import HIPCC
from tests.test_uam_terms_resources_cpu import PLAIN, _usage

pytestmark = pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
# what the parent commit reports with the same command
TERMS = {"VGPRs": 128, "TotalSGPRs": 106, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 30928,
         "Occupancy [waves/SIMD]": 4}
RESET = {"VGPRs": 118, "TotalSGPRs": 106, "ScratchSize [bytes/lane]": 0, "LDS Size [bytes/block]": 31440,
         "Occupancy [waves/SIMD]": 4}


@pytest.fixture(scope="module")
def kernels():
    return _usage("aac_uam.hip")


def _one(kernels, key):
    hit = [v for k, v in kernels.items() if key in k]
    assert len(hit) == 1, (key, sorted(kernels))
    return hit[0]


@pytest.mark.parametrize("key,want", [("uam_step_kernelILb0E", PLAIN), ("uam_step_kernelILb1E", TERMS),
                                      ("uam_reset_kernel", RESET)])
def test_step_and_reset_kernels_report_the_parent_figures(kernels, key, want):
    got = _one(kernels, key)
    assert {k: got.get(k) for k in want} == want, got


def test_reward_map_kernel_figures_are_printed(kernels):
    got = _one(kernels, "uam_reward_map_kernel")
    print("uam_reward_map_kernel:", {k: got.get(k) for k in PLAIN})
    assert all(k in got for k in PLAIN), got
