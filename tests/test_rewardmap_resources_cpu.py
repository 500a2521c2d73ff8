"""Compile-time guard (hipcc, no GPU): the reward map left the env's existing kernels alone.  The map kernel
calls the step's own reward functions (``att_reward`` / ``wgru_reward`` compiled without their state writes,
``drone_contacts``, ``building_scan``, ...) and the helpers the step, reset, band-fix and probe kernels use
(``building_hit``, ``goal_reached``, ``bound_crash``, ``radar_ray_exact``); a second caller and a function
boundary can change what the compiler inlines and schedules where, so their VGPR / SGPR / LDS / scratch
figures must be the ones the commit before the map had, taken with the command of
tests/test_probe_resources_cpu.py."""
import os
import shutil

import pytest

from tests.test_kernel_resources_cpu import HIPCC
from tests.test_probe_resources_cpu import PARENT as BEFORE_PROBE
from tests.test_probe_resources_cpu import _name, _usage

# kernel -> (VGPRs, TotalSGPRs, LDS bytes / block, scratch bytes / lane) before the reward map was added
PARENT = dict(BEFORE_PROBE)
PARENT["radar_probe_kernel"] = (118, 106, 8448, 0)


def _rmap_name(mangled):
    if "reward_map_kernelILi0E" in mangled:
        return "reward_map_kernel<0>"
    if "reward_map_kernelILi1E" in mangled:
        return "reward_map_kernel<1>"
    return None


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_existing_env_kernels_keep_their_resources():
    got, new = {}, {}
    for k, u in _usage("aac_env.hip").items():
        fig = (u["VGPRs"], u["TotalSGPRs"], u["LDS Size"], u["ScratchSize"])
        if _rmap_name(k):
            new[_rmap_name(k)] = fig
        elif _name(k):
            got[_name(k)] = fig
    # no bound on the new kernels: DESIGN records their figures
    for k in sorted(new):
        print(k, "(VGPRs, SGPRs, LDS, scratch):", new[k])
    assert sorted(new) == ["reward_map_kernel<0>", "reward_map_kernel<1>"]
    assert len(PARENT) == 19 and got == PARENT
