"""Compile-time guards (hipcc, no GPU) of the reward ledger: every kernel of aac_terms.hip keeps its
registers (no scratch), and the step kernel's terms instantiations exist for every (variant, radar
mode, tail) the plain ones exist for, with no scratch and within the 128 VGPRs of 4 waves per SIMD."""
import shutil

import pytest

from tests.test_kernel_resources_cpu import HIPCC, _usage

pytestmark = pytest.mark.skipif(not shutil.which(HIPCC), reason="hipcc not available")


def test_terms_kernels_have_no_scratch():
    ks = _usage("aac_terms.hip")
    for want in ("terms_accum_kernel", "terms_reduce_kernel", "terms_record_kernel"):
        assert any(want in k for k in ks), (want, sorted(ks))
    for name, u in ks.items():
        assert u.get("ScratchSize", 0) == 0, (name, u)


def test_step_kernel_terms_forms_match_the_plain_ones():
    ks = {k: v for k, v in _usage("aac_env.hip").items() if "step_kernel" in k}
    plain = {k: v for k, v in ks.items() if "ELb0EEEv" in k}          # TERMS = false: ...ELb<tail>ELb0EEEv
    assert len(plain) == 8 and len(ks) == 16, sorted(ks)
    for k, u in plain.items():
        t = ks[k.replace("ELb0EEEv", "ELb1EEEv")]
        assert t.get("ScratchSize", 0) == 0 and u.get("ScratchSize", 0) == 0, (k, u, t)
        assert t["VGPRs"] <= 128, (k, t)          # 4 waves per SIMD, as the plain form is built for
