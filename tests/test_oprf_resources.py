"""Resource guard for the oblivious pseudo-random values' kernels (CPU: compiles oprf.hip for gfx950 and reads the
code-object descriptors, as test_ms_center_resources.py does).  Neither kernel may spill to scratch, and neither
may hold more than 1 KB of LDS: k_oprf_rows keeps one ChaCha block per lane in registers and exchanges quarters
over the lanes of a quad, k_oprf_body_add is one load and one store per lane, so any LDS at all would be a change
of design.  As built (hipcc -O3, gfx950):

    kernel            registers (next_free_vgpr)  LDS  scratch
    k_oprf_rows         34                        0    0
    k_oprf_body_add      6                         0    0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors

KERNELS = ["k_oprf_rows", "k_oprf_body_add"]


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "oprf.hip"), tmp_path_factory.mktemp("oprf"))
    out = {}
    for name in KERNELS:
        ks = [v for k, v in d.items() if name in k]
        assert len(ks) == 1, f"{name} not found in oprf.hip"
        print(name, {k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
        out[name] = ks[0]
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(desc, kernel):
    assert desc[kernel]["private_segment_fixed_size"] == 0, "scratch spill"


@pytest.mark.parametrize("kernel", KERNELS)
def test_lds_bound(desc, kernel):
    assert desc[kernel]["group_segment_fixed_size"] <= 1024, f"{desc[kernel]['group_segment_fixed_size']} bytes of LDS"
