"""Resource guard for the stored form's kernels (CPU: compiles switched.hip for gfx950 and reads the code-object
descriptors, as test_oprf_resources.py does).  Both kernels are one lane per 64-byte unit, four 16-byte loads and
three dword stores or the reverse: neither may spill to scratch, and any LDS at all would be a change of design.
As built (hipcc -O3, gfx950):

    kernel         registers (next_free_vgpr)  LDS  scratch
    k_ms_pack        22                          0    0
    k_ms_unpack      22                          0    0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors

KERNELS = ["k_ms_pack", "k_ms_unpack"]


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "switched.hip"), tmp_path_factory.mktemp("switched"))
    out = {}
    for name in KERNELS:
        ks = [v for k, v in d.items() if name in k]
        assert len(ks) == 1, f"{name} not found in switched.hip"
        print(name, {k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
        out[name] = ks[0]
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(desc, kernel):
    assert desc[kernel]["private_segment_fixed_size"] == 0, "scratch spill"


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_lds(desc, kernel):
    assert desc[kernel]["group_segment_fixed_size"] == 0, f"{desc[kernel]['group_segment_fixed_size']} bytes of LDS"
