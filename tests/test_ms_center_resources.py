"""Resource guard for the centered modulus switch's kernel (CPU: compiles ms_center.hip for gfx950 and reads the
code-object descriptor, as test_rerandomize_resources.py does).  k_ms_center may not spill to scratch and may hold
at most 1 KB of LDS: it stages nothing (one wave per row, the partial sums meet by lane exchanges), so any LDS at
all would be a change of design.  As built (hipcc -O3, gfx950):

    kernel        registers (next_free_vgpr)  LDS  scratch
    k_ms_center     42                         0    0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors

KERNELS = ["k_ms_center"]


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "ms_center.hip"), tmp_path_factory.mktemp("ms_center"))
    out = {}
    for name in KERNELS:
        ks = [v for k, v in d.items() if name in k]
        assert len(ks) == 1, f"{name} not found in ms_center.hip"
        print(name, {k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
        out[name] = ks[0]
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(desc, kernel):
    assert desc[kernel]["private_segment_fixed_size"] == 0, "scratch spill"


@pytest.mark.parametrize("kernel", KERNELS)
def test_lds_bound(desc, kernel):
    assert desc[kernel]["group_segment_fixed_size"] <= 1024, f"{desc[kernel]['group_segment_fixed_size']} bytes of LDS"
