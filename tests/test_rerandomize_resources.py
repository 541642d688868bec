"""Resource guard for the re-randomization kernels (CPU: compiles rerandomize.hip for gfx950 and reads the
code-object descriptors, as test_public_key_resources.py does).  Neither kernel may spill to scratch, and each
may hold at most 40,960 bytes of LDS, a quarter of a CU's 160 KB: k_rerand_zero's 32 KB table [-P | P], R, the
segment's noise words and the waves' partial sums with room to spare; k_rerand_add stages nothing.  As built (hipcc -O3, gfx950):

    kernel           registers (next_free_vgpr)  LDS      scratch
    k_rerand_zero      108                        35584    0
    k_rerand_add       49                         0        0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors

KERNELS = ["k_rerand_zero", "k_rerand_add"]


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "rerandomize.hip"), tmp_path_factory.mktemp("rerandomize"))
    out = {}
    for name in KERNELS:
        ks = [v for k, v in d.items() if name in k]
        assert len(ks) == 1, f"{name} not found in rerandomize.hip"
        print(name, {k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
        out[name] = ks[0]
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(desc, kernel):
    assert desc[kernel]["private_segment_fixed_size"] == 0, "scratch spill"


@pytest.mark.parametrize("kernel", KERNELS)
def test_lds_bound(desc, kernel):
    assert desc[kernel]["group_segment_fixed_size"] <= 40960, f"{desc[kernel]['group_segment_fixed_size']} bytes of LDS"
