"""Resource guard for the resident client key's kernels (CPU: compiles client_ops.hip for gfx950 and reads the
code-object descriptors, as test_oprf_resources.py does).  Neither kernel may spill to scratch.  k_client_encrypt
keeps one ChaCha block per lane in registers, exchanges quarters over the lanes of a quad and sums over the lanes of
a wave; its only LDS is the four waves' partial sums, 4 x 8 = 32 bytes, and the bound below is that figure: anything
more would be a change of design.  k_client_phase is one wave per row and uses none.  As built (hipcc -O3, gfx950):

    kernel              registers (next_free_vgpr)  LDS  scratch
    k_client_encrypt      66                        32   0
    k_client_phase        63                         0   0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors

KERNELS = {"k_client_encrypt": 32, "k_client_phase": 0}  # LDS bytes


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "client_ops.hip"), tmp_path_factory.mktemp("client_ops"))
    out = {}
    for name in KERNELS:
        ks = [v for k, v in d.items() if name in k]
        assert len(ks) == 1, f"{name} not found in client_ops.hip"
        print(name, {k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
        out[name] = ks[0]
    return out


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_no_scratch(desc, kernel):
    assert desc[kernel]["private_segment_fixed_size"] == 0, "scratch spill"


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_lds_bound(desc, kernel):
    assert desc[kernel]["group_segment_fixed_size"] <= KERNELS[kernel], f"{desc[kernel]['group_segment_fixed_size']} bytes of LDS"
