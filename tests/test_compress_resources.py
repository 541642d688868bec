"""Resource guard for the kernels of the compressed computed ciphertexts (CPU: compiles compress.hip for
gfx950 and reads the code-object descriptors, as test_seeded_key_resources.py does).  None of them may
spill to scratch.  LDS: only k_pk_pack holds any -- the 2048 uint16 values of one polynomial, 4096 bytes --
and the others none.  As built (hipcc -O3, gfx950):

    kernel               registers (next_free_vgpr)  LDS    scratch
    k_pksk_to_planes       71                         0      0
    k_pk_digits            60                         0      0
    k_pk_mfma<1>           80                         0      0
    k_pk_mfma<4>          304  (accumulators: 4 x 8 x 4; one wave per SIMD, launch bound 256)
    k_pk_pack              34                      4096      0
    k_pk_unpack            10                         0      0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors

KERNELS = ("k_pksk_to_planes", "k_pk_digits", "k_pk_mfmaILi1E", "k_pk_mfmaILi4E", "k_pk_pack", "k_pk_unpack")


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "compress.hip"), tmp_path_factory.mktemp("compress"))
    for name, f in sorted(d.items()):
        print(name, {k: v for k, v in f.items() if "vgpr" in k or "agpr" in k or "segment" in k})
    return d


def one(desc, name):
    ks = [v for k, v in desc.items() if name in k]
    assert len(ks) == 1, f"{name} not found in compress.hip"
    return ks[0]


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch(desc, name):
    assert one(desc, name)["private_segment_fixed_size"] == 0, "scratch spill"


@pytest.mark.parametrize("name", KERNELS)
def test_lds_bound(desc, name):
    bound = 4096 if name == "k_pk_pack" else 0
    assert one(desc, name)["group_segment_fixed_size"] <= bound, f"{one(desc, name)['group_segment_fixed_size']} bytes of LDS"
