"""Resource guard for the compact-list extraction kernel (CPU: compiles public_key.hip for gfx950 and reads
the code-object descriptor, as test_compress_resources.py does).  k_compact_extract may not spill to scratch
and may hold at most 16,384 bytes of LDS (one chunk's C_A, if it staged it; as written it stages nothing:
every word of C_A is read once per slot).  As built (hipcc -O3, gfx950):

    kernel               registers (next_free_vgpr)  LDS    scratch
    k_compact_extract      32                         0      0
(eight global_load_dwordx2, four global_store_dwordx4 and the body's global_store_dwordx2; no flat access)
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "public_key.hip"), tmp_path_factory.mktemp("public_key"))
    ks = [v for k, v in d.items() if "k_compact_extract" in k]
    assert len(ks) == 1, "k_compact_extract not found in public_key.hip"
    print({k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
    return ks[0]


def test_no_scratch(desc):
    assert desc["private_segment_fixed_size"] == 0, "scratch spill"


def test_lds_bound(desc):
    assert desc["group_segment_fixed_size"] <= 16384, f"{desc['group_segment_fixed_size']} bytes of LDS"
