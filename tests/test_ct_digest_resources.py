"""Resource guard for the ciphertext digest kernel (CPU: compiles ct_digest.hip for gfx950 and reads the
code-object descriptor, as test_rerandomize_resources.py does).  k_ct_digest may not spill to scratch -- the 8
state words, the 16-word schedule window and the 16 prefetched words of the next block must all stay in
registers -- and may hold at most 40,960 bytes of LDS, a quarter of a CU's 160 KB: it stages 2 KB of leaf digests
and 256 bytes of node digests.  As built (hipcc -O3, gfx950):

    kernel         registers (next_free_vgpr)  LDS      scratch
    k_ct_digest      94                         2304     0
"""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = descriptors(os.path.join(CSRC, "ct_digest.hip"), tmp_path_factory.mktemp("ct_digest"))
    ks = [v for k, v in d.items() if "k_ct_digest" in k]
    assert len(ks) == 1, "k_ct_digest not found in ct_digest.hip"
    print({k: v for k, v in ks[0].items() if "vgpr" in k or "agpr" in k or "segment" in k})
    return ks[0]


def test_no_scratch(desc):
    assert desc["private_segment_fixed_size"] == 0, "scratch spill"


def test_lds_bound(desc):
    assert desc["group_segment_fixed_size"] <= 40960, f"{desc['group_segment_fixed_size']} bytes of LDS"
