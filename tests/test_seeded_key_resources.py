"""Resource guard for the seeded server key's install kernels (CPU: compiles seeded_key.hip for gfx950 and
reads the code-object descriptors, as test_qz_resources.py does): neither kernel may spill to scratch, and
k_expand_bsk_fourier -- one wave per polynomial, a 16 KB staging copy of the generated mask polynomial next
to the transform's 17 KB exchange buffer -- must keep its LDS at or below 40 KB so that four of its waves
still fit a CU."""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors


@pytest.fixture(scope="module")
def desc(tmp_path_factory):
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return descriptors(os.path.join(CSRC, "seeded_key.hip"), tmp_path_factory.mktemp("seeded_key"))


def one(desc, name):
    ks = [v for k, v in desc.items() if name in k]
    assert len(ks) == 1, f"{name} not found in seeded_key.hip"
    return ks[0]


def test_expand_ksk_has_no_scratch(desc):
    assert one(desc, "k_expand_ksk")["private_segment_fixed_size"] == 0, "scratch spill"


def test_expand_bsk_fourier_has_no_scratch_and_fits_several_waves(desc):
    f = one(desc, "k_expand_bsk_fourier")
    assert f["private_segment_fixed_size"] == 0, "scratch spill"
    assert f["group_segment_fixed_size"] <= 40 * 1024, f"{f['group_segment_fixed_size']} bytes of LDS"
