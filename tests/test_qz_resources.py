"""Occupancy guard for k_blind_rotate_qz (CPU: compiles br_qy.hip for gfx950 and reads the code-object
descriptor, as test_kernel_resources.py does for the other kernels): two workgroups per CU need at most
256 registers a lane and half the LDS, and a spill in the CMUX loop is not acceptable."""
import os
import shutil

import pytest

from test_kernel_resources import CSRC, HIPCC, descriptors


@pytest.mark.skipif(not shutil.which(HIPCC) and not os.path.exists(HIPCC), reason="hipcc not available")
def test_qz_occupancy(tmp_path):
    d = descriptors(os.path.join(CSRC, "br_qy.hip"), tmp_path, ("-mllvm", "-amdgpu-sched-strategy=max-memory-clause"))
    ks = [v for k, v in d.items() if "k_blind_rotate_qzE" in k]
    assert len(ks) == 1, "k_blind_rotate_qz not found in br_qy.hip"
    f = ks[0]
    assert max(f["next_free_vgpr"], f["accum_offset"]) <= 256, f"{f['next_free_vgpr']} registers: one workgroup per CU"
    assert f["private_segment_fixed_size"] == 0, "scratch spill"
    assert 2 * f["group_segment_fixed_size"] <= 160 * 1024, "LDS: one workgroup per CU"
