"""k_blind_rotate_qz's lane-ordered table of the inverse-A twiddles on the CPU (tools/qz_emulate.py, a
transcription of the prologue's fill and the CMUX loop's reads): each lane reads the W entries it loaded
from global memory every step before the table existed, the reads are conflict-free, and the table's
size and place parsed from br_qy.hip still leave room for two workgroups on a CU."""
import os
import re
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import qz_emulate as Q  # noqa: E402
from lds_layout_qx import RG  # noqa: E402

LDS_PER_CU = 163840


def _kernel_constants():
    """the qz kernel's LDS sizes and offsets (complex entries), evaluated from the constexpr lines of br_qy.hip"""
    src = open(os.path.join(ROOT, "fhe-sign_amd", "csrc", "br_qy.hip")).read()
    body = src[src.index("void k_blind_rotate_qz("):]
    body = body[:body.index("\n}\n")]
    env = {"NC": 2, "ZR_SZ": Q.ZR_SZ}
    for text, names in ((src, ("ZZ_SZ", "ZT_SZ", "ZW_SZ")), (body, ("ZL_Z", "ZL_T", "ZL_W"))):
        for name in names:
            m = re.search(r"constexpr int [^;]*\b%s = ([A-Z_0-9a-z *+]+)[,;]" % name, text)
            assert m, name
            env[name] = eval(m.group(1), {"__builtins__": {}}, env)
    m = re.search(r"cplx s_lds\[([A-Z_ +]+)\];", body)
    assert m, "s_lds"
    env["LDS"] = eval(m.group(1), {"__builtins__": {}}, env)
    assert re.search(r"cplx\* s_w = s_lds \+ ZL_W;", body)
    return env


def test_every_lane_reads_the_w_entries_it_loaded_before():
    idx = Q.lane_twiddle_indices()
    assert idx.min() >= 0, "an entry of the table is never written"
    for L in range(64):
        v = Q.idx_zA(L, 0)
        want = [8 * v, 4 * v, 2 * v, 2 * v + 128, v, v + 64, v + 128, v + 192]
        assert [idx[Q.lane_twiddle_read(k, L)] for k in range(8)] == want, L
    assert 0 <= idx.min() and idx.max() < 512  # inside W (fft_tables: 512 entries)
    assert len(Q.W) >= 512


def test_reads_are_conflict_free():
    """ds_read_b128: four 16-lane groups, bank = 16-byte slot mod 16"""
    k = _kernel_constants()
    for row in range(8):
        pos = np.array([k["ZL_W"] + Q.lane_twiddle_read(row, L) for L in range(64)])
        for g in RG:
            assert np.bincount(pos[g] % 16, minlength=16).max() == 1, (row, g)
    assert Q.twiddle_table_conflicts() == 0


def test_size_and_offset_are_the_kernels():
    k = _kernel_constants()
    assert k["ZW_SZ"] == Q.ZW_SZ == 8 * 64
    assert (k["ZZ_SZ"], k["ZT_SZ"]) == (Q.ZZ_SZ, Q.ZT_SZ)
    assert k["ZL_W"] == Q.ZL_W == k["ZL_T"] + k["ZT_SZ"]  # directly behind s_t, nothing overlaps
    assert k["ZL_T"] == k["ZL_Z"] + k["ZZ_SZ"] and k["ZL_Z"] == 4 * Q.ZR_SZ
    assert k["LDS"] == k["ZL_W"] + k["ZW_SZ"]  # the table ends the allocation: the last read stays inside
    assert max(Q.lane_twiddle_read(r, L) for r in range(8) for L in range(64)) == k["ZW_SZ"] - 1
    assert (16 * k["ZL_W"]) % 16 == 0


def test_two_workgroups_fit_a_cu():
    k = _kernel_constants()
    assert 16 * k["LDS"] == Q.LDS_BYTES == 81280
    assert 2 * 16 * k["LDS"] <= LDS_PER_CU
