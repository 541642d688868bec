"""k_blind_rotate_qz (FHE_BR_QZ = 9) with every CU holding two workgroups at once: the kernel's LDS (four
polynomial regions, the zeta and twiddle tables and the lane-ordered table of the inverse-A twiddles) is
sized so that exactly two workgroups fit a CU, and a batch of 1026 bootstraps is 513 workgroups -- two on
each of the 256 CUs and one slot refilled.  Word for word against k_blind_rotate_qy (kind 4, which has no
such table) at n = 834, and rows 0, 1 and 1025 against the oracle.  Exact equality of 64-bit words."""
import numpy as np
import pytest

import oracle
from fhe_sign import Context, generate_keys
from test_keyswitch_gpu import _assert_words
from test_pbs_gpu import _luts

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
QY, AUTO, QZ = 4, 7, 9
B = 1026


def test_two_resident_workgroups_per_cu_equal_qy_and_oracle():
    ck, sk = generate_keys(seed=SEED)
    ok = oracle.OracleKeys(SEED)
    ctx = Context(0)
    ctx.set_server_key(sk)
    try:
        tables = _luts()
        ids = np.array([ctx.lut(t) for t in tables], np.uint32)
        r = ok.rng(1026)
        cts = np.stack([ok.encrypt(r, (5 * i + 3) % 16) for i in range(B)])
        lut_of = (np.arange(B) % len(tables)).astype(np.uint32)
        rows = np.array([0, 1, B - 1])
        ref = ok.pbs_batch(np.ascontiguousarray(cts[rows]), np.stack([ok.make_lut(t) for t in tables]), lut_of[rows])
        got = {}
        ctx.set_wide_threshold(0)
        for kind in (QY, QZ):
            ctx.set_br_kernel(kind)
            got[kind] = ctx.pbs(cts, ids[lut_of])
        _assert_words(got[QZ], got[QY], f"kind 9 against kind 4, batch of {B}")
        _assert_words(got[QZ][rows], ref, f"kind 9, rows 0, 1, {B - 1} of {B} against the oracle")
        assert [ok.decrypt(o) for o in got[QZ][rows]] == [tables[lut_of[i]][(5 * i + 3) % 16] for i in rows]
    finally:
        ctx.close()
