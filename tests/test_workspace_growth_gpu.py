"""The context's workspaces across their growth points, on one context and one key.

Every workspace of fhe_ctx is a DeviceBuf (csrc/device_buf.h) grown behind a wait on the stream.  Batches of
8, 300, 1100 and 8 raw bootstraps at n = 16 cross the 256-row floor of d_ms and of the stage buffers (300) and
the 1024 floor of the keyswitch workspace (1100, which also takes the throughput kernel); 70 more lookup
tables cross the 64-table floor of d_luts.  A buffer regrown at the wrong size, freed while the stream reads
it, or kept under a stale capacity shows as a word that differs from the oracle's.  The compression
workspaces (256 blocks each) are crossed the same way under the smallest compression set.

All comparisons are exact equality of 64-bit words.  Allocation failures are tools/device_buf_host_check.cpp's
(tests/test_device_buf.py), not made to happen here.
"""
import numpy as np
import pytest

import compress_ref as R
import seeded_key_ref as K
from fhe_sign import Context
from lwe_dims import CLASSIC, product_params
from test_compress_gpu import SEED as COMP_SEED
from test_compress_gpu import Env as CompEnv
from test_lwe_dims_gpu import _keys, _rekey_checks
from test_pbs_gpu import _luts

pytestmark = pytest.mark.gpu


def test_pbs_workspaces_regrow_with_the_same_words():
    tables = _luts()
    _, sk, ok = _keys(16, CLASSIC)
    ctx = Context(0)
    try:
        ctx.set_server_key(sk)
        ids = np.array([ctx.lut(t) for t in tables], np.uint32)
        # _rekey_checks: keyswitch words on both kernels and the bootstraps' words against the oracle; its
        # inputs are 12 fixed encryptions tiled to the count, so rows 0-7 are the same in every batch
        first = _rekey_checks(ctx, ok, ids, tables, 8, 8, "8 rows, fresh workspaces")
        assert first.shape == (8, 2049)
        grown = _rekey_checks(ctx, ok, ids, tables, 300, 300, "300 rows: d_ms and stage past 256")
        assert np.array_equal(grown[:8], first)
        # 5 tables so far; 70 more distinct ones: d_luts past its 64-table floor, regrown with all 75
        # (entries 0 and 1 tell them apart, entry 2 = 15 from the five above)
        more = [ctx.lut([j % 16, j // 16] + [(7 * m + 1) % 16 for m in range(2, 16)]) for j in range(70)]
        assert more == list(range(len(tables), len(tables) + 70))
        assert [ctx.lut(t) for t in tables] == list(ids)
        again = _rekey_checks(ctx, ok, ids, tables, 8, 8, "8 rows after d_luts regrew")
        assert np.array_equal(again, first)
        big = _rekey_checks(ctx, ok, ids, tables, 1100, 1100, "1100 rows: keyswitch workspace past 1024")
        assert np.array_equal(big[:8], first)
        last = _rekey_checks(ctx, ok, ids, tables, 8, 8, "8 rows in the grown workspaces")
        assert np.array_equal(last, first)
    finally:
        ctx.close()


def test_compression_workspaces_regrow_with_the_same_words():
    """compress and decompress 8, 300 and 8 blocks under SMALL_A (k' N' = 8): the packing and the decompression
    workspaces start at 256 blocks and regrow at 300"""
    cp = R.SMALL_A
    kn = cp.k * cp.N
    env = CompEnv(cp, product_params(kn))
    try:
        env.use()
        ok = K.rekeyed_oracle(COMP_SEED, kn, 1, np.zeros(R.N_BIG * 5 * (kn + 1), np.uint64), env.key.export()[1])
        vals = [(5 * i + 3) % 16 for i in range(300)]
        cts = env.ck.encrypt_blocks(vals)
        outs = []
        for B in (8, 300, 8):
            x = env.raw(cts[:B], 15)
            lst = x.compress()
            blob = lst.serialize()
            assert blob == env.host(x, lst).serialize(), f"{B} blocks: GPU list differs from the host's"
            want_rows = R.extract_rows(cp, R.parse_list(cp, blob)[3])
            assert np.array_equal(lst.extract_rows(), want_rows)
            got = lst.decompress().export()
            assert np.array_equal(got, R.oracle_decompress(ok, want_rows)), f"{B} blocks: decompressed words"
            assert [env.ck.decrypt_block(c) for c in got] == vals[:B]
            outs.append(got)
        assert np.array_equal(outs[0], outs[2])
    finally:
        env.close()
