"""Resident client key, the host side (CPU): the definitions the device kernels are held against,
and the refusals that need no device.

Addressing.  ClientKey.encrypt_rows_indexed_host restates encrypt_blocks from counter-indexed ChaCha blocks through
csrc/client_ops_index.h, the arithmetic client_ops.hip runs: block i of a batch that starts at u64 stream word W0
is the 257 ChaCha blocks from (W0 + 2049 i) / 8 on, entered (W0 + i) mod 8 words in.  On twin keys (one key,
deserialized twice, seed_encryption(42, 100)) the rows and the serialized client keys -- encryption-stream state
included -- must be equal, at block counts 1, 2, 7, 8, 9, 65, 129 and W0 = 0, 3, 2049 + 5.  With 8 or more rows
every offset 0 .. 7 starts a row and, as a row is 2049 = 1 mod 8 words, ends one; W0 = 3 and 2054 move which.

Phases.  ClientKey.decrypt_phase_host against numpy on the exported key, uint64 wrap arithmetic.

Refusals.  NULL arguments and a simulated context, for every new entry point.  The two refusals that need an
installed server key to be told apart from "no device" (no server key: FHE_ERR_NO_KEY; parameters that differ:
FHE_ERR_INVALID) are in tests/test_client_ops_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from fhe_sign import ClientKey, CompressedFheUint, SimContext, _lib, generate_keys, set_server_key
from lwe_dims import product_params

BIG = 2049
COUNTS = [1, 2, 7, 8, 9, 65, 129]
W0S = [0, 3, 2049 + 5]
FHE_ERR_INVALID = -1


@pytest.fixture(scope="module")
def key_bytes():
    ck, _ = generate_keys(product_params(16), seed=0xC11E)
    return ck.serialize()


def advance(ck, w0):
    """move the encryption stream w0 u64 words on: a full block is 2049 words, a seeded block one"""
    if w0 >= BIG:
        ck.encrypt_block(1)
        w0 -= BIG
    if w0:
        CompressedFheUint.try_encrypt(0, ck, bits=2 * w0, seed=bytes(range(32)))


def twins(key_bytes, w0):
    out = []
    for _ in range(2):
        ck = ClientKey.deserialize(key_bytes)
        ck.seed_encryption(42, 100)
        advance(ck, w0)
        out.append(ck)
    assert out[0].serialize() == out[1].serialize()
    return out


@pytest.mark.parametrize("w0", W0S)
@pytest.mark.parametrize("count", COUNTS)
def test_indexed_rows_equal_encrypt_blocks(key_bytes, count, w0):
    a, b = twins(key_bytes, w0)
    values = (np.arange(count, dtype=np.uint64) * 7 + 3) % 16
    want = a.encrypt_blocks(values)
    got = b.encrypt_rows_indexed_host(values)
    bad = np.argwhere(want != got)
    assert bad.size == 0, f"first differing (row, word): {bad[0]} of {len(bad)}"
    assert a.serialize() == b.serialize()
    # and what follows on the stream is the same
    assert np.array_equal(a.encrypt_blocks([5]), b.encrypt_blocks([5]))


def test_indexed_rows_decrypt(key_bytes):
    (ck,) = twins(key_bytes, 3)[:1]
    values = np.arange(40, dtype=np.uint64) % 16
    rows = ck.encrypt_rows_indexed_host(values)
    assert [ck.decrypt_block(r) for r in rows] == [int(v) for v in values]


def test_phase_host_equals_numpy(key_bytes):
    ck = ClientKey.deserialize(key_bytes)
    _, glwe = ck.export()
    assert glwe.size == 2048 and set(np.unique(glwe)) <= {0, 1}
    rng = np.random.default_rng(0x9A5E)
    rows = np.concatenate([ck.encrypt_blocks(np.arange(16, dtype=np.uint64)),
                           rng.integers(0, 1 << 64, size=(9, BIG), dtype=np.uint64)])
    want = rows[:, 2048] - (rows[:, :2048] * glwe[None, :]).sum(axis=1, dtype=np.uint64)
    got = ck.decrypt_phase_host(rows)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    # the phase is what decrypt_block decodes: (phase + delta / 2) / delta mod 16 at the default moduli
    delta = 1 << 59
    assert [((int(p) + delta // 2) % (1 << 64)) // delta % 16 for p in got[:16]] == list(range(16))


def test_null_arguments(key_bytes):
    lib = _lib.load()
    ck = ClientKey.deserialize(key_bytes)
    one = np.zeros(1, np.uint64)
    row = np.zeros(BIG, np.uint64)
    r, a, b = C.c_int(), C.c_uint64(), C.c_uint64()
    f, g = C.c_float(), C.c_float()
    assert lib.fhe_ctx_set_client_key(None, ck.handle) == FHE_ERR_INVALID
    assert lib.fhe_ctx_clear_client_key(None) == FHE_ERR_INVALID
    assert lib.fhe_ctx_client_ops_info(None, C.byref(r), C.byref(a), C.byref(b)) == FHE_ERR_INVALID
    assert lib.fhe_client_encrypt_rows(None, ck.handle, _lib.ptr(one), 1, _lib.ptr(row)) == FHE_ERR_INVALID
    assert lib.fhe_client_phase_rows(None, _lib.ptr(row), 1, _lib.ptr(one)) == FHE_ERR_INVALID
    assert lib.fhe_ctx_time_client_ops(None, 1, 1, C.byref(f), C.byref(g)) == FHE_ERR_INVALID
    assert lib.fhe_client_encrypt_rows_indexed_host(None, _lib.ptr(one), 1, _lib.ptr(row)) == FHE_ERR_INVALID
    assert lib.fhe_client_encrypt_rows_indexed_host(ck.handle, None, 1, _lib.ptr(row)) == FHE_ERR_INVALID
    assert lib.fhe_client_encrypt_rows_indexed_host(ck.handle, _lib.ptr(one), 1, None) == FHE_ERR_INVALID
    assert lib.fhe_decrypt_phase_host(None, _lib.ptr(row), 1, _lib.ptr(one)) == FHE_ERR_INVALID
    assert lib.fhe_decrypt_phase_host(ck.handle, None, 1, _lib.ptr(one)) == FHE_ERR_INVALID
    assert lib.fhe_decrypt_phase_host(ck.handle, _lib.ptr(row), 1, None) == FHE_ERR_INVALID
    # nothing to do is not an error, and a block value off the message space is
    assert lib.fhe_client_encrypt_rows_indexed_host(ck.handle, None, 0, None) == 0
    assert lib.fhe_decrypt_phase_host(ck.handle, None, 0, None) == 0
    before = ck.serialize()
    one[0] = 16
    assert lib.fhe_client_encrypt_rows_indexed_host(ck.handle, _lib.ptr(one), 1, _lib.ptr(row)) == FHE_ERR_INVALID
    assert ck.serialize() == before  # refused before the stream moved


def test_simulated_context_refuses(key_bytes):
    lib = _lib.load()
    ck = ClientKey.deserialize(key_bytes)
    ctx = SimContext()
    set_server_key(ctx)
    try:
        one = np.zeros(1, np.uint64)
        row = np.zeros(BIG, np.uint64)
        r, a, b = C.c_int(), C.c_uint64(), C.c_uint64()
        f, g = C.c_float(), C.c_float()
        for rc in (lib.fhe_ctx_set_client_key(ctx.handle, ck.handle),
                   lib.fhe_ctx_clear_client_key(ctx.handle),
                   lib.fhe_ctx_client_ops_info(ctx.handle, C.byref(r), C.byref(a), C.byref(b)),
                   lib.fhe_client_encrypt_rows(ctx.handle, ck.handle, _lib.ptr(one), 1, _lib.ptr(row)),
                   lib.fhe_client_phase_rows(ctx.handle, _lib.ptr(row), 1, _lib.ptr(one)),
                   lib.fhe_ctx_time_client_ops(ctx.handle, 1, 1, C.byref(f), C.byref(g))):
            assert rc == FHE_ERR_INVALID
            assert b"simulated context" in lib.fhe_last_error()
    finally:
        set_server_key(None)
        ctx.close()
