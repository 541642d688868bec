"""Re-randomization under the compact public key on the host: fhe_rerandomize_host, the word-for-word
definition of the GPU kernels (include/fhe_rocm.h "re-randomization under the public key", csrc/rerandomize.cpp),
against tests/rerandomize_ref.py, a numpy restatement on public_key_ref's own RFC 8439.  No GPU, no context.

The phase bound is derived, not measured: the added error is E R + E2 - E1 S with R and S binary and every noise
word in [-2^17, 2^17], so |error| <= 2048 2^17 + 2^17 + 2048 2^17 < 2^30."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import public_key_ref as pkref
import rerandomize_ref as ref
from fhe_sign import (CompactCiphertextList, CompactPublicKey, generate_keys, rerandomization_seed, rerandomize_host,
                      rerandomize_zero_host)
from fhe_sign._lib import FheError, load, ptr

SEED = 0x5EED12
MASK_SEED = bytes(range(17, 49))
RR_SEED = bytes(range(101, 133))
OTHER_SEED = bytes(range(102, 134))
N = pkref.N
# t = 0, 1, 2046, 2047 and the second chunk's first coefficient; 4097 reaches a third chunk
SIZES = [1, 2, 128, 2047, 2048, 2049, 4097]


@pytest.fixture(scope="module")
def keys():
    ck, _ = generate_keys(seed=SEED)
    sk = ck.export()[1]
    pk = CompactPublicKey.new(ck, seed=MASK_SEED)
    return ck, sk, pk


@pytest.fixture(scope="module")
def reference(keys):
    """the restatement's zero encryptions of every size, computed once"""
    _, _, pk = keys
    body = pk.export()[1]
    return {n: ref.zero(MASK_SEED, body, RR_SEED, n) for n in SIZES}


def _rows(n, salt=0):
    """any words do: the definition is linear in the input"""
    return np.random.default_rng(1000 + n + salt).integers(0, 1 << 64, (n, N + 1), dtype=np.uint64)


@pytest.mark.parametrize("n", SIZES)
def test_zero_encryptions_and_rows_equal_the_definition(keys, reference, n):
    _, _, pk = keys
    za, zb = rerandomize_zero_host(pk, RR_SEED, n)
    want_a, want_b = reference[n]
    assert np.array_equal(za, want_a)
    assert np.array_equal(zb, want_b)
    rows = _rows(n)
    out = rerandomize_host(pk, RR_SEED, rows)
    assert np.array_equal(out, ref.apply(want_a, want_b, rows))
    assert not np.array_equal(out[:, :N], rows[:, :N])


def test_trivial_rows(keys, reference):
    """a trivial block enters as mask 0, body delta value: the output is the extraction itself plus the body"""
    _, _, pk = keys
    n = 128
    rows = np.zeros((n, N + 1), np.uint64)
    rows[:, N] = (np.arange(n, dtype=np.uint64) % np.uint64(16)) * np.uint64(pkref.DELTA)
    out = rerandomize_host(pk, RR_SEED, rows)
    za, zb = reference[n]
    assert np.array_equal(out, ref.apply(za, zb, rows))
    assert np.array_equal(out[0, :N], np.append(za[0, :1], np.uint64(0) - za[0, :0:-1]))
    assert np.array_equal(out[:, N] - rows[:, N], zb)


def test_no_blocks_is_a_no_op(keys):
    _, _, pk = keys
    out = rerandomize_host(pk, RR_SEED, np.zeros((0, N + 1), np.uint64))
    assert out.shape == (0, N + 1)
    assert load().fhe_rerandomize_host(pk.handle, RR_SEED, None, 0) == 0
    za, zb = rerandomize_zero_host(pk, RR_SEED, 0)
    assert za.size == 0 and zb.size == 0


def test_determinism_and_separation(keys):
    _, _, pk = keys
    n = 130
    rows = _rows(n)
    a, b = rerandomize_host(pk, RR_SEED, rows), rerandomize_host(pk, RR_SEED, rows)
    assert np.array_equal(a, b)
    other = rerandomize_host(pk, OTHER_SEED, rows)
    assert not np.array_equal(a[:, :N], other[:, :N])
    assert not np.array_equal(rerandomize_zero_host(pk, RR_SEED, n)[0], rerandomize_zero_host(pk, OTHER_SEED, n)[0])
    # a compact list of zeros whose ENCRYPTION seed is the same 32 bytes: other stream ids, unrelated words
    x = CompactCiphertextList.builder(pk).push(0, bits=2 * n).build(seed=RR_SEED)
    ca, cb = x.export()
    za, zb = rerandomize_zero_host(pk, RR_SEED, n)
    assert not np.array_equal(ca, za) and not np.array_equal(cb, zb)
    assert not np.any(ca[0] == za[0])
    # ... and they are the list's words once the restatement is given the list's stream ids
    saved = ref.STREAM_BINARY, ref.STREAM_NOISE
    try:
        ref.STREAM_BINARY, ref.STREAM_NOISE = pkref.STREAM_BINARY, pkref.STREAM_NOISE
        la, lb = ref.zero(MASK_SEED, pk.export()[1], RR_SEED, n)
    finally:
        ref.STREAM_BINARY, ref.STREAM_NOISE = saved
    assert np.array_equal(ca, la) and np.array_equal(cb, lb)


def test_every_block_value_decrypts_and_the_added_error_is_below_2_30(keys):
    """one full chunk: every t of the extraction, all 16 block values"""
    ck, sk, pk = keys
    values = np.arange(N, dtype=np.uint64) % np.uint64(16)
    rows = ck.encrypt_blocks(values)
    out = rerandomize_host(pk, RR_SEED, rows)
    assert [ck.decrypt_block(r) for r in out] == [int(v) for v in values]
    before, after = pkref.phase_errors(rows, sk, values), pkref.phase_errors(out, sk, values)
    added = after - before
    print("largest added phase error: 2^%.2f" % np.log2(float(np.abs(added).max())))
    assert int(np.abs(added).max()) < 1 << 30
    assert np.abs(added).max() > 0


def test_seed_helper_is_the_tagged_sha256():
    for domain, data in [(b"", b""), (b"request", b"\x01" * 32), (b"a", b"bc"), (b"ab", b"c"), (b"x" * 200, b"y" * 300)]:
        t = hashlib.sha256(b"fhe-rocm/rerandomize").digest()
        want = hashlib.sha256(t + t + len(domain).to_bytes(8, "little") + domain + data).digest()
        assert rerandomization_seed(domain, data) == want == ref.derive_seed(domain, data)
    assert rerandomization_seed(b"a", b"bc") != rerandomization_seed(b"ab", b"c")


def test_refusals(keys):
    _, _, pk = keys
    lib = load()
    rows = np.zeros((1, N + 1), np.uint64)
    assert lib.fhe_rerandomize_host(None, RR_SEED, ptr(rows), 1) != 0
    assert lib.fhe_rerandomize_host(pk.handle, None, ptr(rows), 1) != 0
    assert lib.fhe_rerandomize_host(pk.handle, RR_SEED, None, 1) != 0
    # the count is checked before a word is touched: one row stands for the 2^24 + 1
    assert lib.fhe_rerandomize_host(pk.handle, RR_SEED, ptr(rows), (1 << 24) + 1) != 0
    assert not rows.any()
    za, zb = np.zeros(N, np.uint64), np.zeros(1, np.uint64)
    assert lib.fhe_rerandomize_zero_host(None, RR_SEED, 1, ptr(za), za.size, ptr(zb), zb.size) != 0
    assert lib.fhe_rerandomize_zero_host(pk.handle, None, 1, ptr(za), za.size, ptr(zb), zb.size) != 0
    assert lib.fhe_rerandomize_zero_host(pk.handle, RR_SEED, 1, None, 0, ptr(zb), zb.size) != 0
    assert lib.fhe_rerandomize_zero_host(pk.handle, RR_SEED, (1 << 24) + 1, ptr(za), za.size, ptr(zb), zb.size) != 0
    assert lib.fhe_rerandomize_zero_host(pk.handle, RR_SEED, 2, ptr(za), za.size, ptr(zb), zb.size) != 0  # zb too small
    out = (C.c_uint8 * 32)()
    assert lib.fhe_rerandomize_seed(None, 1, b"x", 1, out) != 0
    assert lib.fhe_rerandomize_seed(b"x", 1, None, 1, out) != 0
    assert lib.fhe_rerandomize_seed(b"x", 1, b"x", 1, None) != 0
    assert lib.fhe_set_public_key(None, pk.handle) != 0
    with pytest.raises(ValueError):
        rerandomize_host(pk, b"short", rows)
    with pytest.raises(FheError):
        rerandomize_zero_host(pk, None, 1)  # the host definition takes no NULL seed: no entropy is drawn for it
