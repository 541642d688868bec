"""Host definitions of the ciphertext digests and the re-randomization context (csrc/ct_digest.cpp:
fhe_ct_digest_host, fhe_ct_value_digest_host, fhe_rerand_context_*) against their restatement in hashlib
(tests/ct_digest_ref.py), byte for byte.  No GPU: tests/test_ct_digest_gpu.py pins the kernel to the host
definition."""
import ctypes as C

import numpy as np
import pytest

import ct_digest_ref as ref
from fhe_sign import ReRandomizationContext, ct_digest_host, ct_value_digest_host
from fhe_sign._lib import FheError, load, ptr

ROW = 2049


def _hex(d):
    return bytes(d).hex()


def test_known_answers():
    got = ct_digest_host(np.stack([np.zeros(ROW, np.uint64), ref.ramp_row()]))
    assert _hex(got[0]) == ref.ZERO_ROW_DIGEST
    assert _hex(got[1]) == ref.RAMP_ROW_DIGEST
    # the reference itself gives the pinned bytes
    assert ref.row_digest(np.zeros(ROW, np.uint64)).hex() == ref.ZERO_ROW_DIGEST
    assert ref.row_digest(ref.ramp_row()).hex() == ref.RAMP_ROW_DIGEST


def test_all_ones_row():
    row = np.full(ROW, 2**64 - 1, np.uint64)
    assert _hex(ct_digest_host(row)[0]) == ref.row_digest(row).hex()


@pytest.mark.parametrize("n", [1, 2, 65])
def test_random_rows(n):
    rows = np.random.default_rng(0xC7D1 + n).integers(0, 2**64, (n, ROW), dtype=np.uint64)
    got = ct_digest_host(rows)
    assert got.shape == (n, 32)
    assert np.array_equal(got, ref.rows_digest(rows))
    assert len({_hex(d) for d in got}) == n


def test_zero_rows():
    assert ct_digest_host(np.zeros((0, ROW), np.uint64)).shape == (0, 32)


@pytest.mark.parametrize("word", ref.FLIP_WORDS)
def test_one_bit_flip_changes_the_digest_to_the_reference(word):
    base = ref.ramp_row()
    flipped = base.copy()
    flipped[word] ^= np.uint64(1) << np.uint64(word % 64)
    got = ct_digest_host(np.stack([base, flipped]))
    assert _hex(got[0]) == ref.RAMP_ROW_DIGEST
    assert _hex(got[1]) == ref.row_digest(flipped).hex() != ref.RAMP_ROW_DIGEST


def _blocks(n, seed):
    rng = np.random.default_rng(seed)
    tags = rng.integers(0, 2, n).astype(np.uint8)
    degrees = rng.integers(0, 16, n).astype(np.uint32)
    noises = rng.integers(0, 26, n).astype(np.uint32)
    rd = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    return tags, degrees, noises, rd


@pytest.mark.parametrize("kind,bits,n", [(0, 2, 1), (0, 64, 32), (1, 96, 48), (1, 0, 0), (0, 4096, 2048)])
def test_value_digest(kind, bits, n):
    tags, degrees, noises, rd = _blocks(n, 0xD16 + n)
    want = ref.value_digest(kind, bits, [(int(t), int(d), int(s), r.tobytes()) for t, d, s, r in zip(tags, degrees, noises, rd)])
    assert ct_value_digest_host(kind, bits, tags, degrees, noises, rd) == want


def test_value_digest_separates_its_fields():
    tags, degrees, noises, rd = _blocks(4, 7)
    base = ct_value_digest_host(0, 8, tags, degrees, noises, rd)
    assert ct_value_digest_host(1, 8, tags, degrees, noises, rd) != base
    assert ct_value_digest_host(0, 10, tags, degrees, noises, rd) != base
    assert ct_value_digest_host(0, 8, tags ^ 1, degrees, noises, rd) != base
    assert ct_value_digest_host(0, 8, tags, degrees + 1, noises, rd) != base
    assert ct_value_digest_host(0, 8, tags, degrees, noises + 1, rd) != base
    assert ct_value_digest_host(0, 8, tags, degrees, noises, rd[::-1]) != base


def test_context_seeds():
    d1, d2 = bytes(range(32)), bytes(range(100, 132))
    for domain in (b"", b"sign/v1", bytes(300)):
        rc = ReRandomizationContext(domain).add_bytes(b"request 17").add_digest(d1).add_bytes(b"").add_digest(d2)
        r = ref.Context(domain).add_bytes(b"request 17").add_digest(d1).add_bytes(b"").add_digest(d2)
        for i in (0, 1, 2**40 + 3, 2**64 - 1):
            assert rc.seed(i) == r.seed(i)
        assert rc.seed(0) == r.seed(0)  # asking again gives the same seed
        assert len({rc.seed(i) for i in range(8)}) == 8
    assert ReRandomizationContext(b"x").seed(0) == ref.Context(b"x").seed(0)  # nothing added


def test_context_framing_splits_one_way():
    d = bytes(range(32))
    seeds = {
        ReRandomizationContext(b"ab").add_bytes(b"c").seed(0),
        ReRandomizationContext(b"a").add_bytes(b"bc").seed(0),
        ReRandomizationContext(b"a").add_bytes(b"b").add_bytes(b"c").seed(0),
        ReRandomizationContext(b"a").add_bytes(d).seed(0),  # the same 32 bytes as caller bytes ...
        ReRandomizationContext(b"a").add_digest(d).seed(0),  # ... and as a digest
    }
    assert len(seeds) == 5


def test_item_order_matters():
    d1, d2 = bytes(range(32)), bytes(range(1, 33))
    a = ReRandomizationContext(b"dom").add_digest(d1).add_digest(d2)
    b = ReRandomizationContext(b"dom").add_digest(d2).add_digest(d1)
    assert a.seed(0) != b.seed(0)
    assert a.seed(0) == ref.Context(b"dom").add_digest(d1).add_digest(d2).seed(0)
    assert b.seed(0) == ref.Context(b"dom").add_digest(d2).add_digest(d1).seed(0)
    c = ReRandomizationContext(b"dom").add_bytes(b"x").add_digest(d1)
    e = ReRandomizationContext(b"dom").add_digest(d1).add_bytes(b"x")
    assert c.seed(0) != e.seed(0)


def test_add_after_seed_is_refused():
    rc = ReRandomizationContext(b"dom").add_bytes(b"x")
    s0 = rc.seed(0)
    with pytest.raises(FheError, match="seed") as e:
        rc.add_bytes(b"y")
    assert e.value.code == -1
    with pytest.raises(FheError, match="seed") as e:
        rc.add_digest(bytes(32))
    assert e.value.code == -1
    assert rc.seed(0) == s0 and rc.seed(1) != s0  # the refused adds changed nothing
    # the device adds check it before they look at the context or the operand's blocks
    lib = load()
    assert lib.fhe_rerand_context_add_radix(None, rc._h, C.c_void_p(1)) == -1
    assert b"seed" in lib.fhe_last_error()
    assert lib.fhe_rerand_context_add_biguint(None, rc._h, C.c_void_p(1)) == -1


def test_null_and_oversized_arguments_are_refused():
    lib = load()
    rows = np.zeros((1, ROW), np.uint64)
    out = np.zeros(32, np.uint8)
    o8 = ptr(out, C.c_uint8)
    assert lib.fhe_ct_digest_host(None, 1, o8) == -1
    assert b"fhe_ct_digest_host" in lib.fhe_last_error()
    assert lib.fhe_ct_digest_host(ptr(rows), 1, None) == -1
    assert lib.fhe_ct_digest_host(None, 0, None) == 0
    assert lib.fhe_ct_digest_host(ptr(rows), (1 << 24) + 1, o8) == -1
    assert b"2^24" in lib.fhe_last_error()
    assert not out.any()
    tags, deg, noi = np.ones(1, np.uint8), np.ones(1, np.uint32), np.ones(1, np.uint32)
    args = [ptr(tags, C.c_uint8), ptr(deg, C.c_uint32), ptr(noi, C.c_uint32), o8]
    for k in range(4):
        a = list(args)
        a[k] = None
        assert lib.fhe_ct_value_digest_host(0, 2, *a, 1, o8) == -1, k
        assert b"fhe_ct_value_digest_host" in lib.fhe_last_error()
    assert lib.fhe_ct_value_digest_host(0, 2, *args, 1, None) == -1
    assert lib.fhe_ct_value_digest_host(0, 0, None, None, None, None, 0, o8) == 0
    out[:] = 0
    assert lib.fhe_ct_value_digest_host(0, 2, *args, (1 << 24) + 1, o8) == -1
    assert lib.fhe_ct_value_digest_host(2, 2, *args, 1, o8) == -1  # kind
    tags[0] = 2
    assert lib.fhe_ct_value_digest_host(0, 2, *args, 1, o8) == -1  # tag
    assert not out.any()
    h = C.c_void_p()
    assert lib.fhe_rerand_context_new(None, 1, C.byref(h)) == -1
    assert b"fhe_rerand_context_new" in lib.fhe_last_error()
    assert lib.fhe_rerand_context_new(b"d", 1, None) == -1
    assert lib.fhe_rerand_context_new(None, 0, C.byref(h)) == 0 and h.value
    assert lib.fhe_rerand_context_add_bytes(None, b"x", 1) == -1
    assert lib.fhe_rerand_context_add_bytes(h, None, 1) == -1
    assert b"fhe_rerand_context_add_bytes" in lib.fhe_last_error()
    assert lib.fhe_rerand_context_add_bytes(h, None, 0) == 0
    assert lib.fhe_rerand_context_add_digest(None, bytes(32)) == -1
    assert lib.fhe_rerand_context_add_digest(h, None) == -1
    assert b"fhe_rerand_context_add_digest" in lib.fhe_last_error()
    assert lib.fhe_rerand_context_seed(None, 0, o8) == -1
    assert lib.fhe_rerand_context_seed(h, 0, None) == -1
    assert b"fhe_rerand_context_seed" in lib.fhe_last_error()
    assert lib.fhe_rerand_context_add_radix(None, None, None) == -1
    assert lib.fhe_rerand_context_add_biguint(None, h, None) == -1
    assert lib.fhe_rerand_context_add_radix(None, h, C.c_void_p(1)) == -1  # no context
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_radix_digest(None, None, o8) == -1
    assert lib.fhe_biguint_digest(None, None, o8) == -1
    assert lib.fhe_ct_digest_rows(None, ptr(rows), 1, o8) == -1
    assert lib.fhe_ct_digest_rows(None, None, 1, o8) == -1
    assert lib.fhe_ct_digest_rows(None, ptr(rows), (1 << 24) + 1, o8) == -1
    ms = C.c_float()
    assert lib.fhe_ctx_time_ct_digest(None, 1, 1, C.byref(ms)) == -1
    assert lib.fhe_schnorr_sign_fhe_with_k0_rerand(None, None, None, 0, None, None, None, 0, None, 0, None) == -1
    # still usable after the refusals: the seed of (empty domain, one empty bytes item)
    assert lib.fhe_rerand_context_seed(h, 0, o8) == 0
    assert out.tobytes() == ref.Context(b"").add_bytes(b"").seed(0)
    lib.fhe_rerand_context_destroy(h)
    lib.fhe_rerand_context_destroy(None)
