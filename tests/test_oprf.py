"""Oblivious pseudo-random values on the host (CPU): fhe_oprf_rows_host and fhe_oprf_lut_host, the word-for-word
definitions of k_oprf_rows (oprf.hip) and of the accumulator, against the numpy restatement tests/oprf_ref.py;
the refusals; and the balance of the definition itself -- the values the definition assigns to 1024 rows of one
seed under the small key of key seed 0x0F0F, counted exactly.  No GPU, no context."""
import numpy as np
import pytest

import oprf_ref as O
from fhe_sign import _lib, default_params, generate_keys, ms_stride, oprf_lut_host, oprf_rows_host
from fhe_sign.core import MS_PAD_WORD

DIMS = (1, 2, 15, 16, 255, 256, 833, 834, 2048)  # n % 8 of 0, 1, 2 and 7
COUNTS = (1, 2, 63, 64, 65, 257)
SEED = bytes(range(32))
KEY_SEED = 0x0F0F
BALANCE_ROWS = 1024
# the exact counts of the definition (include/fhe_rocm.h) for SEED under KEY_SEED's small key
BALANCE = {1: [522, 502], 2: [258, 264, 241, 261]}
# binomial sigma of a count: sqrt(1024 * 1/2 * 1/2) = 16 (80 = 5 sigma), sqrt(1024 * 1/4 * 3/4) = 13.9 (64 = 4.6 sigma)
BALANCE_BOUND = {1: (512, 80), 2: (256, 64)}

_ref = {}


def ref_rows(n):
    """the reference's 257 rows at dimension n, computed once, read-only"""
    if n not in _ref:
        r = O.rows(SEED, n, max(COUNTS), O.ms_stride(n))
        r.setflags(write=False)
        _ref[n] = r
    return _ref[n]


def test_reference_constants():
    assert O.PAD == MS_PAD_WORD and O.ms_stride(834) == ms_stride(834) == 840
    p = default_params()
    assert (1 << 63) // (p.message_modulus * p.carry_modulus) == O.DELTA


@pytest.mark.parametrize("n", DIMS)
def test_rows_equal_reference(n):
    ref = ref_rows(n)
    ws = ms_stride(n)
    for count in COUNTS:
        wide = oprf_rows_host(SEED, n, count, ws)
        assert wide.shape == (count, ws)
        # row b of any call is row b of the longest one: a row starts on a ChaCha block boundary
        assert np.array_equal(wide, ref[:count]), f"n {n}, {count} rows, stride {ws}"
        assert (wide[:, n] == 0).all() and (wide[:, n + 1:] == np.uint64(MS_PAD_WORD)).all()
        tight = oprf_rows_host(SEED, n, count, n + 1)
        assert tight.shape == (count, n + 1) and np.array_equal(tight, ref[:count, :n + 1]), f"n {n}, {count} rows, stride n + 1"
    assert np.array_equal(oprf_rows_host(SEED, n, 3), ref[:3, :n + 1])  # the default stride


def test_rows_depend_on_the_seed_and_the_stream():
    a, b = oprf_rows_host(SEED, 834, 2), oprf_rows_host(bytes(range(1, 33)), 834, 2)
    assert not np.array_equal(a[:, :834], b[:, :834])
    # not the seeded ciphertexts' stream (id 101) under the same seed
    from test_seeded import ROCM, mask_key, stream_u64
    assert not np.array_equal(a[0, :834], stream_u64(mask_key(SEED), (101, ROCM, 0), 0, 834))
    # and the words are the stream's: block R b of stream 111
    assert np.array_equal(a[1, :834], stream_u64(mask_key(SEED), (111, ROCM, 0), 8 * 105, 834))


@pytest.mark.parametrize("bits", (1, 2))
def test_accumulator_equals_reference(bits):
    got = oprf_lut_host(bits)
    assert np.array_equal(got, O.lut(bits))
    p = 1 << bits
    # stairs of 2N / p coefficients... of which N are in the polynomial: odd multiples of delta / 2, no negated head
    assert [int(v) // (O.DELTA // 2) for v in got[:: 2 * O.N // p]] == [2 * k + 1 for k in range(p // 2)]
    assert int(got[0]) == O.DELTA // 2 and int(got[-1]) == (p - 1) * (O.DELTA // 2)


def test_refusals():
    lib = _lib.load()
    buf = np.zeros(4100, np.uint64)
    p = default_params()
    for bits in (0, 3):
        assert lib.fhe_oprf_lut_host(p, bits, _lib.ptr(buf)) == -1  # FHE_ERR_INVALID
        assert b"bits" in lib.fhe_last_error()
    for n, stride in ((16, 16), (0, 8), (2049, 2056)):
        assert lib.fhe_oprf_rows_host(SEED, n, 1, stride, _lib.ptr(buf)) == -1
    assert b"n must be" in lib.fhe_last_error()
    assert lib.fhe_oprf_rows_host(SEED, 16, 1, 16, _lib.ptr(buf)) == -1 and b"stride" in lib.fhe_last_error()
    assert lib.fhe_oprf_rows_host(None, 16, 1, 17, _lib.ptr(buf)) == -1
    assert not buf.any()
    assert lib.fhe_oprf_rows_host(SEED, 16, 0, 17, _lib.ptr(buf)) == 0


@pytest.fixture(scope="module")
def small_key():
    ck, _ = generate_keys(seed=KEY_SEED)
    key = ck.export()[0]
    assert key.shape == (834,) and set(np.unique(key).tolist()) == {0, 1}
    return key


def test_prediction_agrees_with_the_ideal_rotation(small_key):
    rws = ref_rows(834)[:24]
    for bits in (1, 2):
        fast = O.values(rws, small_key, bits)
        assert [O.value_by_rotation(r, small_key, bits) for r in rws] == [int(v) for v in fast]


@pytest.mark.parametrize("bits", (1, 2))
def test_balance(small_key, bits):
    """a condition on the definition, checked on the reference: exact counts, and inside the binomial bound"""
    v = O.values(O.rows(SEED, 834, BALANCE_ROWS), small_key, bits)
    counts = np.bincount(v, minlength=1 << bits).tolist()
    print(f"bits {bits}: counts {counts}")
    assert len(counts) == 1 << bits and sum(counts) == BALANCE_ROWS
    mid, tol = BALANCE_BOUND[bits]
    assert all(abs(c - mid) <= tol for c in counts), counts
    assert counts == BALANCE[bits]


def test_radix_assembly(small_key):
    full, blocks = O.radix_value(SEED, small_key, 32, 32)
    assert len(blocks) == 16 and blocks == [int(v) for v in O.values(ref_rows(834)[:16], small_key, 2)]
    v13, b13 = O.radix_value(SEED, small_key, 32, 13)
    assert v13 < 1 << 13 and b13[:6] == blocks[:6] and b13[6] in (0, 1) and not any(b13[7:])
    assert b13[6] == int(O.values(ref_rows(834)[6:7], small_key, 1)[0])


@pytest.mark.parametrize("bound", (1, 2, 200, 255, 256))
def test_random_below_reference(bound):
    for extra in (0, 1, 8):
        m = O.random_below_bits(bound, extra)
        seen = set()
        for r in {0, 1, (1 << m) - 1, (1 << m) // 2, (1 << m) // 3} | set(range(min(1 << m, 512))):
            if r < (1 << m):
                v = O.random_below(r, bound, m)
                assert 0 <= v < bound
                seen.add(v)
        if m <= 9:  # every r was tried: every value below the bound is reached
            assert seen == set(range(bound))
