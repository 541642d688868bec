"""Test-only restatement of the oblivious pseudo-random values (include/fhe_rocm.h "oblivious pseudo-random
values") in numpy and Python integers: the rows from tests/test_seeded.py's own ChaCha20, the
accumulator, the value a block must decrypt to (from tests/exact_pbs_ref.py's modulus switch and the small
secret), the radix assembly and random_below.  Nothing here calls the product.  Never used by the product."""
import numpy as np

import exact_pbs_ref as X
from test_seeded import ROCM, chacha_blocks, mask_key

STREAM = 111  # kStreamOprf
PAD = 0xA5A55A5AC3C33C3C  # MS_PAD_WORD
N = 2048
DELTA = 1 << 59  # 2^63 / (message 4 x carry 4)
MSG_BITS = 2


def ms_stride(n):
    return (n + 1 + 7) // 8 * 8


def rows(seed32, n, count, stride=None, first=0):
    """rows [first, first + count): (count, stride) words, mask words from ChaCha blocks [b R, (b + 1) R) of the
    seed's stream, 0 at word n, the marker above"""
    stride = n + 1 if stride is None else stride
    R = (n + 7) // 8
    ctr = np.arange(first * R, (first + count) * R, dtype=np.uint64)
    words = np.ascontiguousarray(chacha_blocks(mask_key(seed32), (STREAM, ROCM, 0), ctr)).astype("<u4")
    words = words.reshape(count, R * 16).view("<u8").astype(np.uint64)
    out = np.full((count, stride), PAD, np.uint64)
    out[:, :n] = words[:, :n]
    out[:, n] = 0
    return out


def lut(bits, delta=DELTA):
    """coefficient i = (2 floor(i p / 2N) + 1) delta / 2"""
    p = 1 << bits
    return np.array([((2 * (i * p // (2 * N)) + 1) * (delta // 2)) % (1 << 64) for i in range(N)], np.uint64)


def body_const(bits, delta=DELTA):
    return ((1 << bits) - 1) * (delta // 2)


def rounded_phase(rws, lwe_sk):
    """m~ = -sum ms(a_i) s_i mod 2N of (count, >= n + 1) rows under the n-word binary secret"""
    n = len(lwe_sk)
    a = X.modswitch(np.asarray(rws, np.uint64)[:, :n], N).astype(np.int64)
    return (-(a @ np.asarray(lwe_sk, np.uint64).astype(np.int64))) % (2 * N)


def values(rws, lwe_sk, bits):
    """what block b decrypts to: floor(m~ p / 2N) + p / 2 for m~ < N, p / 2 - 1 - floor((m~ - N) p / 2N) otherwise"""
    p = 1 << bits
    m = rounded_phase(rws, lwe_sk)
    return np.where(m < N, m * p // (2 * N) + p // 2, p // 2 - 1 - (m - N) * p // (2 * N))


def value_by_rotation(row, lwe_sk, bits, delta=DELTA, mc=16):
    """the same for one row of n + 1 words through exact_pbs_ref.ideal_rotation: coefficient 0 of the noiseless
    blind rotation of the accumulator, plus the body constant, decoded in a message space of mc values
    (delta = 2^63 / mc)"""
    assert delta * mc == 1 << 63
    c0 = int(X.ideal_rotation(np.asarray(row, np.uint64)[:len(lwe_sk) + 1], lwe_sk, lut(bits, delta))[0])
    phase = (c0 + body_const(bits, delta)) % (1 << 64)
    return ((phase + delta // 2) // delta) % mc


def radix_value(seed32, lwe_sk, width_bits, random_bits):
    """the integer a radix value of width_bits with random_bits random bits decrypts to, and its blocks' values"""
    n = len(lwe_sk)
    full, odd = divmod(random_bits, MSG_BITS)
    rws = rows(seed32, n, full + (1 if odd else 0))
    blocks = [int(v) for v in values(rws[:full], lwe_sk, MSG_BITS)] if full else []
    if odd:
        blocks.append(int(values(rws[full:], lwe_sk, odd)[0]))
    blocks += [0] * (width_bits // MSG_BITS - len(blocks))
    return sum(v << (MSG_BITS * i) for i, v in enumerate(blocks)), blocks


def random_below(r, bound, m):
    """(r bound) >> m of the m-bit r"""
    assert 0 <= r < (1 << m) and bound > 0
    return (r * bound) >> m


def random_below_bits(bound, extra_bits):
    return (bound - 1).bit_length() + extra_bits
