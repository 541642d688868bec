"""Test-only exact-integer restatement of the programmable bootstrap: wrapping uint64 / int64 numpy and
Python integers, no floating point anywhere, nothing imported from the oracle or the product.  It is the
reference that tests/test_exact_pbs.py holds oracle/tfhe_oracle.c to, and tests/test_exact_pbs_gpu.py
the blind-rotate kernels: both compute the same blind rotation through an f64 negacyclic FFT, this
module computes it in Z[X]/(X^N + 1) mod 2^64.  Keys and secrets come in as arrays of words.

Shapes.  A polynomial is N uint64 words (N a power of two, 32 or more), a GLWE is (2, N) = (mask, body), a
GGSW is (2, 2, N) = [row][poly] with row 0 multiplying the mask's digit, a bootstrapping key is
(ggsw, 2, 2, N) -- the [ggsw][row][poly][N] words of ServerKey.export().  One gadget level, base 2^23.

The blind rotation is the project's form, not the textbook one:
  classic    acc += (X^a_i - 1) ExtProd(GGSW_i, acc)                              i = 0 .. n - 1
  multi-bit  acc += sum_B (X^m_B - 1) ExtProd(GGSW_(3i + B - 1), acc), B = 1, 2, 3, i = 0 .. n / 2 - 1
             m_1 = a_2i, m_2 = a_2i+1, m_3 = m_1 + m_2 mod 2N, the three terms on the digits of one acc
with ExtProd(G, acc) = digit(acc.mask) G[0] + digit(acc.body) G[1].

Digit tie rule (digit()).  A word is read as a signed value v in [-2^63, 2^63); g = v / 2^41 rounded to
the nearest integer, ties to the even one; the digit is g - 2^23 round(g / 2^23) with the same tie rule,
so it lies in [-2^22, 2^22], both ends reachable: g = 2^22 keeps +2^22 (g / 2^23 = 1/2 rounds to 0) and
g = -2^22 keeps -2^22.  Any other choice at a tie is an equally exact bootstrap with other words (a digit
off by 2^23 adds 2^23 times a key row: an encryption of zero); this one is what fho_tor_digit computes
on the same signed value, which test_exact_pbs.py checks on the tie values.  Where the f64 paths hold an
unreduced representative outside [-2^63, 2^63) their tie can fall the other way; words then differ,
phases agree to the key noise times 2^23.
Never used by the product."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from numpy.lib.stride_tricks import as_strided

import ks_ref

BASE_LOG = 23
SHIFT = 64 - BASE_LOG  # 41
M64 = (1 << 64) - 1


def _u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


def modswitch(x, N):
    """a torus word to [0, 2N): its top log2(2N) bits, rounded half up, the carry out dropped"""
    k = (2 * N).bit_length() - 1
    x = np.asarray(x, np.uint64)
    return (((x >> np.uint64(63 - k)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(2 * N - 1)


def _round_shift_even(v, k):
    """int64 v / 2^k rounded to the nearest integer, ties to even, without leaving int64"""
    lo = v & np.int64((1 << k) - 1)
    q = v >> np.int64(k)  # floor
    half = np.int64(1 << (k - 1))
    up = (lo > half) | ((lo == half) & ((q & np.int64(1)) == 1))
    return q + up.astype(np.int64)


def digit(words):
    """the one-level balanced gadget digit, base 2^23, of each word: int64 in [-2^22, 2^22] (module
    docstring: the tie rule)"""
    g = _round_shift_even(np.asarray(words, np.uint64).view(np.int64), SHIFT)  # [-2^22, 2^22]
    return g - (_round_shift_even(g, BASE_LOG) << np.int64(BASE_LOG))


def negmul(small, big):
    """small(X) big(X) mod (X^N + 1, 2^64): `small` int64 (any size: the products wrap), `big` uint64.
    Row i of the negacyclic matrix of `big` is big[i - j] for j <= i and -big[N + i - j] beyond: a
    strided view of (-big[1:], big), times `small` as two's complement words."""
    big = _u64(big)
    N = big.size
    with np.errstate(over="ignore"):
        e = np.concatenate([np.uint64(0) - big[1:], big])
        s = e.strides[0]
        T = as_strided(e[N - 1:], (N, N), (s, -s), writeable=False)
        return T @ np.ascontiguousarray(small, dtype=np.int64).view(np.uint64)


def rotate(p, r):
    """X^r p mod (X^N + 1), r in [0, 2N)"""
    p = _u64(p)
    N = p.size
    r = int(r)
    assert 0 <= r < 2 * N
    with np.errstate(over="ignore"):
        if r >= N:
            p, r = np.uint64(0) - p, r - N
        return np.concatenate([np.uint64(0) - p[N - r:], p[:N - r]])


def lut_poly(table, N):
    """the test polynomial of a 16-entry table, padding bit above 4 message bits (delta = 2^59): box m of
    N / 16 coefficients holds table[m] delta, the whole turned back by half a box, so that the
    coefficients that wrap carry -table[0] delta"""
    assert len(table) == 16 and N % 32 == 0
    box = N // 16
    j = np.arange(N) + box // 2
    vals = np.array([(int(t) % 16) << 59 for t in table], np.uint64)
    with np.errstate(over="ignore"):
        return np.where(j < N, vals[np.minimum(j, N - 1) // box], np.uint64(0) - vals[0])


def sample_extract(glwe):
    """the LWE of coefficient 0: mask (a_0, -a_(N-1), .., -a_1), body b_0"""
    glwe = _u64(glwe)
    with np.errstate(over="ignore"):
        return np.concatenate([glwe[0, :1], np.uint64(0) - glwe[0, :0:-1], glwe[1, :1]])


def lwe_phase(ct, secret):
    """body - <mask, secret> mod 2^64 of (.., n + 1) words under a binary secret of n words"""
    ct = np.asarray(ct, np.uint64)
    with np.errstate(over="ignore"):
        return ct[..., -1] - ct[..., :-1] @ _u64(secret)


def glwe_phase(glwe, secret):
    """body - mask S mod (X^N + 1, 2^64): N words"""
    glwe = _u64(glwe)
    with np.errstate(over="ignore"):
        return glwe[1] - negmul(np.asarray(secret, np.uint64).astype(np.int64), glwe[0])


def signed(words):
    """torus words as int64 in [-2^63, 2^63)"""
    return np.asarray(words, np.uint64).view(np.int64)


def ext_prod(ggsw, acc, threads=1):
    """digit(acc.mask) G[0] + digit(acc.body) G[1], both output polynomials: (2, N)"""
    d = (digit(acc[0]), digit(acc[1]))
    p = threads_map(lambda rw: negmul(d[rw[0]], ggsw[rw[0], rw[1]]), [(0, 0), (1, 0), (0, 1), (1, 1)], threads)
    with np.errstate(over="ignore"):
        return np.stack([p[0] + p[1], p[2] + p[3]])


def _times_monomial_minus_one(glwe, r):
    with np.errstate(over="ignore"):
        return np.stack([rotate(p, r) - p for p in glwe])


def blind_rotate(bsk, small, lut, grouping=1, steps=None, threads=1):
    """(2, N) accumulator after the blind rotation of the small LWE `small` (n + 1 words) through the
    polynomial `lut`; `steps` stops after that many classic updates / multi-bit groups; `threads` spreads
    the four products of an external product (for a single long rotation)"""
    lut = _u64(lut)
    N = lut.size
    small = _u64(small)
    n = small.size - 1
    bsk = np.asarray(bsk, np.uint64).reshape(-1, 2, 2, N)
    a = [int(x) for x in modswitch(small, N)]
    acc = np.stack([np.zeros(N, np.uint64), rotate(lut, (2 * N - a[n]) % (2 * N))])
    assert grouping in (1, 2) and n % grouping == 0
    assert bsk.shape[0] == (n if grouping == 1 else n // 2 * 3)
    count = n // grouping if steps is None else steps
    with np.errstate(over="ignore"):
        for i in range(count):
            if grouping == 1:
                acc = acc + _times_monomial_minus_one(ext_prod(bsk[i], acc, threads), a[i])
            else:
                m = (a[2 * i], a[2 * i + 1], (a[2 * i] + a[2 * i + 1]) % (2 * N))
                acc = acc + sum(_times_monomial_minus_one(ext_prod(bsk[3 * i + B], acc, threads), m[B]) for B in range(3))
    return acc


def ideal_rotation(small, lwe_secret, lut):
    """what a noiseless blind rotation holds in its body: X^(-b + sum a_i s_i) lut, exponents after
    the modulus switch"""
    N = len(lut)
    a = [int(x) for x in modswitch(_u64(small), N)]
    s = [int(x) for x in lwe_secret]
    r = (sum(ai * si for ai, si in zip(a[:-1], s)) - a[-1]) % (2 * N)
    return rotate(lut, r)


def threads_map(fn, items, threads=8):
    """fn over items on a few threads (numpy's integer products release the interpreter lock)"""
    items = list(items)
    if len(items) < 2 or threads < 2:
        return [fn(x) for x in items]
    with ThreadPoolExecutor(threads) as pool:
        return list(pool.map(fn, items))


def blind_rotate_batch(bsk, smalls, luts, grouping=1, threads=8):
    """(count, 2, N): blind_rotate of every row of `smalls` through the matching row of `luts`"""
    return np.stack(threads_map(lambda i: blind_rotate(bsk, smalls[i], luts[i], grouping), range(len(smalls)), threads))


def bootstrap_batch(ksk, bsk, n, cts, luts, grouping=1, threads=8):
    """keyswitch (tests/ks_ref.py, N = 2048), blind rotation, sample extraction of (count, 2049) big LWE
    rows: the (count, n + 1) small rows, the (count, 2, 2048) accumulators and the (count, 2049) outputs"""
    smalls = ks_ref.keyswitch_np(ksk, n, cts)
    accs = blind_rotate_batch(bsk, smalls, luts, grouping, threads)
    return smalls, accs, np.stack([sample_extract(g) for g in accs])
