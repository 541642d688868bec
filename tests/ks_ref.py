"""Test-only integer restatement of the keyswitch and of the radix layer's linear prologue, in wrapping
uint64 numpy -- the word-level reference of tests/test_keyswitch_ref.py (against the oracle, on the CPU)
and tests/test_keyswitch_gpu.py (against both kernels).  Parameters of the default set: 2048 mask
words, 5 balanced base-8 digits of the top 15 bits.  Never used by the product."""
import numpy as np

N = 2048
BIG_CT = N + 1
LEVELS = 5
BASE_LOG = 3
M64 = (1 << 64) - 1


def digits(ct):
    """balanced digits of the mask words of `ct` (..., >= 2048 words): int64 (..., 2048, 5), level 0 the
    most significant, as the KSK rows are ordered.  Closed form: round to the top 15 bits, add 4 to every
    base-8 digit (0o44444: the carries of that sum are the balancing carries), take the digits of the
    sum and subtract the 4 again -- digits in [-4, 3]; the carry out of the top digit falls off the mask."""
    a = np.asarray(ct, np.uint64)[..., :N]
    v = (((a >> np.uint64(63 - BASE_LOG * LEVELS)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(0x7FFF)
    w = v + np.uint64(0o44444)
    sh = np.uint64(BASE_LOG) * np.arange(LEVELS - 1, -1, -1, dtype=np.uint64)
    return ((w[..., None] >> sh) & np.uint64(7)).astype(np.int64) - 4


def keyswitch_np(ksk, n, ct):
    """(..., 2049) big LWE -> (..., n + 1) small LWE: body - sum_{j, l} d[j, l] KSK[j, l] mod 2^64, with
    `ksk` the flat [2048][5][n + 1] key of ServerKey.export()"""
    K = np.asarray(ksk, np.uint64).reshape(N * LEVELS, n + 1)
    ct = np.asarray(ct, np.uint64)
    d = digits(ct).reshape(ct.shape[:-1] + (N * LEVELS,)).astype(np.uint64)  # two's complement
    with np.errstate(over="ignore"):
        out = np.uint64(0) - np.dot(d, K)
        out[..., n] += ct[..., N]
    return out


def lincomb_np(blocks, terms, cst):
    """sum coef * blocks[src] over `terms` = [(src, coef), ...], plus `cst` on the body, mod 2^64"""
    blocks = np.asarray(blocks, np.uint64)
    acc = np.zeros(BIG_CT, np.uint64)
    with np.errstate(over="ignore"):
        for src, coef in terms:
            acc += np.uint64(coef & M64) * blocks[src]
        acc[N] += np.uint64(cst & M64)
    return acc


def byte_planes(ksk):
    """balanced signed bytes of every KSK word: int64 (8, len), ksk = sum_b planes[b] 256^b mod 2^64
    with planes[b] in [-128, 128) -- the split ks_mfma.hip contracts plane by plane"""
    v = np.asarray(ksk, np.uint64).copy()
    planes = np.empty((8, v.size), np.int64)
    with np.errstate(over="ignore"):
        for b in range(8):
            s = (v & np.uint64(255)).astype(np.int64)
            s[s >= 128] -= 256
            planes[b] = s
            v = (v - s.astype(np.uint64)) >> np.uint64(8)
    return planes


def plane_sum(plane, b, n, ct):
    """(sum_{j, l} d[j, l] K_b[j, l]) << 8 b mod 2^64 for plane = byte_planes(ksk)[b]: what plane b
    contributes to the keyswitch (the keyswitch subtracts it)"""
    ct = np.asarray(ct, np.uint64)
    d = digits(ct).reshape(ct.shape[:-1] + (N * LEVELS,))
    s = np.dot(d, np.asarray(plane, np.int64).reshape(N * LEVELS, n + 1))  # |s| < 2^23: exact
    return s.astype(np.uint64) << np.uint64(8 * b)


def modswitch(x):
    """the blind rotation's view of a small LWE word: bits 51 and up, rounded (device_math.h
    modswitch_2n, oracle fho_modswitch)"""
    x = np.asarray(x, np.uint64)
    return (((x >> np.uint64(51)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(2 * N - 1)


EDGE_PATTERNS = (0, 0x7FFF, 0x4000, 0x3FFF, 0o44444, 0o33333, 0o43434, 0o34343)
EDGE_LOWS = (0, (1 << 48) - 1, 1 << 48, (1 << 48) + 1, (1 << 49) - 1)


def edge_rows():
    """four hand-built big LWE rows that put the rounding bit and every digit carry chain at their
    edges: (0) every 15-bit pattern of EDGE_PATTERNS over every low part of EDGE_LOWS (below, at and
    above the rounding bit 2^48), body 0; (1) every digit 4 -> -4 with a carry through all five
    levels, body 2^63; (2) all ones: rounds up and wraps to zero digits, body 2^64 - 1; (3) zero
    mask: the output is (0, .., 0, body)"""
    words = [(p << 49) | lo for p in EDGE_PATTERNS for lo in EDGE_LOWS]
    rows = np.zeros((4, BIG_CT), np.uint64)
    rows[0, :N] = np.resize(np.array(words, np.uint64), N)
    rows[1, :N] = np.uint64(0o44444 << 49)
    rows[1, N] = np.uint64(1 << 63)
    rows[2, :] = np.uint64(M64)
    rows[3, N] = np.uint64(0x0123456789ABCDEF)
    return rows
