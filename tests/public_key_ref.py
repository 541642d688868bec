"""numpy restatement of public-key encryption (include/fhe_rocm.h "public-key encryption"),
with its own RFC 8439 block function: it uses neither the engine's nor the oracle's stream code.

  key    A = u64 words [0, 2048) of ChaCha20(key = the 32 PUBLIC seed bytes as little-endian words,
         nonce = {104, "ROCM", 0}); B = A S + E in Z_2^64[X] / (X^2048 + 1), E_j = tuniform(w_j), w the next
         2048 u64 of the client key's encryption stream
  list   chunk c, from streams keyed by the SECRET encryption seed: R bit i = bit (i & 63) of u64 word
         32 c + (i >> 6) under nonce {105, "ROCM", 0}; E1 = u64 words [4096 c, 4096 c + 2048) under nonce
         {106, "ROCM", 0}, E2 the words after them; C_A = A R + E1, C_B[j] = (B R)[j] + E2[j] + delta m_j
  expand row of coefficient t: mask u = C_A[t - u] (u <= t), -C_A[t - u + 2048] (u > t); body C_B[t]
"""
import struct

import numpy as np

N = 2048
ROCM = 0x524F434D
FHES = 0x46484553
NOISE_LOG2 = 17
DELTA = 1 << 59  # 2^63 / (message 4 x carry 4)
M64 = (1 << 64) - 1
STREAM_PK_MASK, STREAM_BINARY, STREAM_NOISE = 104, 105, 106
RADIX, BIGUINT = 0, 1
KEY_BYTES = 32 + 36 + 32 + 8 * N  # frame header, params, seed, body


def list_bytes(nvalues, ncoef):
    """a serialized list: frame header, params, packed + nvalues, the value table, C_A per chunk, C_B"""
    return 32 + 36 + 8 + 8 * nvalues + 8 * (N * ((ncoef + N - 1) // N) + ncoef)


# ------------------------------------------------------------------ ChaCha20 (RFC 8439)
def _rotl(v, c):
    return (v << np.uint32(c)) | (v >> np.uint32(32 - c))


def chacha_blocks(key8, nonce3, counters):
    """the block function for an array of block counters -> (len, 16) uint32"""
    ctr = np.asarray(counters, dtype=np.uint32)
    const = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
    s = [np.full(ctr.shape, v, np.uint32) for v in (*const, *key8)] + [ctr] + [np.full(ctr.shape, v, np.uint32) for v in nonce3]
    x = [v.copy() for v in s]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        return np.stack([x[i] + s[i] for i in range(16)], axis=1)


def stream_u64(key8, nonce3, first, n):
    """u64 words [first, first + n) of the stream: word w = u32 word 2w | u32 word 2w + 1 << 32"""
    b0, b1 = first // 8, (first + n + 7) // 8
    words = np.ascontiguousarray(chacha_blocks(key8, nonce3, np.arange(b0, b1, dtype=np.uint64))).astype("<u4")
    return words.reshape(-1).view("<u8")[first - 8 * b0: first - 8 * b0 + n].astype(np.uint64)


def seed_key(seed32):
    return struct.unpack("<8I", seed32)


def enc_stream_key(seed64):
    """fhe_client_key_seed_encryption(S, T): key {S lo, S hi, "FHES", 0 ...}, nonce {T, "ROCM", 0}"""
    return (seed64 & 0xFFFFFFFF, seed64 >> 32, FHES, 0, 0, 0, 0, 0)


def tuniform(words, b=NOISE_LOG2):
    """tuniform_of over an array of stream words, as uint64 mod 2^64"""
    w = np.asarray(words, dtype=np.uint64)
    u = w & np.uint64((1 << (b + 1)) - 1)
    c = (w >> np.uint64(b + 1)) & np.uint64(1)
    return u + c - np.uint64(1 << b)  # wraps


# ------------------------------------------------------------------ polynomials
def mul_binary(a, bits):
    """a * s mod (X^N + 1) over Z / 2^64 for the binary polynomial s (array of 0 / 1)"""
    a = np.asarray(a, dtype=np.uint64)
    r = np.zeros(N, np.uint64)
    for j in np.flatnonzero(np.asarray(bits)):
        j = int(j)
        r[j:] += a[:N - j]
        r[:j] -= a[N - j:]
    return r


def key_body(mask_seed, sk, enc_key, enc_nonce, enc_first=0):
    A = stream_u64(seed_key(mask_seed), (STREAM_PK_MASK, ROCM, 0), 0, N)
    E = tuniform(stream_u64(enc_key, enc_nonce, enc_first, N))
    return mul_binary(A, sk) + E


# ------------------------------------------------------------------ lists
def blocks_of(form, value, count):
    """the 2-bit blocks of a value: count = num_bits (radix) or nlimbs (BigUintFHE), LSB first"""
    nb = count // 2 if form == RADIX else 16 * count
    return [(value >> (2 * k)) & 3 for k in range(nb)]


def coefficients(values, packed):
    """values: [(form, value, count)] -> the plaintext of every coefficient, and each value's first one"""
    m, firsts = [], []
    for form, value, count in values:
        firsts.append(len(m))
        b = blocks_of(form, value, count)
        if packed:
            m += [b[k] + (4 * b[k + 1] if k + 1 < len(b) else 0) for k in range(0, len(b), 2)]
        else:
            m += b
    return m, firsts


def encrypt(mask_seed, body, enc_seed, m):
    """(C_A (nchunks, N), C_B (ncoef,)) of the coefficient plaintexts m"""
    A = stream_u64(seed_key(mask_seed), (STREAM_PK_MASK, ROCM, 0), 0, N)
    key = seed_key(enc_seed)
    ncoef = len(m)
    chunks = (ncoef + N - 1) // N
    ca, cb = np.zeros((chunks, N), np.uint64), np.zeros(ncoef, np.uint64)
    for c in range(chunks):
        used = min(N, ncoef - c * N)
        rw = stream_u64(key, (STREAM_BINARY, ROCM, 0), 32 * c, 32)
        R = np.array([(int(rw[i >> 6]) >> (i & 63)) & 1 for i in range(N)], np.uint64)
        noise = tuniform(stream_u64(key, (STREAM_NOISE, ROCM, 0), 2 * N * c, N + used))
        ca[c] = mul_binary(A, R) + noise[:N]
        mm = np.array(m[c * N: c * N + used], np.uint64) * np.uint64(DELTA)
        cb[c * N: c * N + used] = mul_binary(body, R)[:used] + noise[N:] + mm
    return ca, cb


def expand(ca, cb):
    """(ncoef, 2049): the sample extraction of every coefficient"""
    ncoef = len(cb)
    rows = np.zeros((ncoef, N + 1), np.uint64)
    u = np.arange(N)
    for g in range(ncoef):
        t, A = g % N, ca[g // N]
        rows[g, :N] = np.where(u <= t, A[(t - u) % N], np.uint64(0) - A[(t - u) % N])
        rows[g, N] = cb[g]
    return rows


def phase_errors(rows, sk, m):
    """signed phase - delta m of every row"""
    ph = rows[:, N] - (rows[:, :N] * np.asarray(sk, np.uint64)).sum(axis=1, dtype=np.uint64)
    err = ph - np.array(m, np.uint64) * np.uint64(DELTA)
    return err.astype(np.int64)


def refnv(blob):
    """the frame with its checksum recomputed (FNV-1a over the payload's u64 words, tail zero-padded)"""
    blob = bytearray(blob)
    payload = bytes(blob[32:])
    payload += b"\0" * (-len(payload) % 8)
    h = 0xCBF29CE484222325
    for (x,) in struct.iter_unpack("<Q", payload):
        h = ((h ^ x) * 0x100000001B3) & M64
    blob[24:32] = struct.pack("<Q", h)
    return bytes(blob)


def frame(kind, payload):
    return refnv(b"FHEROCM\0" + struct.pack("<IIQQ", 2, kind, len(payload), 0) + payload)
