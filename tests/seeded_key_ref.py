"""Test-only restatement of the seeded server key (include/fhe_rocm.h "seeded (compressed) server key"),
shared by tests/test_seeded_server_key.py and tests/test_seeded_server_key_gpu.py: this file's own RFC 8439
ChaCha20 in numpy, the wire layout of kind 6, and an oracle re-keyed to an expanded key.  It uses neither
the engine's nor the oracle's stream code.  Never used by the product."""
import ctypes as C
import struct

import numpy as np

import oracle
from lwe_dims import oracle_params

ROCM = 0x524F434D
FHES = 0x46484553
N = 2048
KS_LEVEL, KS_BASE_LOG, PBS_BASE_LOG = 5, 3, 23
LWE_NOISE_LOG2, GLWE_NOISE_LOG2 = 45, 17
KSK_ROWS = N * KS_LEVEL
STREAM_KSK, STREAM_BSK = 102, 103
HEADER, PARAMS = 32, 36
SEED_OFF = HEADER + PARAMS
BODY_OFF = SEED_OFF + 32  # = 100
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ ChaCha20 (RFC 8439)
def _rotl(v, c):
    return (v << np.uint32(c)) | (v >> np.uint32(32 - c))


def chacha_blocks(key8, nonce3, counters):
    """block function for an array of block counters -> (len, 16) uint32"""
    ctr = np.asarray(counters, dtype=np.uint32)
    const = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
    s = [np.full(ctr.shape, v, np.uint32) for v in (*const, *key8)] + [ctr] + [np.full(ctr.shape, v, np.uint32) for v in nonce3]
    x = [v.copy() for v in s]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return np.stack([x[i] + s[i] for i in range(16)], axis=1)


def stream_u64(key8, nonce3, first, n):
    """u64 words [first, first + n) of the stream: word w = u32 word 2w | u32 word 2w + 1 << 32"""
    b0, b1 = first // 8, (first + n + 7) // 8
    words = np.ascontiguousarray(chacha_blocks(key8, nonce3, np.arange(b0, b1, dtype=np.uint64))).astype("<u4")
    return words.reshape(-1).view("<u8")[first - 8 * b0: first - 8 * b0 + n].astype(np.uint64)


def row_masks(seed32, stream, rows, width):
    """(rows, width): row r = u64 words [2048 r, 2048 r + width) of the stream keyed by the public seed"""
    key = struct.unpack("<8I", seed32)
    nblk = (width + 7) // 8
    ctr = (256 * np.arange(rows, dtype=np.uint64)[:, None] + np.arange(nblk, dtype=np.uint64)[None, :]).reshape(-1)
    w = np.ascontiguousarray(chacha_blocks(key, (stream, ROCM, 0), ctr)).astype("<u4")
    return w.reshape(rows, nblk * 16).view("<u8")[:, :width].astype(np.uint64)


def seed_key(seed64):
    """the key of fhe_client_key_seed_encryption(seed64, stream)"""
    return (seed64 & 0xFFFFFFFF, seed64 >> 32, FHES, 0, 0, 0, 0, 0)


def tuniform(x, b):
    """TUniform(b) of stream words, as uint64 (wrapping)"""
    x = np.atleast_1d(np.asarray(x, np.uint64))  # arrays wrap silently, numpy scalars warn
    u = x & np.uint64((1 << (b + 1)) - 1)
    c = (x >> np.uint64(b + 1)) & np.uint64(1)
    return u + c - np.uint64(1 << b)


# ------------------------------------------------------------------ wire format, kind 6
def ggsw_count(n, grouping):
    return n if grouping == 1 else n // grouping * ((1 << grouping) - 1)


def wire_len(n, grouping):
    return 100 + 8 * (N * KS_LEVEL + 4096 * ggsw_count(n, grouping))


def parse(blob, n, grouping):
    """(seed, ksk bodies [10240], bsk bodies [2 ggsw][2048]) of a serialized seeded server key"""
    assert len(blob) == wire_len(n, grouping)
    seed = blob[SEED_OFF:BODY_OFF]
    words = np.frombuffer(blob, "<u8", offset=BODY_OFF).astype(np.uint64)
    return seed, words[:KSK_ROWS], words[KSK_ROWS:].reshape(2 * ggsw_count(n, grouping), N)


def refnv(blob):
    """the frame with its checksum recomputed (FNV-1a over the payload's u64 words, tail zero-padded)"""
    blob = bytearray(blob)
    payload = bytes(blob[32:])
    payload += b"\0" * (-len(payload) % 8)
    h = 0xCBF29CE484222325
    for x in np.frombuffer(payload, "<u8").tolist():
        h = ((h ^ x) * 0x100000001B3) & M64
    blob[24:32] = struct.pack("<Q", h)
    return bytes(blob)


def frame(kind, payload):
    return refnv(b"FHEROCM\0" + struct.pack("<IIQQ", 2, kind, len(payload), 0) + payload)


def ggsw_messages(lwe_sk, n, grouping):
    s = [int(v) for v in lwe_sk]
    if grouping == 1:
        return s
    out = []
    for q in range(ggsw_count(n, grouping)):
        i, b = q // 3, q % 3 + 1
        f0 = s[2 * i] if b & 1 else 1 - s[2 * i]
        f1 = s[2 * i + 1] if b & 2 else 1 - s[2 * i + 1]
        out.append(f0 & f1)
    return out


def negacyclic_binary(a, sk):
    """rows of `a` times the binary polynomial sk mod X^N + 1, exact in Z / 2^64"""
    r = np.zeros_like(a)
    for j in np.flatnonzero(sk):
        j = int(j)
        r[:, j:] += a[:, :N - j]
        if j:
            r[:, :j] -= a[:, N - j:]
    return r


# ------------------------------------------------------------------ the oracle under an expanded key
def rekeyed_oracle(seed, n, grouping, ksk, bsk, fourier=True):
    """oracle.OracleKeys(seed) -- the secrets of generate_keys(seed=seed) -- with its KSK and BSK words
    overwritten by an expanded seeded key's; the Fourier BSK recomputed polynomial by polynomial
    (fourier=False: keyswitch only, the Fourier key stays the oracle's own and must not be used)"""
    ok = oracle.OracleKeys(seed, oracle_params(n, grouping))
    assert ok.ksk.shape == ksk.shape and ok.bsk.shape == bsk.shape
    ok.ksk[:] = ksk
    ok.bsk[:] = bsk
    if fourier:
        lib = oracle.load()
        poly = np.zeros(N, np.uint64)
        out = np.zeros(N, np.float64)
        f = ok.bsk_f.reshape(-1, N)
        for i, p in enumerate(ok.bsk.reshape(-1, N)):
            poly[:] = p
            lib.fho_poly_to_fourier(poly.ctypes.data_as(oracle.u64p), out.ctypes.data_as(oracle.dblp))
            f[i] = out
    return ok
