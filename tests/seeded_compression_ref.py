"""Test-only numpy restatement of the seeded (compressed) compression key (include/fhe_rocm.h "seeded
(compressed) compression key"), shared by tests/test_seeded_compression_key.py and
tests/test_seeded_compression_key_gpu.py.  Written from the formulas, on compress_ref.py's polynomial
helpers and seeded_key_ref.py's own ChaCha20; it uses nothing of the product:

  masks   ChaCha20 keyed by the public seed, nonce {id, "ROCM", 0}, one row per 256 blocks (2048 u64 words)
          packing KSK (id 107) row r = j ell + l: coefficient m of mask polynomial c = word 2048 r + c N' + m
          BSK (id 108) GGSW q, row rho: mask coefficient m = word 2048 (2 q + rho) + m
  noise   the client key's encryption stream: k' N' secret words, N' words per packing row, 2048 per BSK row
  bodies  packing KSK: B = sum_c A_c * s'_c + e, B[0] += S_j << (64 - beta (l + 1))
          BSK: B = A * S + e; row 1: B[0] += g s'_q; row 0: B[t] -= g s'_q S_t

Never used by the product."""
import struct

import numpy as np

import compress_ref as R
import seeded_key_ref as K

STREAM_PKSK, STREAM_CBSK = 107, 108
KIND = 12
HEADER = 32 + 36 + 28 + 32  # frame, main params, compression params, seed
SEED_OFF = 32 + 36 + 28
N_BIG = R.N_BIG

# (k', N', L, beta, ell, noise): the two sets compress_ref.py does not have
MIXED = R.CP(2, 8, 5, 7, 4, 42)      # cols 24: a tile of masks, then 8 bodies + 8 padding columns; 7-bit digits
STRIDE = R.CP(1, 2048, 4, 4, 1, 42)  # a mask row fills its 256-block stride exactly


def pksk_body_words(cp):
    return N_BIG * cp.ell * cp.N


def bsk_body_words(cp):
    return 2 * cp.k * cp.N * N_BIG


def stream_words(cp):
    """u64 words of the client key's encryption stream the seeded generation consumes"""
    return cp.k * cp.N + pksk_body_words(cp) + bsk_body_words(cp)


def wire_len(cp):
    return HEADER + 8 * (pksk_body_words(cp) + bsk_body_words(cp))


def parse(cp, blob):
    """(seed, packing bodies [2048 ell][N'], BSK bodies [2 k' N'][2048]) of a serialized seeded key"""
    assert len(blob) == wire_len(cp)
    assert struct.unpack_from("<7I", blob, 68) == (cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12)
    words = np.frombuffer(blob, "<u8", offset=HEADER).astype(np.uint64)
    n = pksk_body_words(cp)
    return bytes(blob[SEED_OFF:HEADER]), words[:n].reshape(N_BIG * cp.ell, cp.N), words[n:].reshape(2 * cp.k * cp.N, N_BIG)


def masks(seed32, stream, rows, width):
    """(len(rows), width): row r = u64 words [2048 r, 2048 r + width) of the stream keyed by the public seed"""
    key = struct.unpack("<8I", seed32)
    rows = np.asarray(rows, np.uint64)
    nblk = (width + 7) // 8
    ctr = (np.uint64(256) * rows[:, None] + np.arange(nblk, dtype=np.uint64)[None, :]).reshape(-1)
    w = np.ascontiguousarray(K.chacha_blocks(key, (stream, K.ROCM, 0), ctr)).astype("<u4")
    return w.reshape(len(rows), nblk * 16).view("<u8")[:, :width].astype(np.uint64)


def _noise(enc_seed, enc_stream, first, rows, width, total):
    rows = np.asarray(rows)
    if len(rows) == total:  # every row: one pass over the stream
        return R.enc_stream(enc_seed, enc_stream, first, total * width).reshape(total, width)
    return np.stack([R.enc_stream(enc_seed, enc_stream, first + int(r) * width, width) for r in rows])


def pksk_bodies(cp, enc_seed, enc_stream, seed32, sprime, S, rows):
    """(masks (len(rows), k' N'), bodies (len(rows), N')) of the packing-key rows"""
    rows = np.asarray(rows)
    kn = cp.k * cp.N
    A = masks(seed32, STREAM_PKSK, rows, kn)
    w = _noise(enc_seed, enc_stream, kn, rows, cp.N, N_BIG * cp.ell)
    body = K.tuniform(w.reshape(-1), cp.noise).reshape(len(rows), cp.N)
    for c in range(cp.k):
        body = body + R.negacyclic_binary(A[:, c * cp.N:(c + 1) * cp.N], sprime[c * cp.N:(c + 1) * cp.N], cp.N)
    shift = (64 - cp.beta * (rows % cp.ell + 1)).astype(np.uint64)
    body[:, 0] += np.asarray(S, np.uint64)[rows // cp.ell] << shift
    return A, body


def bsk_bodies(cp, enc_seed, enc_stream, seed32, sprime, S, rows):
    """(masks, bodies), both (len(rows), 2048), of the BSK rows r = 2 q + rho"""
    rows = np.asarray(rows)
    kn = cp.k * cp.N
    S = np.asarray(S, np.uint64)
    A = masks(seed32, STREAM_CBSK, rows, N_BIG)
    w = _noise(enc_seed, enc_stream, kn + pksk_body_words(cp), rows, N_BIG, 2 * kn)
    body = K.tuniform(w.reshape(-1), R.GLWE_NOISE_LOG2).reshape(len(rows), N_BIG)
    body = body + R.negacyclic_binary(A, S, N_BIG)
    g = np.uint64(1 << (64 - R.PBS_BASE_LOG))
    for i, r in enumerate(rows):
        m = np.uint64(sprime[int(r) // 2])
        if int(r) % 2:
            body[i, :1] += g * m
        else:
            body[i] -= g * m * S
    return A, body
