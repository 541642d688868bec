"""numpy restatement of the re-randomization under the compact public key (include/fhe_rocm.h "re-randomization
under the public key"), on the ChaCha and product helpers of tests/public_key_ref.py: it uses
neither the engine's nor the oracle's stream code.

  chunk c of blocks 0 .. n-1, from streams keyed by the re-randomization seed:
      R bit i = bit (i & 63) of u64 word 32 c + (i >> 6) under nonce {109, "ROCM", 0}
      E1 = u64 words [4096 c, 4096 c + 2048) under nonce {110, "ROCM", 0}, E2 the words after them (one per used
      block), each through tuniform
      Z_A = A R + E1, Z_B[j] = (B R)[j] + E2[j]
  block i (t = i mod 2048 of chunk i // 2048): mask u += Z_A[t - u] (u <= t), -= Z_A[t - u + 2048] (u > t);
      body += Z_B[t]
"""
import hashlib
import struct

import numpy as np

from public_key_ref import N, ROCM, STREAM_PK_MASK, mul_binary, seed_key, stream_u64, tuniform

STREAM_BINARY, STREAM_NOISE = 109, 110
TAG = b"fhe-rocm/rerandomize"


def zero(mask_seed, body, seed, n):
    """(Z_A (nchunks, N), Z_B (n,)) of the zero encryptions of n blocks"""
    A = stream_u64(seed_key(mask_seed), (STREAM_PK_MASK, ROCM, 0), 0, N)
    key = seed_key(seed)
    chunks = (n + N - 1) // N
    za, zb = np.zeros((chunks, N), np.uint64), np.zeros(n, np.uint64)
    for c in range(chunks):
        used = min(N, n - c * N)
        rw = stream_u64(key, (STREAM_BINARY, ROCM, 0), 32 * c, 32)
        R = np.array([(int(rw[i >> 6]) >> (i & 63)) & 1 for i in range(N)], np.uint64)
        noise = tuniform(stream_u64(key, (STREAM_NOISE, ROCM, 0), 2 * N * c, N + used))
        za[c] = mul_binary(A, R) + noise[:N]
        zb[c * N: c * N + used] = mul_binary(body, R)[:used] + noise[N:]
    return za, zb


def apply(za, zb, rows):
    """the rows (n, 2049) with the sample extraction of (za, zb) at coefficient i added to row i"""
    out = np.array(rows, dtype=np.uint64).reshape(-1, N + 1)
    u = np.arange(N)
    for i in range(out.shape[0]):
        t, Z = i % N, za[i // N]
        out[i, :N] += np.where(u <= t, Z[(t - u) % N], np.uint64(0) - Z[(t - u) % N])
    out[:, N] += np.asarray(zb, np.uint64)
    return out


def rerandomize(mask_seed, body, seed, rows):
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, N + 1)
    za, zb = zero(mask_seed, body, seed, rows.shape[0])
    return apply(za, zb, rows)


def derive_seed(domain, data):
    t = hashlib.sha256(TAG).digest()
    return hashlib.sha256(t + t + struct.pack("<Q", len(domain)) + domain + data).digest()
