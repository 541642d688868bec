"""Test-only restatement of the modulus-switched stored ciphertexts (include/fhe_rocm.h "modulus-switched stored
ciphertexts"), shared by tests/test_switched.py and tests/test_switched_gpu.py.  Built from the
restatements the suite already pins -- ks_ref (keyswitch_np, modswitch), ms_center_ref, compress_ref's pack12 /
unpack12 -- it uses nothing of the product:

  r      = keyswitch_np(ksk, n, c)            n + 1 words
  r      = center_ref(r)                      in the centered mode only
  v[t]   = modswitch(r[t])                    in [0, 4096)
  stored = pack12(v[0 .. n])                  ceil(12 (n + 1) / 8) bytes, the pad nibble zero
  back   = v[t] << 52
  client : phase = (v[n] - sum v[i] s[i]) mod 4096, value = round(phase / 128) mod 16

Never used by the product."""
import struct

import numpy as np

import compress_ref as R
import ks_ref
import ms_center_ref
import seeded_key_ref as K

KIND_LIST = 13
HEADER = 32 + 36 + 12  # frame, main params, form / count / B
RADIX, BIGUINT = 0, 1
MS_PAD_WORD = 0xA5A55A5AC3C33C3C
N_LIST = (1, 2, 15, 16, 255, 256, 833, 834, 2047, 2048)
EDGE_TOPS = (0, 0x7FF, 0x800, 0xFFF)
EDGE_LOWS = (0, (1 << 51) - 1, 1 << 51, (1 << 51) + 1, (1 << 52) - 1)


def row_bytes(n):
    return (12 * (n + 1) + 7) // 8


def ws_stride(n):
    return (n + 1 + 7) // 8 * 8


def wire_len(n, B):
    return HEADER + B * (1 + row_bytes(n))


def main_bytes(n, grouping=1):
    return struct.pack("<9I", n, 23, 3, 5, 45, 17, 4, 4, grouping)


def edge_words():
    """every top-12-bit pattern of EDGE_TOPS over every low part of EDGE_LOWS: below, at and above the rounding bit;
    0xFFF over 2^51 rounds up and wraps to 0"""
    return np.array([(t << 52) | lo for t in EDGE_TOPS for lo in EDGE_LOWS], np.uint64)


def edge_rows(n, count, seed=0):
    """(count, n + 1) words: row 0 cycles through the edge words, row 1 is all ones, row 2 zero, the rest uniform
    with the edge words sprinkled in at a stride co-prime to 8"""
    rng = np.random.default_rng(0x5317C + 4099 * n + seed)
    rows = rng.integers(0, 1 << 64, (count, n + 1), dtype=np.uint64)
    e = edge_words()
    rows[0] = np.resize(e, n + 1)
    if count > 1:
        rows[1] = np.uint64((1 << 64) - 1)
    if count > 2:
        rows[2] = 0
    for b in range(3, count):
        rows[b, b % 7::7] = np.resize(np.roll(e, b), len(rows[b, b % 7::7]))
    return rows


def values(rows, n):
    """(count, n + 1) 12-bit values of rows of any stride >= n + 1"""
    return ks_ref.modswitch(np.asarray(rows, np.uint64)[:, :n + 1]).astype(np.uint32)


def pack_rows(rows, n):
    """list of bytes, one stored row each"""
    return [R.pack12(v) for v in values(rows, n)]


def unpack_rows(packed, n, stride=None):
    """(count, stride) words: value << 52, MS_PAD_WORD above word n"""
    stride = n + 1 if stride is None else stride
    out = np.full((len(packed), stride), MS_PAD_WORD, np.uint64)
    for b, p in enumerate(packed):
        out[b, :n + 1] = R.unpack12(p[:row_bytes(n)], n + 1).astype(np.uint64) << np.uint64(52)
    return out


def small_rows(ksk, n, cts, centered):
    """the keyswitched (and, in the centered mode, centered) rows of (B, 2049) blocks: (B, n + 1) words"""
    r = ks_ref.keyswitch_np(ksk, n, np.asarray(cts, np.uint64).reshape(-1, ks_ref.BIG_CT))
    return ms_center_ref.center_ref(r, n) if centered else r


def compress(ksk, n, cts, centered):
    """list of bytes, one stored row per block"""
    return pack_rows(small_rows(ksk, n, cts, centered), n)


def wire(main_params_bytes, form, count, degrees, rows):
    """the serialized list (kind 13) from its parts"""
    payload = main_params_bytes + struct.pack("<3I", form, count, len(degrees)) + bytes(degrees) + b"".join(rows)
    return K.frame(KIND_LIST, payload)


def parse_list(n, blob):
    """(form, count, degrees, [stored rows as bytes]) of a serialized list"""
    form, count, B = struct.unpack_from("<3I", blob, HEADER - 12)
    assert len(blob) == wire_len(n, B)
    degrees = list(blob[HEADER:HEADER + B])
    off, rb = HEADER + B, row_bytes(n)
    return form, count, degrees, [blob[off + i * rb:off + (i + 1) * rb] for i in range(B)]


def decrypt_values(rows, n, lwe_sk):
    """per stored row: the decoded value and the phase mod 4096"""
    s = np.asarray(lwe_sk, np.int64)
    vals, phases = [], []
    for p in rows:
        v = R.unpack12(p, n + 1).astype(np.int64)
        ph = int(v[n] - (v[:n] * s).sum()) % 4096
        phases.append(ph)
        vals.append(((ph + 64) >> 7) % 16)
    return vals, phases


# ------------------------------------------------------------------ the re-keying key
KIND_REKEY = 14
STREAM_REKEY = 112
KSK_ROWS = 2048 * 5


def rekey_ksk(seed32, noise_words, s_dst, S_src, lwe_noise_log2=45):
    """the expanded re-keying KSK, (2048 * 5, n_dst + 1): row r = j 5 + l has the stream's words [2048 r, 2048 r +
    n_dst) as its mask and <mask, s_dst> + (S_src[j] << (64 - 3 (l + 1))) + TUniform(noise_words[r]) as its body"""
    s_dst = np.asarray(s_dst, np.uint64)
    n = s_dst.size
    out = np.zeros((KSK_ROWS, n + 1), np.uint64)
    out[:, :n] = K.row_masks(seed32, STREAM_REKEY, KSK_ROWS, n)
    r = np.arange(KSK_ROWS)
    with np.errstate(over="ignore"):
        body = (out[:, :n] * s_dst[None, :]).sum(axis=1, dtype=np.uint64)
        body += np.asarray(S_src, np.uint64)[r // 5] << (np.uint64(64) - np.uint64(3) * (r % 5 + 1).astype(np.uint64))
        body += K.tuniform(noise_words, lwe_noise_log2)
    out[:, n] = body
    return out


def rekey_wire(main_params_bytes, seed32, bodies):
    return K.frame(KIND_REKEY, main_params_bytes + seed32 + np.asarray(bodies, "<u8").tobytes())


def assemble(vals, form, bits):
    """radix: sum v_k 4^k mod 2^bits; BigUintFHE: the same per 16-block limb mod 2^32, limb i at bits 32 i"""
    if form == RADIX:
        return R.assemble(vals, bits)
    return sum(R.assemble(vals[i:i + 16], 32) << (2 * i) for i in range(0, len(vals), 16))
