"""Test-only numpy restatement of the compressed computed ciphertexts (include/fhe_rocm.h "compressed
computed ciphertexts"), shared by tests/test_compress.py and tests/test_compress_gpu.py.  Written from the
formulas, it uses nothing of the product:

  T_i   = (0, .., 0, b_i X^0) - sum_{j < 2048} sum_{l < ell} d[i, j, l] PKSK[j][l]   (k' + 1 polynomials, mod 2^64)
  G_g   = sum_{i in g} X^t T_i        (negacyclic: what leaves the top re-enters at the bottom with a minus)
  store = modswitch12(mask coefficients of G_g, body coefficients 0 .. b_g - 1),  b_g = min(L, B - g L)
  modswitch12(x) = (((x >> 51) + 1) >> 1) & 4095

Never used by the product."""
import struct
from collections import namedtuple

import numpy as np

import seeded_key_ref as K

N_BIG = 2048
BIG_CT = N_BIG + 1
M64 = (1 << 64) - 1
HEADER = 32 + 36 + 28 + 12  # frame, main params, compression params, form / count / B
KIND_PRIVATE, KIND_KEY, KIND_LIST = 7, 8, 9
PBS_BASE_LOG, GLWE_NOISE_LOG2 = 23, 17

CP = namedtuple("CP", "k N L beta ell noise")
SMALL_A = CP(1, 8, 8, 4, 4, 42)
SMALL_B = CP(2, 16, 16, 3, 5, 42)
DEFAULT = CP(4, 256, 256, 4, 4, 42)


def cols(cp):
    return (cp.k + 1) * cp.N


def stream_words(cp):
    """u64 words of the client key's encryption stream the key generation consumes"""
    kn = cp.k * cp.N
    return kn + N_BIG * cp.ell * cols(cp) + 8192 * kn


def glwe_bytes(cp, nb):
    return (12 * (cp.k * cp.N + nb) + 7) // 8


def bodies_of(cp, B):
    return [min(cp.L, B - g * cp.L) for g in range((B + cp.L - 1) // cp.L)]


def wire_len(cp, B):
    return HEADER + B + sum(glwe_bytes(cp, nb) for nb in bodies_of(cp, B))


# ------------------------------------------------------------------ digits
def digits(a, beta, ell):
    """balanced digits of the words `a`: int64 (..., ell), level 0 the most significant.  Round to the top
    beta ell bits, add 2^(beta - 1) to every digit, take the base-2^beta digits, subtract 2^(beta - 1)
    again; the carry out of the top digit falls off (tests/ks_ref.py digits, generalised)"""
    a = np.asarray(a, np.uint64)
    bl = beta * ell
    v = (((a >> np.uint64(63 - bl)) + np.uint64(1)) >> np.uint64(1)) & np.uint64((1 << bl) - 1)
    bias = sum((1 << (beta - 1)) << (beta * i) for i in range(ell))
    w = v + np.uint64(bias)
    sh = np.uint64(beta) * np.arange(ell - 1, -1, -1, dtype=np.uint64)
    return ((w[..., None] >> sh) & np.uint64((1 << beta) - 1)).astype(np.int64) - (1 << (beta - 1))


def digits_by_carry(a, beta, ell):
    """the same digits by the decomposer's own loop (least significant first, carry upward), for one word"""
    bl = beta * ell
    v = (((int(a) >> (63 - bl)) + 1) >> 1) & ((1 << bl) - 1)
    out = []
    for _ in range(ell):
        d = v & ((1 << beta) - 1)
        v >>= beta
        if d >= 1 << (beta - 1):
            d -= 1 << beta
            v += 1
        out.append(d)
    return out[::-1]


def edge_rows(beta, ell):
    """big LWE rows that put the rounding bit and every carry chain at their edges (tests/ks_ref.py
    edge_rows, re-made for (beta, ell)): (0) a set of top-bit patterns over low parts below, at and above
    the rounding bit 2^(63 - beta ell), body 0; (1) every digit 2^(beta - 1) -> -2^(beta - 1) with a carry
    through all levels, body 2^63; (2) all ones: rounds up and wraps to zero digits; (3) a zero mask"""
    bl = beta * ell
    rb = 63 - bl  # the rounding bit's position
    half_all = sum((1 << (beta - 1)) << (beta * i) for i in range(ell))
    below_all = sum(((1 << (beta - 1)) - 1) << (beta * i) for i in range(ell))
    carry_all = below_all + 1  # digits (h - 1, .., h - 1, h): the lowest becomes -h and carries, so does every next
    pats = (0, (1 << bl) - 1, 1 << (bl - 1), (1 << (bl - 1)) - 1, half_all, below_all, carry_all)
    lows = (0, (1 << rb) - 1, 1 << rb, (1 << rb) + 1, (1 << (rb + 1)) - 1)
    words = [((p << (rb + 1)) | lo) & M64 for p in pats for lo in lows]
    rows = np.zeros((4, BIG_CT), np.uint64)
    rows[0, :N_BIG] = np.resize(np.array(words, np.uint64), N_BIG)
    rows[1, :N_BIG] = np.uint64((carry_all << (rb + 1)) & M64)
    rows[1, N_BIG] = np.uint64(1 << 63)
    rows[2, :] = np.uint64(M64)
    rows[3, N_BIG] = np.uint64(0x0123456789ABCDEF)
    return rows


# ------------------------------------------------------------------ polynomials
def negacyclic_binary(a, s, n):
    """the rows of `a` (.., n) times the binary polynomial s mod X^n + 1, exact in Z / 2^64"""
    r = np.zeros_like(a)
    for j in np.flatnonzero(s):
        j = int(j)
        r[..., j:] += a[..., :n - j]
        if j:
            r[..., :j] -= a[..., n - j:]
    return r


def modswitch12(x):
    x = np.asarray(x, np.uint64)
    return ((((x >> np.uint64(51)) + np.uint64(1)) >> np.uint64(1)) & np.uint64(4095)).astype(np.uint32)


# ------------------------------------------------------------------ keys
def enc_stream(seed, stream, first, n):
    return K.stream_u64(K.seed_key(seed), (stream, K.ROCM, 0), first, n)


def secret_bits(cp, seed, stream):
    return enc_stream(seed, stream, 0, cp.k * cp.N) & np.uint64(1)


def pksk_rows(cp, seed, stream, sprime, S, rows):
    """rows (j, l) = divmod(r, ell) of the packing KSK, (len(rows), k' + 1, N'): the masks are the stream
    words, B = sum_c A_c * s'_c + e + (S_j << (64 - beta (l + 1))) at coefficient 0"""
    kn, c, total = cp.k * cp.N, cols(cp), N_BIG * cp.ell
    rows = np.asarray(rows)
    if len(rows) == total:  # every row: one pass over the stream
        w = enc_stream(seed, stream, kn, total * c).reshape(total, cp.k + 1, cp.N)
    else:
        w = np.stack([enc_stream(seed, stream, kn + int(r) * c, c).reshape(cp.k + 1, cp.N) for r in rows])
    out = w.copy()
    body = K.tuniform(w[:, cp.k].reshape(-1), cp.noise).reshape(len(rows), cp.N)
    for p in range(cp.k):
        body = body + negacyclic_binary(w[:, p], sprime[p * cp.N:(p + 1) * cp.N], cp.N)
    shift = (64 - cp.beta * (rows % cp.ell + 1)).astype(np.uint64)
    body[:, 0] += np.asarray(S, np.uint64)[rows // cp.ell] << shift
    out[:, cp.k] = body
    return out


def bsk_noise(cp, seed, stream, rows):
    """TUniform noise of the BSK rows r = 2 q + rho, (len(rows), 2048), and the masks' stream words"""
    kn = cp.k * cp.N
    first = kn + N_BIG * cp.ell * cols(cp)
    A = np.zeros((len(rows), N_BIG), np.uint64)
    e = np.zeros((len(rows), N_BIG), np.uint64)
    for i, r in enumerate(rows):
        w = enc_stream(seed, stream, first + r * 2 * N_BIG, 2 * N_BIG)
        A[i] = w[:N_BIG]
        e[i] = K.tuniform(w[N_BIG:], GLWE_NOISE_LOG2)
    return A, e


# ------------------------------------------------------------------ the packing keyswitch
def contract(d, pksk):
    """sum_k d[.., k] pksk[k, ..] mod 2^64 for int64 digits |d| <= 64: the key split into four 16-bit limbs,
    each product summed in float64 (|sum| <= 64 * 65535 * 65536 < 2^53: exact), recombined mod 2^64"""
    d = np.asarray(d, np.float64)
    out = np.zeros((d.shape[0], pksk.shape[1]), np.uint64)
    for limb in range(4):
        part = ((pksk >> np.uint64(16 * limb)) & np.uint64(0xFFFF)).astype(np.float64)
        s = np.rint(d @ part).astype(np.int64)
        out += s.astype(np.uint64) << np.uint64(16 * limb)
    return out


def contract_u64(d, pksk):
    """the same in wrapping uint64, directly (slow: the check of `contract` at small sizes)"""
    with np.errstate(over="ignore"):
        return np.dot(np.asarray(d, np.int64).astype(np.uint64), pksk)


def key_matrix(cp, pksk):
    """pksk flat [2048][ell][k' + 1][N'] as the matrix `contract` takes: row j ell + l, (k' + 1) N' columns"""
    return np.asarray(pksk, np.uint64).reshape(N_BIG * cp.ell, cols(cp))


def contraction_words(cp, pksk, cts):
    """P[i] = sum_{j, l} d[i, j, l] PKSK[j][l] mod 2^64, (B, (k' + 1) N'): the packing keyswitch before the
    sign, the bodies, the rotation and the rounding to 12 bits"""
    cts = np.asarray(cts, np.uint64).reshape(-1, BIG_CT)
    d = digits(cts[:, :N_BIG], cp.beta, cp.ell).reshape(cts.shape[0], N_BIG * cp.ell)
    return contract(d, key_matrix(cp, pksk))


# The device's byte planes, restated from the layout comment at the top of csrc/compress.hip: the key's rows in
# LEVEL-MAJOR order k = level * 2048 + j, cut into KT = 32 ell k-tiles of 64; its columns into tiles of 16, the
# last one padded with zero columns.  int8 [8 planes][column tiles][KT][64 lanes][16]: lane l of a fragment holds
# column l & 15 of its tile and the 16 bytes k = 64 kt + 16 (l >> 4) + jj.  Plane b holds the balanced bytes
# (tests/ks_ref.py byte_planes): word = sum_b plane_b 256^b mod 2^64 with plane_b in [-128, 128).
def plane_layout(cp, pksk):
    """the int8 array (8, column tiles, 32 ell, 64, 16) of the packing key pksk flat [2048][ell][k' + 1][N']"""
    c, KT = cols(cp), 32 * cp.ell
    tiles = (c + 15) // 16
    v = np.zeros((cp.ell * N_BIG, 16 * tiles), np.uint64)
    v[:, :c] = np.asarray(pksk, np.uint64).reshape(N_BIG, cp.ell, c).transpose(1, 0, 2).reshape(cp.ell * N_BIG, c)
    out = np.empty((8, tiles, KT, 64, 16), np.int8)
    for b in range(8):
        s = (v & np.uint64(255)).astype(np.int64)
        s[s >= 128] -= 256
        with np.errstate(over="ignore"):
            v = (v - s.astype(np.uint64)) >> np.uint64(8)
        # rows k = (kt, l >> 4, jj), columns (tile, l & 15) -> (tile, kt, lane = 16 (l >> 4) + (l & 15), jj)
        f = s.astype(np.int8).reshape(KT, 4, 16, tiles, 16).transpose(3, 0, 1, 4, 2)
        out[b] = f.reshape(tiles, KT, 64, 16)
    return out


def words_of_planes(cp, planes):
    """sum_b plane_b 256^b mod 2^64 read back out of the layout: (pksk flat [2048][ell][k' + 1][N'], the padding
    columns' bytes)"""
    c, KT = cols(cp), 32 * cp.ell
    tiles = (c + 15) // 16
    p = np.asarray(planes, np.int8).reshape(8, tiles, KT, 4, 16, 16)  # (b, tile, kt, l >> 4, l & 15, jj)
    p = p.transpose(0, 2, 3, 5, 1, 4).reshape(8, cp.ell * N_BIG, 16 * tiles)
    v = np.zeros(p.shape[1:], np.uint64)
    with np.errstate(over="ignore"):
        for b in range(8):
            v += p[b].astype(np.int64).astype(np.uint64) << np.uint64(8 * b)
    key = v[:, :c].reshape(cp.ell, N_BIG, c).transpose(1, 0, 2)
    return np.ascontiguousarray(key).reshape(-1), p[:, :, c:]


def pack_keyswitch(cp, pksk, cts):
    """pksk flat [2048][ell][k' + 1][N'], cts (B, 2049) -> per GLWE the uint32 array of its k' N' + b_g
    stored values"""
    cts = np.asarray(cts, np.uint64).reshape(-1, BIG_CT)
    B, c = cts.shape[0], cols(cp)
    key = np.asarray(pksk, np.uint64).reshape(N_BIG * cp.ell, c)
    d = digits(cts[:, :N_BIG], cp.beta, cp.ell).reshape(B, N_BIG * cp.ell)  # k = j ell + l, as the key's rows
    with np.errstate(over="ignore"):
        T = np.uint64(0) - contract(d, key)
        T[:, cp.k * cp.N] += cts[:, N_BIG]
    T = T.reshape(B, cp.k + 1, cp.N)
    out = []
    for g, nb in enumerate(bodies_of(cp, B)):
        G = np.zeros((cp.k + 1, cp.N), np.uint64)
        for t in range(nb):
            Ti = T[g * cp.L + t]
            G[:, t:] += Ti[:, :cp.N - t]
            if t:
                G[:, :t] -= Ti[:, cp.N - t:]
        out.append(modswitch12(np.concatenate([G[:cp.k].reshape(-1), G[cp.k, :nb]])))
    return out


def pack12(vals):
    """12-bit values, little-endian bit-contiguous, zero-padded to a byte"""
    vals = [int(v) for v in vals]
    acc = sum(v << (12 * i) for i, v in enumerate(vals))
    return acc.to_bytes((12 * len(vals) + 7) // 8, "little")


def unpack12(data, n):
    acc = int.from_bytes(data, "little")
    return np.array([(acc >> (12 * i)) & 4095 for i in range(n)], np.uint32)


def wire(cp, main_params_bytes, form, count, degrees, glwes):
    """the serialized list (kind 9) from its parts"""
    payload = main_params_bytes + struct.pack("<7I", cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12)
    payload += struct.pack("<3I", form, count, len(degrees)) + bytes(degrees) + b"".join(pack12(g) for g in glwes)
    return K.frame(KIND_LIST, payload)


def parse_list(cp, blob):
    """(form, count, degrees, [per GLWE uint32 values]) of a serialized list"""
    form, count, B = struct.unpack_from("<3I", blob, HEADER - 12)
    assert len(blob) == wire_len(cp, B)
    degrees = list(blob[HEADER:HEADER + B])
    off, glwes = HEADER + B, []
    for nb in bodies_of(cp, B):
        n = glwe_bytes(cp, nb)
        glwes.append(unpack12(blob[off:off + n], cp.k * cp.N + nb))
        off += n
    return form, count, degrees, glwes


# ------------------------------------------------------------------ the client's and the server's reading
def sample_extract(cp, glwe, t):
    """LWE (k' N' + 1 values mod 4096) of slot t: mask word (c, u) = A_c[t - u] for u <= t, -A_c[t - u + N']
    above; body = coefficient t of B"""
    kn = cp.k * cp.N
    A = np.asarray(glwe[:kn], np.int64).reshape(cp.k, cp.N)
    u = np.arange(cp.N)
    row = np.where(u <= t, A[:, (t - u) % cp.N], -A[:, (t - u) % cp.N]) % 4096
    return np.append(row.reshape(-1), int(glwe[kn + t])).astype(np.uint64)


def extract_rows(cp, glwes):
    """every block's sample-extracted row, each value << 52: what the unpack kernel writes"""
    rows = []
    for glwe in glwes:
        for t in range(len(glwe) - cp.k * cp.N):
            rows.append(sample_extract(cp, glwe, t) << np.uint64(52))
    return np.array(rows, np.uint64)


def decrypt_values(cp, glwes, sprime):
    """per block: phase = body - <mask, s'> mod 2^12, value = round(phase / 2^7) mod 16; and the phases"""
    vals, phases = [], []
    s = np.asarray(sprime, np.int64)
    for glwe in glwes:
        for t in range(len(glwe) - cp.k * cp.N):
            row = sample_extract(cp, glwe, t).astype(np.int64)
            ph = int(row[-1] - (row[:-1] * s).sum()) % 4096
            phases.append(ph)
            vals.append(((ph + 64) >> 7) % 16)
    return vals, phases


def assemble(vals, bits):
    """sum v_k 4^k mod 2^bits (blocks above degree 3 carry into their neighbours)"""
    return sum(v << (2 * k) for k, v in enumerate(vals)) % (1 << bits)


# ------------------------------------------------------------------ helpers of the tests
def oracle_decompress(ok, rows, table=None):
    """fho_blind_rotate + fho_sample_extract of an oracle.OracleKeys (re-keyed at n = k' N' with the
    decompression BSK) over sample-extracted rows: (len(rows), 2049) big LWE words"""
    import oracle

    lib = oracle.load()
    lut = ok.make_lut(list(range(16)) if table is None else table)
    rows = np.ascontiguousarray(rows, np.uint64)
    out = np.zeros((rows.shape[0], BIG_CT), np.uint64)
    glwe = np.zeros(2 * N_BIG, np.uint64)
    for i in range(rows.shape[0]):
        lib.fho_blind_rotate(ok.ref, rows[i].ctypes.data_as(oracle.u64p), lut.ctypes.data_as(oracle.u64p),
                             glwe.ctypes.data_as(oracle.u64p))
        lib.fho_sample_extract(glwe.ctypes.data_as(oracle.u64p), out[i].ctypes.data_as(oracle.u64p))
    return out


def _raw_blocks(cts, degree, noise):
    head = struct.pack("<BII", 1, degree, noise)
    return b"".join(head + np.ascontiguousarray(ct, "<u8").tobytes() for ct in cts)


def raw_radix_blob(main_params_bytes, cts, degree, noise=1):
    """a serialized FheUint (kind 3) around given block ciphertexts: how a test hands the engine blocks of
    any value, degree and noise"""
    cts = np.asarray(cts, np.uint64).reshape(-1, BIG_CT)
    return K.frame(3, main_params_bytes + struct.pack("<II", 2 * len(cts), len(cts)) + _raw_blocks(cts, degree, noise))


def raw_biguint_blob(main_params_bytes, cts, degree, noise=1):
    """the same as a BigUintFHE (kind 4): 16 blocks per limb"""
    cts = np.asarray(cts, np.uint64).reshape(-1, 16, BIG_CT)
    limbs = b"".join(struct.pack("<II", 32, 16) + _raw_blocks(limb, degree, noise) for limb in cts)
    return K.frame(4, main_params_bytes + struct.pack("<I", len(cts)) + limbs)
