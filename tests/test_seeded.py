"""Seeded (compressed) ciphertexts on the host: tfhe-rs' CompressedFheUint::try_encrypt / decompress
(include/fhe_rocm.h "seeded (compressed) ciphertexts", csrc/keys.cpp encrypt_seeded / expand_seeded_host).

The definition is checked word for word against this file's own RFC 8439 block function in numpy: it
uses neither the engine's nor the oracle's stream code.
  masks   block i = u64 words [2048 i, 2048 (i + 1)) of ChaCha20(key = the 32 seed bytes as little-endian
          words, nonce = {101, "ROCM", 0}), block counter from 0
  bodies  mask . s + delta m + (u + c - 2^17), u / c from the next u64 of the client key's encryption
          stream (fhe_client_key_seed_encryption(S, T): key {S lo, S hi, "FHES", 0...}, nonce {T, "ROCM", 0})
No GPU, no context."""
import struct

import numpy as np
import pytest

from fhe_sign import (ClientKey, CompressedBigUintFHE, CompressedFheUint, CompressedFheUint32, CompressedFheUint256,
                      ServerKey, default_params, generate_keys)
from fhe_sign._lib import FheError

SEED = 0x5EED0C
ENC_SEED, ENC_STREAM = 0x0123456789ABCDEF, 100
MASK_SEED = bytes(range(7, 39))
ROCM = 0x524F434D
FHES = 0x46484553
NOISE_LOG2 = 17
DELTA = 1 << 59  # 2^63 / (message 4 x carry 4)
M64 = (1 << 64) - 1
SEED_OFF = 32 + 9 * 4 + 8  # frame header, params, form + count


# ------------------------------------------------------------------ the test's own ChaCha20
def _rotl(v, c):
    return (v << np.uint32(c)) | (v >> np.uint32(32 - c))


def chacha_blocks(key8, nonce3, counters):
    """RFC 8439 block function for an array of block counters -> (len, 16) uint32"""
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


def mask_key(seed32):
    return struct.unpack("<8I", seed32)


ENC_KEY = (ENC_SEED & 0xFFFFFFFF, ENC_SEED >> 32, FHES, 0, 0, 0, 0, 0)
ENC_NONCE = (ENC_STREAM, ROCM, 0)


def tuniform(x, b=NOISE_LOG2):
    u = x & ((1 << (b + 1)) - 1)
    c = (x >> (b + 1)) & 1
    return u + c - (1 << b)


def dot(mask, sk):
    return int((mask * sk).sum(dtype=np.uint64))  # wraps mod 2^64


def expected(seed32, sk, digits, enc_first=0):
    """(nblocks, 2049) by the definition above, block by block"""
    nb = len(digits)
    out = np.zeros((nb, 2049), np.uint64)
    noise = stream_u64(ENC_KEY, ENC_NONCE, enc_first, nb) if nb else []
    for i, m in enumerate(digits):
        mask = stream_u64(mask_key(seed32), (101, ROCM, 0), 2048 * i, 2048)
        out[i, :2048] = mask
        out[i, 2048] = (dot(mask, sk) + DELTA * m + tuniform(int(noise[i]))) & M64
    return out


def digits_of(value, nblocks):
    return [(value >> (2 * i)) & 3 for i in range(nblocks)]


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


@pytest.fixture(scope="module")
def keys():
    ck, _ = generate_keys(seed=SEED)
    return ck, ck.export()[1]


def fresh(ck):
    ck.seed_encryption(ENC_SEED, ENC_STREAM)
    return ck


VALUE = int.from_bytes(np.random.default_rng(20).bytes(32), "little") | 1 << 255


# ------------------------------------------------------------------ the definition, word for word
@pytest.mark.parametrize("bits", [2, 4, 10, 32, 256])  # 1, 2, 5, 16 and 128 blocks (128: the threaded path)
def test_radix_words_equal_the_definition(keys, bits):
    ck, sk = keys
    v = VALUE % (1 << bits)
    c = CompressedFheUint.try_encrypt(v, fresh(ck), bits=bits, seed=MASK_SEED)
    assert (c.bits, c.nblocks) == (bits, bits // 2)
    got = c.expand_host()
    assert got.shape == (bits // 2, 2049)
    assert np.array_equal(got, expected(MASK_SEED, sk, digits_of(v, bits // 2)))


def test_biguint_words_equal_the_definition(keys):
    ck, sk = keys
    v = VALUE % (1 << 96) | 1 << 95  # three limbs, 48 blocks, limb 0 first
    c = CompressedBigUintFHE.new(v, fresh(ck), seed=MASK_SEED)
    assert (len(c), c.nblocks) == (3, 48)
    assert np.array_equal(c.expand_host(), expected(MASK_SEED, sk, digits_of(v, 48)))


def test_words_at_lwe_dimension_16():
    """the big-key ciphertext does not depend on n; the params field does"""
    p = default_params()
    p.lwe_dimension = 16
    ck, _ = generate_keys(p, seed=SEED)
    sk = ck.export()[1]
    c = CompressedFheUint.try_encrypt(0x2D9, fresh(ck), bits=10, seed=MASK_SEED)
    assert np.array_equal(c.expand_host(), expected(MASK_SEED, sk, digits_of(0x2D9, 5)))
    blob = c.serialize()
    assert struct.unpack_from("<I", blob, 32)[0] == 16
    assert np.array_equal(CompressedFheUint.deserialize(blob).expand_host(), c.expand_host())


# ------------------------------------------------------------------ decryption
def test_expanded_blocks_decrypt(keys):
    ck, sk = keys
    c = CompressedFheUint256.try_encrypt(VALUE, fresh(ck), seed=MASK_SEED)
    cts = c.expand_host()
    for i, m in enumerate(digits_of(VALUE, 128)):
        assert ck.decrypt_block(cts[i]) == m
        phase = (int(cts[i, 2048]) - dot(cts[i, :2048], sk)) & M64
        err = (phase - DELTA * m) & M64
        err -= (err >> 63) << 64
        assert abs(err) <= 1 << NOISE_LOG2


# ------------------------------------------------------------------ stream accounting
@pytest.mark.parametrize("nb", [1, 5, 128])
def test_encryption_stream_advances_one_word_per_block(keys, nb):
    ck, sk = keys
    before = fresh(ck).serialize()
    CompressedFheUint.try_encrypt(3, ck, bits=2 * nb, seed=MASK_SEED)
    after = ck.encrypt_block(5)

    def block_at(first):  # fhe_encrypt_block with the stream at u64 word `first`: 2048 masks, then the noise word
        w = stream_u64(ENC_KEY, ENC_NONCE, first, 2049)
        return np.append(w[:2048], np.uint64((dot(w[:2048], sk) + DELTA * 5 + tuniform(int(w[2048]))) & M64))

    # the copy taken before the seeded encryption stands at word 0; the key itself at word nb
    assert np.array_equal(ClientKey.deserialize(before).encrypt_block(5), block_at(0))
    assert np.array_equal(after, block_at(nb))


# ------------------------------------------------------------------ seeds
def test_default_seed_is_entropy_and_a_given_seed_is_kept(keys):
    ck, _ = keys
    a = CompressedFheUint32.try_encrypt(9, ck).serialize()
    b = CompressedFheUint32.try_encrypt(9, ck).serialize()
    sa, sb = a[SEED_OFF:SEED_OFF + 32], b[SEED_OFF:SEED_OFF + 32]
    assert sa != sb and sa != bytes(32) and sb != bytes(32)
    g = CompressedFheUint32.try_encrypt(9, ck, seed=MASK_SEED).serialize()
    assert g[SEED_OFF:SEED_OFF + 32] == MASK_SEED
    with pytest.raises(ValueError):
        CompressedFheUint32.try_encrypt(9, ck, seed=b"short")


# ------------------------------------------------------------------ format
def test_round_trip_and_size(keys):
    ck, _ = keys
    for bits in (2, 32, 256):
        c = CompressedFheUint.try_encrypt(VALUE % (1 << bits), fresh(ck), bits=bits, seed=MASK_SEED)
        blob = c.serialize()
        assert len(blob) <= 128 + 8 * (bits // 2)
        d = CompressedFheUint.deserialize(blob)
        assert type(d) is type(c) and d.bits == bits
        assert np.array_equal(d.expand_host(), c.expand_host())
        assert d.serialize() == blob
    assert len(blob) * 1000 <= 128 * 2049 * 8
    b = CompressedBigUintFHE.new(VALUE, fresh(ck), seed=MASK_SEED)
    d = CompressedBigUintFHE.deserialize(b.serialize())
    assert len(d) == 8 and np.array_equal(d.expand_host(), b.expand_host())
    with pytest.raises(FheError):
        CompressedFheUint.deserialize(b.serialize())  # the other form
    with pytest.raises(FheError):
        CompressedBigUintFHE.deserialize(blob)


def test_zero_limbs(keys):
    ck, _ = keys
    z = CompressedBigUintFHE.new(0, ck, seed=MASK_SEED)
    assert (len(z), z.nblocks) == (0, 0) and z.expand_host().shape == (0, 2049)
    d = CompressedBigUintFHE.deserialize(z.serialize())
    assert (len(d), d.nblocks) == (0, 0) and d.serialize() == z.serialize()


# ------------------------------------------------------------------ refusals
def test_rejects_every_corruption_and_truncation(keys):
    ck, _ = keys
    blob = CompressedFheUint.try_encrypt(2, ck, bits=4, seed=MASK_SEED).serialize()
    for i in range(0, len(blob), 7):
        bad = bytearray(blob)
        bad[i] ^= 0x01
        with pytest.raises(FheError):
            CompressedFheUint.deserialize(bytes(bad))
    one = CompressedFheUint.try_encrypt(2, ck, bits=2, seed=MASK_SEED).serialize()
    for n in range(len(one)):
        with pytest.raises(FheError):
            CompressedFheUint.deserialize(one[:n])
    with pytest.raises(FheError):
        CompressedFheUint.deserialize(one + b"\0")


def test_rejects_other_kinds(keys):
    ck, _ = keys
    blob = CompressedFheUint32.try_encrypt(1, ck, seed=MASK_SEED).serialize()
    payload = blob[32:]
    for kind in (1, 2, 3, 4):  # client key, server key, radix, BigUintFHE frames
        with pytest.raises(FheError, match="kind"):
            CompressedFheUint.deserialize(frame(kind, payload))
    with pytest.raises(FheError, match="kind"):
        CompressedFheUint.deserialize(ck.serialize())
    with pytest.raises(FheError, match="kind"):
        ClientKey.deserialize(blob)
    with pytest.raises(FheError, match="kind"):
        ServerKey.deserialize(blob)
    assert CompressedFheUint.deserialize(frame(5, payload)).serialize() == blob  # the crafting itself is sound


def test_rejects_bad_widths_and_counts(keys):
    ck, _ = keys
    for bits in (3, 4098, 0):
        with pytest.raises(FheError):
            CompressedFheUint.try_encrypt(1, ck, bits=bits or None, seed=MASK_SEED)
    blob = CompressedFheUint.try_encrypt(1, ck, bits=4, seed=MASK_SEED).serialize()
    form_off, count_off = 32 + 36, 32 + 40

    def with_fields(form, count, bodies=None):
        b = bytearray(blob)
        struct.pack_into("<II", b, form_off, form, count)
        if bodies is not None:
            b = b[:SEED_OFF + 32] + bytes(8 * bodies)
            struct.pack_into("<Q", b, 16, len(b) - 32)
        return refnv(bytes(b))

    assert CompressedFheUint.deserialize(with_fields(0, 4)).serialize() == blob
    with pytest.raises(FheError, match="num_bits"):
        CompressedFheUint.deserialize(with_fields(0, 3))                 # odd
    with pytest.raises(FheError, match="num_bits"):
        CompressedFheUint.deserialize(with_fields(0, 4098, bodies=2049))  # even, too wide, length consistent
    with pytest.raises(FheError, match="form"):
        CompressedFheUint.deserialize(with_fields(2, 4))
    for count in (2, 6):  # the checksum is right, so the count check itself is reached
        with pytest.raises(FheError, match="inconsistent"):
            CompressedFheUint.deserialize(with_fields(0, count))
    with pytest.raises(FheError, match="inconsistent"):
        CompressedBigUintFHE.deserialize(with_fields(1, 1))              # 16 blocks claimed, 2 present
    # more than 2^24 blocks: refused from the header alone, nothing of that size is allocated
    for limbs in ((1 << 20) + 1, 0xFFFFFFFF):
        with pytest.raises(FheError, match=r"2\^24"):
            CompressedBigUintFHE.deserialize(with_fields(1, limbs))
    with pytest.raises(FheError, match="inconsistent"):
        CompressedBigUintFHE.deserialize(with_fields(1, 1 << 20))        # exactly 2^24 blocks: legal count, no payload
