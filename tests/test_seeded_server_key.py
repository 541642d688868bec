"""The seeded (compressed) server key on the host: tfhe-rs' CompressedServerKey::new / decompress
(include/fhe_rocm.h "seeded (compressed) server key", csrc/keys.cpp generate_seeded_server_key /
expand_seeded_server_key_host, csrc/serial.cpp kind 6).

Checked word for word against tests/seeded_key_ref.py's own RFC 8439 block function in numpy:
  masks   KSK row r = j 5 + l: word t < n = u64 word 2048 r + t of ChaCha20(key = the 32 seed bytes, nonce
          {102, "ROCM", 0}); BSK GGSW q, row rho: coefficient m = u64 word 2048 (2 q + rho) + m, nonce id 103
  noise   10240 + 4096 ggsw words of the client key's encryption stream, KSK rows first, then (q, rho, m)
  bodies  KSK <mask, s> + (S_j << (64 - 3 (l + 1))) + e;  BSK A * S + e, row 1: + g m_q at coefficient 0,
          row 0: - g m_q S_t at every coefficient t (g = 2^41); the mask of row 0 is the raw stream
and, through the untouched oracle re-keyed to the expanded words, for validity: every block value
bootstraps to f(m).  No GPU, no context."""
import struct

import numpy as np
import pytest

import seeded_key_ref as K
from fhe_sign import ClientKey, CompressedServerKey, ServerKey, default_params, generate_keys, multi_bit_params
from fhe_sign._lib import FheError
from lwe_dims import CLASSIC, MULTIBIT, product_params

SEED = 0x5EEDC0DE
ENC_SEED, ENC_STREAM = 0x0FEDCBA987654321, 100
MASK_SEED = bytes(range(11, 43))
SETS = [(1, CLASSIC), (7, CLASSIC), (8, CLASSIC), (9, CLASSIC), (16, CLASSIC), (2, MULTIBIT), (16, MULTIBIT)]
DELTA = 1 << 59


def set_id(s):
    return f"n{s[0]}-{'mb' if s[1] == MULTIBIT else 'cl'}"


class Case:
    """a client key with a known encryption stream, its seeded server key and the expanded words"""

    def __init__(self, n, g):
        self.n, self.g = n, g
        self.ngg = K.ggsw_count(n, g)
        self.ck, _ = generate_keys(product_params(n, g), seed=SEED)
        self.ck.seed_encryption(ENC_SEED, ENC_STREAM)
        self.before = self.ck.serialize()
        self.ssk = CompressedServerKey.new(self.ck, seed=MASK_SEED)
        self.blob = self.ssk.serialize()
        self.seed, self.kb, self.bb = K.parse(self.blob, n, g)
        self.ksk, self.bsk = self.ssk.decompress().export()
        self.lwe, self.glwe = self.ck.export()
        self.noise_words = K.KSK_ROWS + 2 * self.ngg * K.N


@pytest.fixture(scope="module", params=SETS, ids=set_id)
def case(request):
    return Case(*request.param)


# ------------------------------------------------------------------ masks
def test_masks_equal_the_streams(case):
    n, ngg = case.n, case.ngg
    assert case.seed == MASK_SEED
    ksk = case.ksk.reshape(K.KSK_ROWS, n + 1)
    assert np.array_equal(ksk[:, :n], K.row_masks(MASK_SEED, K.STREAM_KSK, K.KSK_ROWS, n))  # every row
    assert np.array_equal(ksk[:, n], case.kb)
    bsk = case.bsk.reshape(2 * ngg, 2, K.N)
    # every row, row 0 of each GGSW included: the raw stream, no gadget in A[0]
    assert np.array_equal(bsk[:, 0], K.row_masks(MASK_SEED, K.STREAM_BSK, 2 * ngg, K.N))
    assert np.array_equal(bsk[:, 1], case.bb)


# ------------------------------------------------------------------ bodies
def test_bodies_word_for_word(case):
    n, ngg = case.n, case.ngg
    noise = K.stream_u64(K.seed_key(ENC_SEED), (ENC_STREAM, K.ROCM, 0), 0, case.noise_words)
    s, S = case.lwe, case.glwe
    r = np.arange(K.KSK_ROWS)
    shift = (64 - K.KS_BASE_LOG * (r % K.KS_LEVEL + 1)).astype(np.uint64)
    masks = K.row_masks(MASK_SEED, K.STREAM_KSK, K.KSK_ROWS, n)
    want = (masks * s[None, :]).sum(axis=1, dtype=np.uint64) + (S[r // K.KS_LEVEL] << shift) \
        + K.tuniform(noise[:K.KSK_ROWS], K.LWE_NOISE_LOG2)
    assert np.array_equal(case.kb, want)

    A = K.row_masks(MASK_SEED, K.STREAM_BSK, 2 * ngg, K.N)
    B = K.negacyclic_binary(A, S) + K.tuniform(noise[K.KSK_ROWS:], K.GLWE_NOISE_LOG2).reshape(2 * ngg, K.N)
    g = np.uint64(1 << (64 - K.PBS_BASE_LOG))
    for q, m in enumerate(K.ggsw_messages(s, n, case.g)):
        B[2 * q] -= g * np.uint64(m) * S      # row 0: the gadget lives in the body, on every coefficient
        B[2 * q + 1, 0] += g * np.uint64(m)   # row 1
    assert np.array_equal(case.bb, B)


# ------------------------------------------------------------------ stream accounting
def _block_at(first, sk, value=5):
    """fhe_encrypt_block with the encryption stream at u64 word `first`: 2048 masks, then the noise word"""
    w = K.stream_u64(K.seed_key(ENC_SEED), (ENC_STREAM, K.ROCM, 0), first, 2049)
    body = (w[:2048] * sk).sum(dtype=np.uint64, keepdims=True) + np.uint64(DELTA * value) \
        + K.tuniform(w[2048], K.GLWE_NOISE_LOG2)
    return np.append(w[:2048], body)


def test_encryption_stream_advances_by_the_noise_words(case):
    S = case.glwe
    saved = case.ck.serialize()  # after the generation
    assert np.array_equal(case.ck.encrypt_block(5), _block_at(case.noise_words, S))
    assert np.array_equal(ClientKey.deserialize(saved).encrypt_block(5), _block_at(case.noise_words, S))
    # a key serialized before: the same object, then the same position
    early = ClientKey.deserialize(case.before)
    assert np.array_equal(ClientKey.deserialize(case.before).encrypt_block(5), _block_at(0, S))
    assert CompressedServerKey.new(early, seed=MASK_SEED).serialize() == case.blob
    assert np.array_equal(early.encrypt_block(5), _block_at(case.noise_words, S))


# ------------------------------------------------------------------ validity, through the oracle
@pytest.mark.parametrize("g", [CLASSIC, MULTIBIT], ids=["cl", "mb"])
def test_expanded_key_bootstraps_in_the_oracle(g):
    """the row-0 form is right: the oracle (its own keyswitch, blind rotation and sample extraction),
    with the expanded words in place of its key, maps every block value through both tables"""
    ck, _ = generate_keys(product_params(16, g), seed=SEED)
    ksk, bsk = CompressedServerKey.new(ck, seed=MASK_SEED).decompress().export()
    ok = K.rekeyed_oracle(SEED, 16, g, ksk, bsk)
    lwe, glwe = ck.export()
    assert np.array_equal(lwe, ok.lwe_sk) and np.array_equal(glwe, ok.glwe_sk)
    r = ok.rng(3)
    cts = np.stack([ok.encrypt(r, m) for m in range(16)])
    for table in (list(range(16)), [(5 * m + 3) % 16 for m in range(16)]):
        out = ok.pbs_batch(cts, ok.make_lut(table)[None, :], np.zeros(16, np.uint32))
        assert [ok.decrypt(o) for o in out] == table
        assert [ck.decrypt_block(o) for o in out] == table


# ------------------------------------------------------------------ seeds
def test_default_seed_is_entropy():
    ck, _ = generate_keys(product_params(1), seed=SEED)
    a, b = (CompressedServerKey.new(ck).serialize()[K.SEED_OFF:K.BODY_OFF] for _ in range(2))
    assert a != b and a != bytes(32) and b != bytes(32)
    with pytest.raises(ValueError):
        CompressedServerKey.new(ck, seed=b"short")


# ------------------------------------------------------------------ format
def test_length_round_trip_and_params(case):
    assert len(case.blob) == K.wire_len(case.n, case.g)
    d = CompressedServerKey.deserialize(case.blob)
    assert d.serialize() == case.blob
    assert (d.params.lwe_dimension, d.params.grouping) == (case.n, case.g)
    full = d.decompress()
    assert full.serialize() == case.ssk.decompress().serialize()
    assert ServerKey.deserialize(full.serialize()).serialize() == full.serialize()  # an ordinary server key


@pytest.mark.parametrize("params,want", [(default_params, 27_410_532), (multi_bit_params, 100 + 8 * (10240 + 4096 * 1251))],
                         ids=["cl", "mb"])
def test_length_at_the_default_parameters(params, want):
    ck, _ = generate_keys(params(), seed=SEED)
    blob = CompressedServerKey.new(ck, seed=MASK_SEED).serialize()
    assert len(blob) == want == K.wire_len(834, params().grouping)
    assert CompressedServerKey.deserialize(blob).serialize() == blob


def test_refusals_before_allocation():
    ck, sk = generate_keys(product_params(1), seed=SEED)
    blob = CompressedServerKey.new(ck, seed=MASK_SEED).serialize()
    assert len(blob) == 100 + 8 * (10240 + 4096)
    # truncation at every field boundary: header fields, params, seed, KSK bodies, BSK bodies
    for cut in (0, 8, 12, 16, 24, 32, 36, 64, 68, 99, 100, 100 + 8 * 10240, len(blob) - 8, len(blob) - 1):
        with pytest.raises(FheError):
            CompressedServerKey.deserialize(blob[:cut])
    with pytest.raises(FheError):
        CompressedServerKey.deserialize(blob + b"\0")
    # one flipped byte: header, params, seed, first / last body
    for i in (0, 9, 13, 17, 25, 33, 70, 101, 100 + 8 * 10240 + 3, len(blob) - 1):
        bad = bytearray(blob)
        bad[i] ^= 0x40
        with pytest.raises(FheError):
            CompressedServerKey.deserialize(bytes(bad))
    # a wrong kind, both directions
    with pytest.raises(FheError, match="kind"):
        CompressedServerKey.deserialize(sk.serialize())
    with pytest.raises(FheError, match="kind"):
        ServerKey.deserialize(blob)
    with pytest.raises(FheError, match="kind"):
        CompressedServerKey.deserialize(K.frame(2, blob[32:]))
    assert CompressedServerKey.deserialize(K.frame(6, blob[32:])).serialize() == blob  # the crafting is sound
    # one word longer or shorter, length field and checksum right: the formula itself refuses
    for payload in (blob[32:] + bytes(8), blob[32:-8]):
        with pytest.raises(FheError, match="payload length"):
            CompressedServerKey.deserialize(K.frame(6, payload))
    # parameters that claim a larger key than the payload backs (n = 2: twice the BSK), or that no kernel takes
    for off, v, why in ((0, 2, "payload length"), (1, 22, "unsupported parameters"), (3, 4, "unsupported parameters")):
        bad = bytearray(blob)
        struct.pack_into("<I", bad, 32 + 4 * off, v)
        with pytest.raises(FheError, match=why) as e:
            CompressedServerKey.deserialize(K.refnv(bad))
        assert e.value.code == -1
