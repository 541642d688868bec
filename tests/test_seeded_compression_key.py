"""The seeded (compressed) compression key on the host: tfhe-rs' CompressedCompressionKey /
CompressedDecompressionKey (include/fhe_rocm.h "seeded (compressed) compression key"; csrc/compress_host.cpp).
No GPU, no context.

Checked word for word, in wrapping uint64, against tests/seeded_compression_ref.py's numpy restatement at
(k', N', L, beta, ell) in {(1, 8, 8, 4, 4), (2, 8, 5, 7, 4), (2, 16, 16, 3, 5)} (every row), (4, 256, 256, 4, 4)
and (1, 2048, 4, 4, 1) (first, last and a few random rows: the numpy products of all rows would take
minutes): the bodies, the secret, the stream accounting, the host expansion; then compression and
decompression through the expanded key (the re-keyed oracle pins the body form of the BSK's row 0), the wire
format's length and every refusal, and the new kernel's resources."""
import os
import shutil
import struct

import numpy as np
import pytest

import compress_ref as R
import seeded_compression_ref as SC
import seeded_key_ref as K
from fhe_sign import (ClientKey, CompressedCiphertextList, CompressedCompressionKey, CompressionKey, CompressionKeys,
                      CompressionParams, generate_keys)
from fhe_sign._lib import FheError
from lwe_dims import product_params

SEED = 0x5EEDC0DE
ENC_SEED, ENC_STREAM = 0x0FEDCBA987654321, 100
MASK_SEED = bytes((37 * i + 11) % 256 for i in range(32))
SMALL = [R.SMALL_A, SC.MIXED, R.SMALL_B]
SETS = SMALL + [R.DEFAULT, SC.STRIDE]
RADIX = 0
DELTA = 1 << 59


def c_params(cp):
    return CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12)


def set_id(cp):
    return f"k{cp.k}N{cp.N}L{cp.L}b{cp.beta}l{cp.ell}"


class Case:
    """a client key with a known encryption stream and its seeded compression key.  The main LWE dimension
    is k' N' at the small sets, so that the oracle re-keyed at that dimension has the same big key."""

    def __init__(self, cp):
        self.cp = cp
        self.n = cp.k * cp.N if cp in SMALL else 16
        self.ck, _ = generate_keys(product_params(self.n), seed=SEED)
        self.ck.seed_encryption(ENC_SEED, ENC_STREAM)
        self.before = self.ck.serialize()
        self.priv, self.sck = CompressionKeys.generate_compressed(self.ck, c_params(cp), seed=MASK_SEED)
        self.after = self.ck.serialize()
        self.blob = self.sck.serialize()
        self.seed, self.pb, self.bb = SC.parse(cp, self.blob)
        self.sprime = self.priv.export()
        _, self.S = self.ck.export()
        self._key = None

    @property
    def key(self):
        """the host-expanded key"""
        if self._key is None:
            self._key = self.sck.decompress()
        return self._key

    def rows(self, total):
        if self.cp in SMALL:
            return list(range(total))
        rng = np.random.default_rng(total + self.cp.N)
        return sorted({0, 1, total - 2, total - 1} | {int(r) for r in rng.integers(0, total, 4)})


_cases = {}


def get(cp):
    if cp not in _cases:
        _cases[cp] = Case(cp)
    return _cases[cp]


@pytest.fixture(scope="module", params=SETS, ids=set_id)
def case(request):
    return get(request.param)


# ------------------------------------------------------------------ definition
def test_bodies_word_for_word(case):
    cp = case.cp
    assert case.seed == MASK_SEED
    rows = case.rows(R.N_BIG * cp.ell)
    _, want = SC.pksk_bodies(cp, ENC_SEED, ENC_STREAM, MASK_SEED, case.sprime, case.S, rows)
    assert np.array_equal(case.pb[rows], want)
    rows = case.rows(2 * cp.k * cp.N)
    _, want = SC.bsk_bodies(cp, ENC_SEED, ENC_STREAM, MASK_SEED, case.sprime, case.S, rows)
    assert np.array_equal(case.bb[rows], want)


def test_secret_is_the_full_generations(case):
    cp = case.cp
    assert np.array_equal(case.sprime, R.secret_bits(cp, ENC_SEED, ENC_STREAM))
    priv, _ = CompressionKeys.generate(ClientKey.deserialize(case.before), c_params(cp))
    assert priv.serialize() == case.priv.serialize()


def _block_at(first, sk, value=5):
    """fhe_encrypt_block with the encryption stream at u64 word `first`: 2048 masks, then the noise word"""
    w = R.enc_stream(ENC_SEED, ENC_STREAM, first, 2049)
    body = (w[:2048] * sk).sum(dtype=np.uint64, keepdims=True) + np.uint64(DELTA * value) \
        + K.tuniform(w[2048], R.GLWE_NOISE_LOG2)
    return np.append(w[:2048], body)


def test_encryption_stream_advances_by_the_documented_words(case):
    cp = case.cp
    words = cp.k * cp.N + 2048 * cp.ell * cp.N + 4096 * cp.k * cp.N
    assert words == SC.stream_words(cp)
    if cp is R.DEFAULT:
        assert words == 6_292_480
    assert np.array_equal(ClientKey.deserialize(case.after).encrypt_block(5), _block_at(words, case.S))


def test_same_seed_and_stream_state_same_bytes(case):
    early = ClientKey.deserialize(case.before)
    priv, sck = CompressionKeys.generate_compressed(early, c_params(case.cp), seed=MASK_SEED)
    assert priv.serialize() == case.priv.serialize()
    assert sck.serialize() == case.blob
    assert early.serialize() == case.after


def test_os_entropy_seeds_differ():
    cp = R.SMALL_A
    blobs = []
    for _ in range(2):
        ck = ClientKey.deserialize(get(cp).before)
        blobs.append(CompressionKeys.generate_compressed(ck, c_params(cp))[1].serialize())
    a, b = (SC.parse(cp, x) for x in blobs)
    assert a[0] != b[0] and not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    with pytest.raises(ValueError):
        CompressionKeys.generate_compressed(ClientKey.deserialize(get(cp).before), c_params(cp), seed=bytes(31))


def test_host_expansion_has_the_stream_words_and_the_bodies(case):
    cp = case.cp
    kn = cp.k * cp.N
    pksk, bsk = case.key.export()
    pksk = pksk.reshape(R.N_BIG * cp.ell, R.cols(cp))
    bsk = bsk.reshape(2 * kn, 2, R.N_BIG)
    assert np.array_equal(pksk[:, kn:], case.pb)
    assert np.array_equal(bsk[:, 1], case.bb)
    rows = case.rows(R.N_BIG * cp.ell)
    assert np.array_equal(pksk[rows, :kn], SC.masks(MASK_SEED, SC.STREAM_PKSK, rows, kn))
    rows = case.rows(2 * kn)
    assert np.array_equal(bsk[rows, 0], SC.masks(MASK_SEED, SC.STREAM_CBSK, rows, R.N_BIG))
    assert (case.key.params.glwe_dimension, case.key.params.polynomial_size, case.key.params.pks_level) == (cp.k, cp.N, cp.ell)
    assert case.key.main_params.lwe_dimension == case.n


# ------------------------------------------------------------------ the expanded key at work
@pytest.mark.parametrize("cp", SMALL + [R.DEFAULT], ids=set_id)
def test_compression_through_the_expanded_key(cp):
    case = get(cp)
    for B in (1, cp.L + 1):
        v = int.from_bytes(np.random.default_rng(B).bytes((2 * B + 7) // 8), "little") % (1 << (2 * B))
        vals = [(v >> (2 * i)) & 3 for i in range(B)]
        lst = CompressedCiphertextList.compress_host(case.key, case.ck.encrypt_blocks(vals), 3, RADIX, 2 * B)
        assert lst.decrypt(case.priv) == v
        got, _ = R.decrypt_values(cp, R.parse_list(cp, lst.serialize())[3], case.sprime)
        assert got == vals


@pytest.mark.parametrize("cp", SMALL, ids=set_id)
def test_decompression_through_the_rekeyed_oracle(cp):
    """unpack and sample-extract in numpy, then the untouched oracle's blind rotate under the EXPANDED
    decompression BSK: all 16 values come back.  A row 0 whose gadget were missing, or of the wrong sign,
    would rotate by garbage."""
    case = get(cp)
    kn = cp.k * cp.N
    ok = K.rekeyed_oracle(SEED, kn, 1, np.zeros(R.N_BIG * 5 * (kn + 1), np.uint64), case.key.export()[1])
    assert np.array_equal(ok.glwe_sk, case.S)
    B = max(16, cp.L + 1)
    vals = [(5 * i + 3) % 16 for i in range(B)]
    assert set(vals) == set(range(16))
    lst = CompressedCiphertextList.compress_host(case.key, case.ck.encrypt_blocks(vals), 15, RADIX, 2 * B)
    rows = R.extract_rows(cp, R.parse_list(cp, lst.serialize())[3])
    out = R.oracle_decompress(ok, rows)
    assert [case.ck.decrypt_block(o) for o in out] == vals


# ------------------------------------------------------------------ wire
def test_wire_length_and_round_trip(case):
    cp = case.cp
    assert len(case.blob) == 128 + 8 * (2048 * cp.ell * cp.N + 4096 * cp.k * cp.N) == SC.wire_len(cp)
    if cp is R.DEFAULT:
        assert len(case.blob) == 50_331_776
    assert struct.unpack_from("<II", case.blob, 8) == (2, SC.KIND)
    back = CompressedCompressionKey.deserialize(case.blob)
    assert back.serialize() == case.blob
    assert (back.params.glwe_dimension, back.params.polynomial_size, back.params.lwe_per_glwe) == (cp.k, cp.N, cp.L)


def test_refusals_of_the_reader():
    case = get(R.SMALL_A)
    cp, blob = case.cp, case.blob
    full = case.key.serialize()
    assert CompressionKey.deserialize(full).serialize() == full  # the expanded key serializes as kind 8
    # kinds 8 and 12 refuse each other, also with a sound frame of the own kind around the other payload
    with pytest.raises(FheError, match="kind"):
        CompressedCompressionKey.deserialize(full)
    with pytest.raises(FheError, match="kind"):
        CompressionKey.deserialize(blob)
    with pytest.raises(FheError, match="payload length"):
        CompressedCompressionKey.deserialize(K.frame(SC.KIND, full[32:]))
    with pytest.raises(FheError, match="payload length"):
        CompressionKey.deserialize(K.frame(R.KIND_KEY, blob[32:]))
    with pytest.raises(FheError, match="kind"):
        CompressedCompressionKey.deserialize(case.before)
    # a flipped checksum, a flipped byte anywhere
    for i in (0, 9, 13, 17, 24, 31, 33, 70, 96, 127, 128, len(blob) - 1):
        bad = bytearray(blob)
        bad[i] ^= 0x40
        with pytest.raises(FheError):
            CompressedCompressionKey.deserialize(bytes(bad))
    # truncation at every field boundary and in the bodies, one trailing byte
    for cut in (0, 8, 12, 16, 24, 32, 36, 64, 68, 72, 92, 96, 100, 127, 128, 129, 136, len(blob) - 8, len(blob) - 1):
        with pytest.raises(FheError):
            CompressedCompressionKey.deserialize(blob[:cut])
        if cut > 32:  # with a sound frame: the parser or the length formula refuses
            with pytest.raises(FheError):
                CompressedCompressionKey.deserialize(K.frame(SC.KIND, blob[32:cut]))
    with pytest.raises(FheError):
        CompressedCompressionKey.deserialize(blob + b"\0")
    # a payload one word short or long, checksum right
    with pytest.raises(FheError, match="payload length"):
        CompressedCompressionKey.deserialize(K.frame(SC.KIND, blob[32:-8]))
    with pytest.raises(FheError, match="payload length"):
        CompressedCompressionKey.deserialize(K.frame(SC.KIND, blob[32:] + bytes(8)))
    # compression parameters out of range, checksum right
    for off, v in ((0, 9), (0, 0), (1, 100), (1, 4096), (2, 0), (2, cp.N + 1), (3, 8), (3, 0), (4, 9), (4, 0), (5, 63), (6, 11)):
        bad = bytearray(blob)
        struct.pack_into("<I", bad, 68 + 4 * off, v)
        with pytest.raises(FheError, match="unsupported compression parameters"):
            CompressedCompressionKey.deserialize(K.refnv(bad))
    # main parameters out of range
    bad = bytearray(blob)
    struct.pack_into("<I", bad, 32 + 6 * 4, 3)  # message_modulus
    with pytest.raises(FheError):
        CompressedCompressionKey.deserialize(K.refnv(bad))
    # parameters that claim another size than the payload backs
    for off, v in ((1, 2 * cp.N), (0, 2), (4, cp.ell + 1)):
        bad = bytearray(blob)
        struct.pack_into("<I", bad, 68 + 4 * off, v)
        with pytest.raises(FheError, match="payload length"):
            CompressedCompressionKey.deserialize(K.refnv(bad))


def test_parameter_ranges_draw_nothing():
    ck = ClientKey.deserialize(get(R.SMALL_A).before)
    with pytest.raises(FheError, match="<= 2048") as e:
        CompressionKeys.generate_compressed(ck, CompressionParams(4, 1024, 256, 4, 4, 42, 12), seed=MASK_SEED)
    assert e.value.code == -5  # FHE_ERR_UNSUPPORTED
    assert ck.serialize() == get(R.SMALL_A).before


# ------------------------------------------------------------------ resources
def test_expand_pksk_planes_has_no_scratch(tmp_path):
    from test_kernel_resources import CSRC, HIPCC, descriptors
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    desc = descriptors(os.path.join(CSRC, "seeded_compression.hip"), tmp_path)
    ks = [v for k, v in desc.items() if "k_expand_pksk_planes" in k]
    assert len(ks) == 1, "k_expand_pksk_planes not found in seeded_compression.hip"
    assert ks[0]["private_segment_fixed_size"] == 0, "scratch spill"
    assert ks[0]["group_segment_fixed_size"] == 64 * 17 * 8  # the 64 x 16 word tile, row stride 17
