"""Compressed computed ciphertexts on the host: tfhe-rs' CompressedCiphertextList (include/fhe_rocm.h
"compressed computed ciphertexts"; csrc/compress_host.cpp).  No GPU, no context.

Checked word for word, in wrapping uint64, against tests/compress_ref.py's numpy restatement at
(k', N', L, beta, ell) in {(1, 8, 8, 4, 4), (2, 16, 16, 3, 5), (4, 256, 256, 4, 4)}: fhe_compress_host at
B in {1, 2, L - 1, L, L + 1, 2 L + 3} (the restatement contracts in exact float64 limbs, so the defaults run
the full set of B too), the generated packing-KSK bodies and the decompression BSK's phase (at the
defaults: every 61st packing row and every 127th BSK row, first and last included -- the numpy stream
and the 2048-coefficient products of all 8192 + 2048 rows would take minutes; the two small sets check
every row).  Then the stream accounting, the direct decryption of all 16 values in every slot, the length
formula, every refusal, and decompression through the untouched oracle re-keyed at n = k' N'."""
import struct

import numpy as np
import pytest

import compress_ref as R
import seeded_key_ref as K
from fhe_sign import (ClientKey, CompressedCiphertextList, CompressedFheUint32, CompressionKey, CompressionKeys,
                      CompressionParams, CompressionPrivateKey, default_compression_params, generate_keys)
from fhe_sign._lib import FheError
from lwe_dims import product_params

SEED = 0x5EEDC0DE
ENC_SEED, ENC_STREAM = 0x0FEDCBA987654321, 100
SETS = [R.SMALL_A, R.SMALL_B, R.DEFAULT]
RADIX, BIGUINT = 0, 1
DELTA = 1 << 59


def c_params(cp):
    return CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12)


def set_id(cp):
    return f"k{cp.k}N{cp.N}L{cp.L}b{cp.beta}l{cp.ell}"


class Case:
    """a client key with a known encryption stream and its compression keys.  The main LWE dimension is
    k' N' at the small sets, so that the oracle re-keyed at that dimension has the same big key."""

    def __init__(self, cp):
        self.cp = cp
        self.n = cp.k * cp.N if cp is not R.DEFAULT else 16
        self.ck, _ = generate_keys(product_params(self.n), seed=SEED)
        self.ck.seed_encryption(ENC_SEED, ENC_STREAM)
        self.before = self.ck.serialize()
        self.priv, self.key = CompressionKeys.generate(self.ck, c_params(cp))
        self.after = self.ck.serialize()
        self.pksk, self.bsk = self.key.export()
        self.sprime = self.priv.export()
        _, self.S = self.ck.export()
        self.main_bytes = struct.pack("<9I", self.n, 23, 3, 5, 45, 17, 4, 4, 1)
        self.rng = np.random.default_rng(0xC0FFEE + cp.N)

    def random_cts(self, B):
        cts = self.rng.integers(0, 1 << 64, (B, R.BIG_CT), dtype=np.uint64)
        if B >= 4:  # the digit edges ride along
            cts[:4] = R.edge_rows(self.cp.beta, self.cp.ell)
        return cts


_cases = {}


@pytest.fixture(scope="module", params=SETS, ids=set_id)
def case(request):
    cp = request.param
    if cp not in _cases:
        _cases[cp] = Case(cp)
    return _cases[cp]


def rows_to_check(cp, total, stride):
    return list(range(total)) if cp is not R.DEFAULT else sorted(set(range(0, total, stride)) | {total - 1})


# ------------------------------------------------------------------ keys
def test_secret_and_packing_key_bodies(case):
    cp = case.cp
    assert np.array_equal(case.sprime, R.secret_bits(cp, ENC_SEED, ENC_STREAM))
    rows = rows_to_check(cp, R.N_BIG * cp.ell, 61)
    got = case.pksk.reshape(R.N_BIG * cp.ell, cp.k + 1, cp.N)[rows]
    assert np.array_equal(got, R.pksk_rows(cp, ENC_SEED, ENC_STREAM, case.sprime, case.S, rows))


def test_decompression_key_phase(case):
    """row (q, rho): the mask is the stream's words (+ g s'_q at A[0] in row 0), and the phase B - A * S is
    e + g s'_q X^0 (row 1) or e - g s'_q S (row 0) with g = 2^41: fhe_generate_keys' gadget form"""
    cp = case.cp
    kn = cp.k * cp.N
    rows = rows_to_check(cp, 2 * kn, 127)
    bsk = case.bsk.reshape(2 * kn, 2, R.N_BIG)
    A, e = R.bsk_noise(cp, ENC_SEED, ENC_STREAM, rows)
    g = np.uint64(1 << (64 - R.PBS_BASE_LOG))
    for i, r in enumerate(rows):
        q, rho = divmod(r, 2)
        m = np.uint64(case.sprime[q])
        want_a = A[i].copy()
        want = e[i].copy()
        if rho == 0:
            want_a[:1] += g * m
            want -= g * m * case.S
        else:
            want[:1] += g * m
        assert np.array_equal(bsk[r, 0], want_a)
        assert np.array_equal(bsk[r, 1] - R.negacyclic_binary(bsk[r, 0], case.S, R.N_BIG), want), (q, rho)


def test_sizes_at_the_defaults():
    cp = R.DEFAULT
    assert R.N_BIG * cp.ell * R.cols(cp) * 8 == 83_886_080
    assert cp.k * cp.N * 4 * R.N_BIG * 8 == 67_108_864
    assert R.stream_words(cp) == 1024 + 10_485_760 + 8_388_608
    d = default_compression_params()
    assert (d.glwe_dimension, d.polynomial_size, d.lwe_per_glwe, d.pks_base_log, d.pks_level, d.pks_noise_log2,
            d.storage_log_modulus) == (4, 256, 256, 4, 4, 42, 12)


# ------------------------------------------------------------------ stream accounting
def _block_at(first, sk, value=5):
    """fhe_encrypt_block with the encryption stream at u64 word `first`: 2048 masks, then the noise word"""
    w = R.enc_stream(ENC_SEED, ENC_STREAM, first, 2049)
    body = (w[:2048] * sk).sum(dtype=np.uint64, keepdims=True) + np.uint64(DELTA * value) \
        + K.tuniform(w[2048], R.GLWE_NOISE_LOG2)
    return np.append(w[:2048], body)


def test_encryption_stream_advances_by_the_documented_words(case):
    cp, S = case.cp, case.S
    words = R.stream_words(cp)
    saved = ClientKey.deserialize(case.after)  # right after the generation
    assert np.array_equal(saved.encrypt_block(5), _block_at(words, S))
    # a key serialized before: the same keys, then the same position
    early = ClientKey.deserialize(case.before)
    priv, key = CompressionKeys.generate(early, c_params(cp))
    assert priv.serialize() == case.priv.serialize()
    if cp is not R.DEFAULT:
        assert key.serialize() == case.key.serialize()
    else:
        assert all(np.array_equal(a, b) for a, b in zip(key.export(), (case.pksk, case.bsk)))
    assert np.array_equal(early.encrypt_block(5), _block_at(words, S))


# ------------------------------------------------------------------ the packing keyswitch
def test_digits_closed_form_is_the_carry_loop(case):
    cp = case.cp
    rows = R.edge_rows(cp.beta, cp.ell)
    d = R.digits(rows[:, :R.N_BIG], cp.beta, cp.ell)
    assert d.min() >= -(1 << (cp.beta - 1)) and d.max() <= (1 << (cp.beta - 1)) - 1
    for r in range(4):
        for j in range(0, 64):
            assert list(d[r, j]) == R.digits_by_carry(rows[r, j], cp.beta, cp.ell)
    assert (d[1] == -(1 << (cp.beta - 1))).all()  # every digit half -> -half, the top carry falls off
    assert (d[2] == 0).all() and (d[3] == 0).all()


def test_float_limb_contraction_is_exact():
    cp = R.SMALL_B
    rng = np.random.default_rng(5)
    d = rng.integers(-4, 4, (5, R.N_BIG * cp.ell))
    key = rng.integers(0, 1 << 64, (R.N_BIG * cp.ell, R.cols(cp)), dtype=np.uint64)
    key[:3] = np.uint64(R.M64)
    assert np.array_equal(R.contract(d, key), R.contract_u64(d, key))


def block_counts(cp):
    return [1, 2, cp.L - 1, cp.L, cp.L + 1, 2 * cp.L + 3]


@pytest.mark.parametrize("which", range(6), ids=["1", "2", "L-1", "L", "L+1", "2L+3"])
def test_compress_host_word_for_word(case, which):
    cp = case.cp
    B = block_counts(cp)[which]
    cts = case.random_cts(B)
    degrees = [(3 * i + 1) % 16 for i in range(B)]
    lst = CompressedCiphertextList.compress_host(case.key, cts, degrees, RADIX, 2 * B)
    blob = lst.serialize()
    want = R.pack_keyswitch(cp, case.pksk, cts)
    form, count, deg, glwes = R.parse_list(cp, blob)
    assert (form, count, deg) == (RADIX, 2 * B, degrees)
    assert len(glwes) == len(want) and all(np.array_equal(a, b) for a, b in zip(glwes, want))
    assert blob == R.wire(cp, case.main_bytes, RADIX, 2 * B, degrees, want)  # padding bits and all
    assert len(blob) == R.wire_len(cp, B) == c_params(cp).wire_bytes(B)
    assert CompressedCiphertextList.deserialize(blob).serialize() == blob


def test_edge_rows_alone(case):
    """the rounding bit below / at / above, the all-levels carry, all ones, and a zero mask: (0, b) goes
    through as itself, its body modulus-switched into slot 3"""
    cp = case.cp
    cts = R.edge_rows(cp.beta, cp.ell)
    lst = CompressedCiphertextList.compress_host(case.key, cts, 3, RADIX, 8)
    _, _, _, glwes = R.parse_list(cp, lst.serialize())
    want = R.pack_keyswitch(cp, case.pksk, cts)
    assert all(np.array_equal(a, b) for a, b in zip(glwes, want))
    alone = CompressedCiphertextList.compress_host(case.key, cts[3:4].repeat(2, 0), 3, RADIX, 4)
    vals = R.parse_list(cp, alone.serialize())[3][0]
    kn = cp.k * cp.N
    b12 = int(R.modswitch12(cts[3, R.N_BIG]))
    assert not vals[:kn].any() and list(vals[kn:]) == [b12, b12]


def test_stored_bytes_cannot_see_the_low_planes():
    """Why tests/test_pack_keyswitch_gpu.py pins the contraction's 64-bit words and not only the compressed
    bytes: at the defaults, 257 blocks (a full GLWE and a one-block one), the stored 12-bit values do not move when
    bits 0-15 of EVERY packing-key word are cleared -- two of the eight byte planes the GPU contracts, and every
    carry out of them, are invisible to any comparison of compressed lists.  Clearing is a one-sided error: the
    digits' mean is -1/2, so it shifts a block's words by about 8192 * 1/2 * 2^15 = 2^27 and a coefficient of a
    full GLWE by up to 2^35, against a rounding step of 2^52 -- a flip has probability up to 2^-17 per
    coefficient, about 2 % over this list (the seed below is one at which none occurs; six other seeds: 0 of
    13,830 values moved at 16 bits, 6 at 24 bits, 1,929 at 32 bits).  Clearing bits 0-47 is the positive control:
    that does move stored values.  Numpy only: any key words show it, so they are uniform random ones."""
    cp, B = R.DEFAULT, 257
    rng = np.random.default_rng(0x10B17E5)
    key = rng.integers(0, 1 << 64, R.N_BIG * cp.ell * R.cols(cp), dtype=np.uint64)
    cts = rng.integers(0, 1 << 64, (B, R.BIG_CT), dtype=np.uint64)
    cts[:4] = R.edge_rows(cp.beta, cp.ell)
    full = R.pack_keyswitch(cp, key, cts)
    low16 = R.pack_keyswitch(cp, key & np.uint64(~0xFFFF & R.M64), cts)
    low48 = R.pack_keyswitch(cp, key & np.uint64(~0xFFFFFFFFFFFF & R.M64), cts)
    assert [len(g) for g in full] == [cp.k * cp.N + 256, cp.k * cp.N + 1]
    assert all(np.array_equal(a, b) for a, b in zip(full, low16))
    moved = sum(int((a != b).sum()) for a, b in zip(full, low48))
    assert moved > 100  # planes 0-5 reach the rounding bit: a large share of the 2305 values moves


PLANE_EDGE_WORDS = (0, 0x80, 0x7F, 0xFF, 0x8000, 0x7FFF, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, 0x7FFFFFFFFFFFFFFF,
                    0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x00FF00FF00FF00FF, 0xFF80FF80FF80FF80, 0x0123456789ABCDEF)


@pytest.mark.parametrize("cp", [R.SMALL_A, R.CP(2, 8, 5, 7, 4, 42), R.SMALL_B, R.DEFAULT], ids=set_id)
def test_plane_layout_round_trip_and_index_formula(cp):
    """compress_ref.plane_layout (the GPU's byte planes, restated): sum_b plane_b 256^b gives the key words back
    mod 2^64, padding columns excluded and all zero; every byte is in [-128, 128) by construction of int8; and
    sampled bytes equal the layout comment's own index formula evaluated one word at a time.  Random words with
    the carry edges (0x80 bytes, runs of 0xFF, the top bit) among them.  (2, 8, 5, 7, 4): 24 columns, a padded
    tile"""
    import ks_ref

    c, KT, tiles = R.cols(cp), 32 * cp.ell, (R.cols(cp) + 15) // 16
    rng = np.random.default_rng(0xB17E + cp.N)
    key = rng.integers(0, 1 << 64, R.N_BIG * cp.ell * c, dtype=np.uint64)
    key[:len(PLANE_EDGE_WORDS)] = np.array(PLANE_EDGE_WORDS, np.uint64)
    key[-len(PLANE_EDGE_WORDS):] = np.array(PLANE_EDGE_WORDS, np.uint64)
    planes = R.plane_layout(cp, key)
    assert planes.shape == (8, tiles, KT, 64, 16) and planes.dtype == np.int8
    words, padding = R.words_of_planes(cp, planes)
    assert np.array_equal(words, key)
    assert padding.size == 8 * cp.ell * R.N_BIG * (16 * tiles - c) and not padding.any()
    # the index formula, a word at a time: every corner of the index space and random places
    k3 = key.reshape(R.N_BIG, cp.ell, c)
    idx = [(tt, kt, lane, jj) for tt in (0, tiles - 1) for kt in (0, 31, 32, KT - 1) for lane in (0, 15, 16, 63) for jj in (0, 15)]
    idx += [tuple(int(x) for x in r) for r in np.stack([rng.integers(0, m, 200) for m in (tiles, KT, 64, 16)], axis=1)]
    for tt, kt, lane, jj in idx:
        k = 64 * kt + 16 * (lane >> 4) + jj
        level, j, col = k // R.N_BIG, k % R.N_BIG, 16 * tt + (lane & 15)
        want = ks_ref.byte_planes(k3[j, level, col:col + 1])[:, 0] if col < c else np.zeros(8, np.int64)
        assert list(planes[:, tt, kt, lane, jj]) == list(want), (tt, kt, lane, jj)


# ------------------------------------------------------------------ direct decryption
def test_direct_decryption_of_all_16_values_in_every_slot(case):
    """16 lists of L + 1 blocks (a full GLWE and a second one): slot t of list r holds (t + r) % 16.  At the
    defaults one list of 16 GLWEs instead (the same 16 L block compressions, one call)"""
    cp = case.cp
    rot = range(16) if cp is not R.DEFAULT else ()
    B = cp.L + 1
    for r in rot:
        vals = [(t + r) % 16 for t in range(B)]
        cts = case.ck.encrypt_blocks(vals)
        lst = CompressedCiphertextList.compress_host(case.key, cts, 15, RADIX, 2 * B)
        lst = CompressedCiphertextList.deserialize(lst.serialize())
        assert lst.decrypt(case.priv) == R.assemble(vals, 2 * B)
        got, _ = R.decrypt_values(cp, R.parse_list(cp, lst.serialize())[3], case.sprime)
        assert got == vals
    if cp is R.DEFAULT:
        # 4096 blocks, BigUintFHE form: slot t of GLWE g holds (t + g) % 16
        vals = [(i % cp.L + i // cp.L) % 16 for i in range(16 * cp.L)]
        lst = CompressedCiphertextList.compress_host(case.key, case.ck.encrypt_blocks(vals), 15, BIGUINT, cp.L)
        got, _ = R.decrypt_values(cp, R.parse_list(cp, lst.serialize())[3], case.sprime)
        assert got == vals
        limbs = [sum(v << (2 * k) for k, v in enumerate(vals[16 * i:16 * i + 16])) % (1 << 32) for i in range(cp.L)]
        assert lst.decrypt(case.priv) == sum(x << (32 * i) for i, x in enumerate(limbs))


def test_biguint_form_decrypts_limb_by_limb():
    case = _cases.get(R.SMALL_B) or Case(R.SMALL_B)
    vals = [15 - (i % 16) for i in range(32)]  # carries above degree 3 stay inside their limb
    lst = CompressedCiphertextList.compress_host(case.key, case.ck.encrypt_blocks(vals), 15, BIGUINT, 2)
    limbs = [sum(v << (2 * k) for k, v in enumerate(vals[16 * i:16 * i + 16])) % (1 << 32) for i in range(2)]
    assert lst.decrypt(case.priv) == limbs[0] | limbs[1] << 32


# ------------------------------------------------------------------ lengths
def test_length_formula():
    cp = R.DEFAULT
    assert R.wire_len(cp, 128) == 108 + 128 + 1728
    assert sum(R.glwe_bytes(cp, nb) for nb in R.bodies_of(cp, 128)) == 12 * (1024 + 128) // 8 == 1728
    case = _cases.get(cp) or Case(cp)
    lst = CompressedCiphertextList.compress_host(case.key, case.random_cts(128), 3, RADIX, 256)
    assert len(lst.serialize()) == 108 + 128 + 1728
    # byte-boundary padding: 12 (k' N' + b_g) is no multiple of 8 for odd b_g
    a = R.SMALL_A
    assert [R.wire_len(a, B) - 108 - B for B in (1, 2, 7, 8, 9, 19)] == [14, 15, 23, 24, 24 + 14, 48 + 17]


# ------------------------------------------------------------------ refusals
BAD_PARAMS = [((4, 100, 64, 4, 4, 42, 12), "power of two"), ((4, 4, 4, 4, 4, 42, 12), "power of two"),
              ((4, 4096, 64, 4, 4, 42, 12), "power of two"), ((0, 256, 256, 4, 4, 42, 12), "glwe_dimension"),
              ((9, 128, 128, 4, 4, 42, 12), "glwe_dimension"), ((4, 1024, 256, 4, 4, 42, 12), "<= 2048"),
              ((4, 256, 0, 4, 4, 42, 12), "lwe_per_glwe"), ((4, 256, 257, 4, 4, 42, 12), "lwe_per_glwe"),
              ((4, 256, 256, 8, 4, 42, 12), "pks_base_log"), ((4, 256, 256, 0, 4, 42, 12), "pks_base_log"),
              ((4, 256, 256, 4, 9, 42, 12), "<= 32"), ((4, 256, 256, 4, 0, 42, 12), "pks_level"),
              ((4, 256, 256, 4, 4, 42, 11), "storage_log_modulus"), ((4, 256, 256, 4, 4, 42, 13), "storage_log_modulus")]


@pytest.mark.parametrize("fields,why", BAD_PARAMS, ids=[str(b[0]) for b in BAD_PARAMS])
def test_parameter_ranges(fields, why):
    ck, _ = generate_keys(product_params(1), seed=SEED)
    before = ck.serialize()
    with pytest.raises(FheError, match=why) as e:
        CompressionKeys.generate(ck, CompressionParams(*fields))
    assert e.value.code == -5  # FHE_ERR_UNSUPPORTED
    assert ck.serialize() == before  # nothing drawn


def test_refusals_of_the_readers():
    case = _cases.get(R.SMALL_A) or Case(R.SMALL_A)
    cp = case.cp
    B = 9
    lst = CompressedCiphertextList.compress_host(case.key, case.random_cts(B), 3, RADIX, 2 * B)
    blobs = {"list": (lst.serialize(), CompressedCiphertextList, R.KIND_LIST),
             "private": (case.priv.serialize(), CompressionPrivateKey, R.KIND_PRIVATE),
             "key": (case.key.serialize(), CompressionKey, R.KIND_KEY)}
    assert len(blobs["private"][0]) == 96 + 8 * cp.k * cp.N
    assert len(blobs["key"][0]) == 96 + 8 * (R.N_BIG * cp.ell * R.cols(cp) + 8192 * cp.k * cp.N)
    others = [case.ck.serialize(), CompressedFheUint32.try_encrypt(7, case.ck, seed=bytes(32)).serialize()]
    for name, (blob, cls, kind) in blobs.items():
        assert cls.deserialize(blob).serialize() == blob
        # every kind refuses every other kind, also with a sound frame around the other payload
        for other, (oblob, _, okind) in blobs.items():
            if other != name:
                with pytest.raises(FheError, match="kind"):
                    cls.deserialize(oblob)
                with pytest.raises(FheError):
                    cls.deserialize(K.frame(kind, oblob[32:]))
        for oblob in others:
            with pytest.raises(FheError, match="kind"):
                cls.deserialize(oblob)
        with pytest.raises(FheError, match="kind"):
            ClientKey.deserialize(blob)
        # truncation at every field boundary and in the body, and one trailing byte
        cuts = [0, 8, 12, 16, 24, 32, 36, 64, 68, 72, 92, 96, 100, 104, 108, 109, len(blob) - 8, len(blob) - 1]
        for cut in (c for c in cuts if c < len(blob)):
            with pytest.raises(FheError):
                cls.deserialize(blob[:cut])
            if 32 < cut:  # with a sound frame: the length formula or the parser refuses
                with pytest.raises(FheError):
                    cls.deserialize(K.frame(kind, blob[32:cut]))
        with pytest.raises(FheError):
            cls.deserialize(blob + b"\0")
        with pytest.raises(FheError, match="payload length"):
            cls.deserialize(K.frame(kind, blob[32:] + bytes(8)))
        # one flipped byte anywhere in the header or the parameters
        for i in (0, 9, 13, 17, 25, 33, 70, 90, len(blob) - 1):
            bad = bytearray(blob)
            bad[i] ^= 0x40
            with pytest.raises(FheError):
                cls.deserialize(bytes(bad))
        # compression parameters out of range, checksum right
        for off, v in ((0, 9), (1, 100), (2, 0), (3, 8), (4, 9), (6, 11)):
            bad = bytearray(blob)
            struct.pack_into("<I", bad, 68 + 4 * off, v)
            with pytest.raises(FheError, match="unsupported compression parameters"):
                cls.deserialize(K.refnv(bad))
        # parameters that claim another size than the payload backs
        bad = bytearray(blob)
        struct.pack_into("<I", bad, 68 + 4, 2 * cp.N)
        with pytest.raises(FheError, match="payload length"):
            cls.deserialize(K.refnv(bad))
    blob = blobs["list"][0]

    def crafted(form=RADIX, count=2 * B, nb=B, degrees=None, tail=None):
        degrees = bytes([3] * nb) if degrees is None else degrees
        tail = blob[R.HEADER + B:] if tail is None else tail
        return K.frame(R.KIND_LIST, blob[32:R.HEADER - 12] + struct.pack("<3I", form, count, nb) + degrees + tail)

    assert CompressedCiphertextList.deserialize(crafted()).serialize() == blob  # the crafting is sound
    with pytest.raises(FheError, match="degree"):
        CompressedCiphertextList.deserialize(crafted(degrees=bytes([3] * (B - 1) + [16])))
    with pytest.raises(FheError, match="form / count"):
        CompressedCiphertextList.deserialize(crafted(count=2 * B + 2))
    with pytest.raises(FheError, match="form / count"):
        CompressedCiphertextList.deserialize(crafted(form=BIGUINT, count=1))
    with pytest.raises(FheError, match="unknown form"):
        CompressedCiphertextList.deserialize(crafted(form=2))
    with pytest.raises(FheError, match="payload length"):
        CompressedCiphertextList.deserialize(crafted(nb=B + 1, count=2 * B + 2, degrees=bytes([3] * (B + 1))))
    with pytest.raises(FheError, match="2\\^24"):
        CompressedCiphertextList.deserialize(crafted(form=BIGUINT, count=(1 << 20) + 1, nb=(1 << 24) + 16))
    with pytest.raises(FheError, match="num_bits"):
        CompressedCiphertextList.deserialize(crafted(count=2 * B + 1))
    # fhe_compress_host's own checks
    cts = case.random_cts(2)
    for args, why in (((cts, 16, RADIX, 4), "degree"), ((cts, 3, RADIX, 6), "nblocks"), ((cts, 3, BIGUINT, 1), "nblocks"),
                      ((cts, 3, 7, 4), "unknown form")):
        with pytest.raises(FheError, match=why):
            CompressedCiphertextList.compress_host(case.key, *args)
    # a private key of another parameter set does not decrypt the list
    other = _cases.get(R.SMALL_B) or Case(R.SMALL_B)
    with pytest.raises(FheError, match="compression parameters"):
        lst.decrypt(other.priv)


# ------------------------------------------------------------------ decompression, through the oracle
@pytest.mark.parametrize("cp", [R.SMALL_A, R.SMALL_B], ids=set_id)
def test_decompression_through_the_rekeyed_oracle(cp):
    """unpack and sample-extract in numpy, then fho_blind_rotate + fho_sample_extract of the untouched
    oracle re-keyed at n = k' N' with the decompression BSK and the identity table; the result decrypts
    under the main key to the block values"""
    case = _cases.get(cp) or Case(cp)
    kn = cp.k * cp.N
    ok = K.rekeyed_oracle(SEED, kn, 1, np.zeros(R.N_BIG * 5 * (kn + 1), np.uint64), case.bsk)
    assert np.array_equal(ok.glwe_sk, case.S)
    B = cp.L + 1 if cp.L + 1 >= 16 else 2 * cp.L
    vals = [(5 * i + 3) % 16 for i in range(B)]
    lst = CompressedCiphertextList.compress_host(case.key, case.ck.encrypt_blocks(vals), 15, RADIX, 2 * B)
    rows = R.extract_rows(cp, R.parse_list(cp, lst.serialize())[3])
    assert rows.shape == (B, kn + 1)
    out = R.oracle_decompress(ok, rows)
    assert [case.ck.decrypt_block(o) for o in out] == vals
    assert [ok.decrypt(o) for o in out] == vals
