"""Public-key encryption on the host: tfhe-rs' CompactPublicKey::new, CompactCiphertextList::builder(..)
.build() / .build_packed(), and the host expansion that defines the GPU kernel (include/fhe_rocm.h "public-key
encryption", csrc/public_key.cpp).  Every word is checked against tests/public_key_ref.py, a numpy restatement
with its own RFC 8439.  No GPU, no context.

The phase bound is derived, not measured: a coefficient's error is E R + E2 - E1 S with R and S binary and
every noise word in [-2^17, 2^17], so |error| <= 2048 2^17 + 2^17 + 2048 2^17 < 2^30."""
import struct

import numpy as np
import pytest

import public_key_ref as ref
from fhe_sign import (ClientKey, CompactCiphertextList, CompactPublicKey, CompressedFheUint, ServerKey, default_params,
                      generate_keys)
from fhe_sign._lib import FheError

SEED = 0x5EED0D
ENC_SEED, ENC_STREAM = 0x0123456789ABCDEF, 100
ENC_KEY, ENC_NONCE = ref.enc_stream_key(ENC_SEED), (ENC_STREAM, ref.ROCM, 0)
MASK_SEED = bytes(range(9, 41))
LIST_SEED = bytes(range(201, 233))
N = ref.N
RADIX, BIGUINT = ref.RADIX, ref.BIGUINT
KIND_KEY, KIND_LIST = 10, 11


@pytest.fixture(scope="module")
def keys():
    ck, _ = generate_keys(seed=SEED)
    sk = ck.export()[1]
    ck.seed_encryption(ENC_SEED, ENC_STREAM)
    pk = CompactPublicKey.new(ck, seed=MASK_SEED)
    return ck, sk, pk


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits) if bits else 0


def build(pk, values, packed, seed=LIST_SEED):
    b = CompactCiphertextList.builder(pk)
    for form, v, count in values:
        if form == RADIX:
            b.push(v, bits=count)
        else:
            b.push_biguint(v)
    return b.build_packed(seed=seed) if packed else b.build(seed=seed)


# 33 bits of limbs -> 2 limbs; the odd radix widths leave a lone last block in the packed form
MIXED = [(RADIX, _value(6), 6), (RADIX, _value(32), 32), (BIGUINT, _value(64) | 1 << 63, 2), (RADIX, 3, 2),
         (BIGUINT, 0, 0), (RADIX, _value(10), 10)]


# ------------------------------------------------------------------ the key
def test_key_body_equals_the_definition(keys):
    _, sk, pk = keys
    seed, body = pk.export()
    assert seed == MASK_SEED
    assert np.array_equal(body, ref.key_body(MASK_SEED, sk, ENC_KEY, ENC_NONCE))


def test_key_generation_advances_the_stream_by_n_words(keys):
    _, sk, _ = keys
    ck, _ = generate_keys(seed=SEED)
    ck.seed_encryption(ENC_SEED, ENC_STREAM)
    clone = ClientKey.deserialize(ck.serialize())
    CompactPublicKey.new(ck, seed=MASK_SEED)
    after = ck.encrypt_block(5)
    # a clone advanced by exactly N words: the seeded form draws one word per block (tests/test_seeded.py)
    CompressedFheUint.try_encrypt(0, clone, bits=2 * N, seed=MASK_SEED)
    assert np.array_equal(after, clone.encrypt_block(5))
    # and by the definition: fhe_encrypt_block with the stream at u64 word N (2048 masks, then the noise word)
    w = ref.stream_u64(ENC_KEY, ENC_NONCE, N, N + 1)
    dot = int((w[:N] * sk).sum(dtype=np.uint64))
    body = (dot + ref.DELTA * 5 + int(ref.tuniform(w[N:])[0])) & ref.M64
    assert np.array_equal(after, np.append(w[:N], np.uint64(body)))
    # a serialized client key continues where the original does
    again = ClientKey.deserialize(ck.serialize())
    assert np.array_equal(again.encrypt_block(1), ck.encrypt_block(1))


def test_default_seeds_are_entropy(keys):
    ck, _, pk = keys
    a, b = CompactPublicKey.new(ck).export()[0], CompactPublicKey.new(ck).export()[0]
    assert a != b and a != bytes(32) and b != bytes(32)
    x = CompactCiphertextList.builder(pk).push(9, bits=32).build_packed().export()
    y = CompactCiphertextList.builder(pk).push(9, bits=32).build_packed().export()
    assert not np.array_equal(x[0], y[0]) and not np.array_equal(x[1], y[1])
    with pytest.raises(ValueError):
        CompactPublicKey.new(ck, seed=b"short")
    with pytest.raises(ValueError):
        CompactCiphertextList.builder(pk).push(9, bits=32).build(seed=b"short")


def test_the_encryption_seed_is_not_in_the_list(keys):
    _, _, pk = keys
    blob = build(pk, MIXED, True).serialize()
    assert LIST_SEED not in blob and LIST_SEED[:8] not in blob


# ------------------------------------------------------------------ the list, word for word
@pytest.mark.parametrize("packed", [False, True])
def test_list_words_equal_the_definition(keys, packed):
    _, sk, pk = keys
    x = build(pk, MIXED, packed)
    m, firsts = ref.coefficients(MIXED, packed)
    assert (x.packed, len(x), x.ncoef, x.nchunks) == (packed, len(MIXED), len(m), 1)
    for i, (form, _, count) in enumerate(MIXED):
        nb = len(ref.blocks_of(form, 0, count))
        assert x.value_info(i) == (form, count, nb, firsts[i], (nb + 1) // 2 if packed else nb)
    ca, cb = x.export()
    want_a, want_b = ref.encrypt(MASK_SEED, pk.export()[1], LIST_SEED, m)
    assert np.array_equal(ca, want_a)
    assert np.array_equal(cb, want_b)


# a 4096-bit value and a 2-bit value are 2049 coefficients unpacked (two chunks); two 4096-bit values and a
# 2-bit value are 4097 (three chunks)
CHUNKED = {2049: [(RADIX, _value(4096), 4096), (RADIX, 2, 2)],
           4097: [(RADIX, _value(4096), 4096), (RADIX, _value(4096, 1), 4096), (RADIX, 2, 2)]}


@pytest.fixture(scope="module", params=sorted(CHUNKED))
def chunked(keys, request):
    _, _, pk = keys
    values = CHUNKED[request.param]
    return values, build(pk, values, False), request.param


def test_later_chunks_words_equal_the_definition(keys, chunked):
    _, _, pk = keys
    values, x, ncoef = chunked
    m, _ = ref.coefficients(values, False)
    assert (x.ncoef, x.nchunks) == (ncoef, (ncoef + N - 1) // N)
    ca, cb = x.export()
    want_a, want_b = ref.encrypt(MASK_SEED, pk.export()[1], LIST_SEED, m)
    assert np.array_equal(ca, want_a) and np.array_equal(cb, want_b)
    assert not np.array_equal(ca[0], ca[1])  # the chunks' streams differ


def test_expand_host_equals_the_definition(keys, chunked):
    _, sk, _ = keys
    values, x, ncoef = chunked
    rows = x.expand_host()
    ca, cb = x.export()
    want = ref.expand(ca, cb)
    assert rows.shape == (ncoef, 2049)
    for t in (0, 1, 2046, 2047, 2048):  # all negated but one, ..., none negated, the second chunk's first
        assert np.array_equal(rows[t], want[t]), t
    assert np.array_equal(rows, want)
    assert rows[0, 0] == ca[0, 0] and int(rows[0, 1]) == -int(ca[0, 2047]) & ref.M64
    assert rows[2047, 0] == ca[0, 2047] and rows[2047, 2047] == ca[0, 0]
    assert rows[2048, 0] == ca[1, 0] and rows[2048, 2048] == cb[2048]
    # every coefficient's phase within the derived bound of delta m, and every block decrypts
    m, _ = ref.coefficients(values, False)
    err = ref.phase_errors(rows, sk, m)
    assert np.abs(err).max() < 1 << 30
    ck = keys[0]
    for t in (0, 1, 2047, 2048):
        assert ck.decrypt_block(rows[t]) == m[t]


@pytest.mark.parametrize("packed", [False, True])
def test_phase_within_the_derived_bound(keys, packed):
    _, sk, pk = keys
    x = build(pk, MIXED, packed)
    m, _ = ref.coefficients(MIXED, packed)
    err = ref.phase_errors(x.expand_host(), sk, m)
    assert len(err) == len(m) and np.abs(err).max() < 1 << 30


# ------------------------------------------------------------------ decryption
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("bits", [2, 6, 32, 256])
def test_radix_round_trip(keys, bits, packed):
    ck, _, pk = keys
    v = _value(bits) | 1 << (bits - 1)
    x = build(pk, [(RADIX, v, bits)], packed, seed=None)
    assert x.ncoef == ((bits // 2 + 1) // 2 if packed else bits // 2)
    assert x.decrypt(ck) == [v]
    assert CompactCiphertextList.deserialize(x.serialize()).decrypt(ck) == [v]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("limbs", [0, 1, 8])
def test_biguint_round_trip(keys, limbs, packed):
    ck, _, pk = keys
    v = _value(32 * limbs) | 1 << (32 * limbs - 1) if limbs else 0
    x = build(pk, [(BIGUINT, v, limbs)], packed, seed=None)
    assert x.value_info(0)[:3] == (BIGUINT, limbs, 16 * limbs)
    assert x.decrypt(ck) == [v]


@pytest.mark.parametrize("packed", [False, True])
def test_several_values_round_trip(keys, packed):
    ck, _, pk = keys
    x = CompactCiphertextList.deserialize(build(pk, MIXED, packed, seed=None).serialize())
    assert x.decrypt(ck) == [v for _, v, _ in MIXED]
    assert x.decrypt_value(ck, 2) == MIXED[2][1]
    with pytest.raises(FheError, match="index 6 out of range"):
        x.decrypt_value(ck, len(MIXED))
    with pytest.raises(FheError, match="index 6 out of range"):
        x.value_info(len(MIXED))


def test_decrypt_names_a_differing_parameter(keys):
    _, _, pk = keys
    p = default_params()
    p.lwe_dimension = 16
    other, _ = generate_keys(p, seed=SEED)
    with pytest.raises(FheError, match="lwe_dimension"):
        build(pk, [(RADIX, 1, 2)], True).decrypt(other)


def test_at_lwe_dimension_16():
    """the big key does not depend on n; the params field does"""
    p = default_params()
    p.lwe_dimension = 16
    ck, _ = generate_keys(p, seed=SEED)
    pk = CompactPublicKey.new(ck)
    assert struct.unpack_from("<I", pk.serialize(), 32)[0] == 16
    x = build(CompactPublicKey.deserialize(pk.serialize()), MIXED, True, seed=None)
    assert struct.unpack_from("<I", x.serialize(), 32)[0] == 16
    assert x.decrypt(ck) == [v for _, v, _ in MIXED]


# ------------------------------------------------------------------ format
def test_exact_sizes(keys):
    _, _, pk = keys
    blob = pk.serialize()
    assert len(blob) == ref.KEY_BYTES == 16484
    again = CompactPublicKey.deserialize(blob)
    assert again.serialize() == blob and again.export()[0] == MASK_SEED
    v = _value(256)
    packed = build(pk, [(RADIX, v, 256)], True).serialize()
    assert len(packed) == ref.list_bytes(1, 64) == 32 + 36 + 8 + 8 + 2048 * 8 + 64 * 8 == 16980
    unpacked = build(pk, [(RADIX, v, 256)], False).serialize()
    assert len(unpacked) == ref.list_bytes(1, 128) == 17492
    for p in (False, True):
        m, _ = ref.coefficients(MIXED, p)
        assert len(build(pk, MIXED, p).serialize()) == ref.list_bytes(len(MIXED), len(m))
    assert len(build(pk, [], True).serialize()) == ref.list_bytes(0, 0) == 76
    assert len(build(pk, [(BIGUINT, 0, 0)], False).serialize()) == 84


def test_empty_lists(keys):
    ck, _, pk = keys
    e = CompactCiphertextList.deserialize(build(pk, [], False).serialize())
    assert (len(e), e.ncoef, e.nchunks) == (0, 0, 0) and e.decrypt(ck) == [] and e.expand_host().shape == (0, 2049)
    z = CompactCiphertextList.deserialize(build(pk, [(BIGUINT, 0, 0)], True).serialize())
    assert (len(z), z.ncoef, z.nchunks) == (1, 0, 0) and z.decrypt(ck) == [0]


# ------------------------------------------------------------------ refusals
def test_key_reader_rejects_every_truncation_and_corruption(keys):
    _, _, pk = keys
    blob = pk.serialize()
    for n in list(range(0, 200)) + list(range(200, len(blob), 97)) + [len(blob) - 1]:
        with pytest.raises(FheError):
            CompactPublicKey.deserialize(blob[:n])
    with pytest.raises(FheError):
        CompactPublicKey.deserialize(blob + b"\0")
    for i in list(range(0, 120)) + list(range(120, len(blob), 331)):
        bad = bytearray(blob)
        bad[i] ^= 0x01
        with pytest.raises(FheError):
            CompactPublicKey.deserialize(bytes(bad))
    # a right checksum over a wrong length: the length check itself
    for payload in (blob[32:-8], blob[32:] + bytes(8), blob[32:68]):
        with pytest.raises(FheError, match="payload length"):
            CompactPublicKey.deserialize(ref.frame(KIND_KEY, payload))


def test_list_reader_rejects_every_truncation_and_corruption(keys):
    _, _, pk = keys
    blob = build(pk, [(RADIX, 2, 4), (BIGUINT, 7, 1)], True).serialize()
    for n in list(range(0, 200)) + list(range(200, len(blob), 89)) + [len(blob) - 1]:
        with pytest.raises(FheError):
            CompactCiphertextList.deserialize(blob[:n])
    with pytest.raises(FheError):
        CompactCiphertextList.deserialize(blob + b"\0")
    for i in list(range(0, 140)) + list(range(140, len(blob), 331)):
        bad = bytearray(blob)
        bad[i] ^= 0x01
        with pytest.raises(FheError):
            CompactCiphertextList.deserialize(bytes(bad))


def test_readers_reject_other_kinds(keys):
    ck, _, pk = keys
    kb, lb = pk.serialize(), build(pk, [(RADIX, 1, 32)], True).serialize()
    for kind in (1, 2, 3, 4, 5, 6, 7, 8, 9, KIND_LIST):
        with pytest.raises(FheError, match="kind"):
            CompactPublicKey.deserialize(ref.frame(kind, kb[32:]))
    for kind in (1, 2, 3, 4, 5, 6, 7, 8, 9, KIND_KEY):
        with pytest.raises(FheError, match="kind"):
            CompactCiphertextList.deserialize(ref.frame(kind, lb[32:]))
    with pytest.raises(FheError, match="kind"):
        CompactPublicKey.deserialize(lb)
    with pytest.raises(FheError, match="kind"):
        CompactCiphertextList.deserialize(kb)
    with pytest.raises(FheError, match="kind"):
        CompactPublicKey.deserialize(ck.serialize())
    with pytest.raises(FheError, match="kind"):
        ClientKey.deserialize(kb)
    with pytest.raises(FheError, match="kind"):
        ServerKey.deserialize(lb)
    with pytest.raises(FheError, match="kind"):
        CompressedFheUint.deserialize(lb)
    # the crafting itself is sound
    assert CompactPublicKey.deserialize(ref.frame(KIND_KEY, kb[32:])).serialize() == kb
    assert CompactCiphertextList.deserialize(ref.frame(KIND_LIST, lb[32:])).serialize() == lb


def test_list_reader_rejects_bad_flags_and_counts(keys):
    _, _, pk = keys
    blob = build(pk, [(RADIX, 2, 4), (RADIX, 1, 2)], True).serialize()  # 1 + 1 coefficients
    flag_off, nv_off, table_off = 32 + 36, 32 + 40, 32 + 44

    def altered(packed=1, nvalues=2, table=((RADIX, 4), (RADIX, 2)), tail=None):
        head = blob[:flag_off] + struct.pack("<II", packed, nvalues) + b"".join(struct.pack("<II", f, c) for f, c in table)
        b = bytearray(head + (blob[table_off + 16:] if tail is None else tail))
        struct.pack_into("<Q", b, 16, len(b) - 32)
        return ref.refnv(bytes(b))

    assert CompactCiphertextList.deserialize(altered()).serialize() == blob
    with pytest.raises(FheError, match="packed flag"):
        CompactCiphertextList.deserialize(altered(packed=2))
    with pytest.raises(FheError, match="value 1's num_bits"):
        CompactCiphertextList.deserialize(altered(table=((RADIX, 4), (RADIX, 3))))
    with pytest.raises(FheError, match="value 0's num_bits"):
        CompactCiphertextList.deserialize(altered(table=((RADIX, 4098), (RADIX, 2))))
    with pytest.raises(FheError, match="value 1's form"):
        CompactCiphertextList.deserialize(altered(table=((RADIX, 4), (2, 2))))
    # counts the payload does not back: refused from the header alone, nothing of that size is allocated
    with pytest.raises(FheError):  # the third entry is read out of C_A: whatever it says, the list is refused
        CompactCiphertextList.deserialize(altered(nvalues=3))
    with pytest.raises(FheError, match="value count inconsistent"):
        CompactCiphertextList.deserialize(altered(nvalues=1 << 16))
    for nvalues in ((1 << 16) + 1, 0xFFFFFFFF):
        with pytest.raises(FheError, match=r"2\^16 values"):
            CompactCiphertextList.deserialize(altered(nvalues=nvalues))
    for table in (((RADIX, 6), (RADIX, 2)), ((RADIX, 4), (BIGUINT, 1)), ((RADIX, 4), (BIGUINT, 0)),
                  ((BIGUINT, 1 << 20), (RADIX, 2))):
        with pytest.raises(FheError, match="inconsistent"):
            CompactCiphertextList.deserialize(altered(table=table))
    for limbs in ((1 << 20) + 1, 0xFFFFFFFF):
        with pytest.raises(FheError, match=r"2\^24"):
            CompactCiphertextList.deserialize(altered(table=((BIGUINT, limbs), (RADIX, 2))))
    with pytest.raises(FheError, match=r"2\^24"):  # each value legal, the sum too large
        CompactCiphertextList.deserialize(altered(packed=0, table=((BIGUINT, 1 << 20), (BIGUINT, 1))))
    # the unpacked reading of the same table needs one more body word
    with pytest.raises(FheError, match="inconsistent"):
        CompactCiphertextList.deserialize(altered(packed=0))


def test_builder_rejects_bad_widths(keys):
    _, _, pk = keys
    for bits in (0, 3, 4098):
        with pytest.raises(FheError, match="num_bits"):
            CompactCiphertextList.builder(pk).push(1, bits=bits)
