"""Message spaces other than 4 x 4 on the CPU (tests/msg_spaces.py says which and why).

  round trips   per space the key words and encrypt_blocks' words equal the oracle's under one seed, every value
                0 .. mc - 1 decodes, value mc is refused; the oracle's own bootstrap computes f(m) for every m (the
                reference the GPU file compares against); the OPRF accumulator equals its restatement at every bits
  the 2+2 rule  under a key that is not exactly message 4, carry 4, every host constructor of a radix value --
                CompressedFheUint.try_encrypt, CompressedBigUintFHE.new, the compact list builder's push and
                push_biguint -- and the deserializers of their blobs answer FHE_ERR_INVALID naming message_modulus,
                and the client key's encryption stream has not moved.  Before the rule, 0xDEADBEEF through a packed
                compact list decrypted to 0x12213223 (2 x 2), 0x10011001 (2 x 1), 0x56253667 (4 x 2), and a 2 x 1
                CompressedFheUint32 serialized 236 bytes of 2-bit digits wrapped through the padding bit.
  stored lists  a degree byte is checked against the key's mc, not against 16, by both compress_host entry points
                and both readers
  the helper    oprf_ref.value_by_rotation decodes in the space it is told
"""
import struct

import numpy as np
import pytest

import compress_ref
import oprf_ref as O
import oracle
import public_key_ref as P
from fhe_sign import (CompactCiphertextList, CompactPublicKey, CompressedBigUintFHE, CompressedCiphertextList,
                      CompressedFheUint, CompressedFheUint32, CompressionKeys, CompressionParams, FheError,
                      SwitchedCiphertextList, generate_keys, oprf_lut_host, oprf_rows_host)
from msg_spaces import (DEFAULT, SPACES, box_of, delta_of, mc_of, oprf_max_bits, oracle_params, product_params, space_id,
                        tables)

SEED = 0x5ACE5
ENC_SEED = 0xE2C
MASK_SEED = bytes(range(40, 72))
VALUE = 0xDEADBEEF
RADIX = 0  # FHE_SEEDED_RADIX
MSG_AT, CARRY_AT = 32 + 6 * 4, 32 + 7 * 4  # the two moduli in a blob: frame, then the nine parameter words

_keys = {}


def keys(space):
    """(client key, server key, oracle keys) of a space at n = 16, made once; tests that draw from the client key's
    stream re-seed it first"""
    if space not in _keys:
        ck, sk = generate_keys(product_params(space), seed=SEED)
        _keys[space] = (ck, sk, oracle.OracleKeys(SEED, oracle_params(space)))
    return _keys[space]


@pytest.fixture(scope="module", autouse=True)
def _drop_keys():
    yield
    _keys.clear()


def refused(call):
    """the call answers FHE_ERR_INVALID and names message_modulus"""
    with pytest.raises(FheError, match="message_modulus") as e:
        call()
    assert e.value.code == -1


# ---------------------------------------------------------------- the table itself
def test_table_is_what_the_abi_admits():
    assert DEFAULT not in SPACES and len(SPACES) == 9
    assert {mc_of(s) for s in SPACES} == {2, 4, 8, 16, 32, 64}
    for s in SPACES:
        ck, _, ok = keys(s)
        assert (ck.params.message_modulus, ck.params.carry_modulus) == s
        assert ok.delta() == delta_of(s) and box_of(s) * mc_of(s) == 2048
        assert 1 <= oprf_max_bits(s) and (1 << oprf_max_bits(s)) == s[0]
    assert box_of((2, 1)) == 1024 and box_of((8, 8)) == 32 and delta_of((2, 8)) == delta_of(DEFAULT)


# ---------------------------------------------------------------- round trips
@pytest.mark.parametrize("space", list(SPACES), ids=space_id)
def test_keys_and_blocks_equal_the_oracle(space):
    ck, sk, ok = keys(space)
    mc = mc_of(space)
    lwe, glwe = ck.export()
    ksk, bsk = sk.export()
    assert np.array_equal(lwe, ok.lwe_sk) and np.array_equal(glwe, ok.glwe_sk)
    assert np.array_equal(ksk, ok.ksk) and np.array_equal(bsk, ok.bsk)
    values = [m % mc for m in range(max(mc, 5) + 3)]  # every value, the first ones twice
    ck.seed_encryption(ENC_SEED, 100)
    cts = ck.encrypt_blocks(values)
    r = ok.rng(ENC_SEED, 100)
    want = np.stack([ok.encrypt(r, m) for m in values])
    assert np.array_equal(cts, want)
    assert [ck.decrypt_block(c) for c in cts] == values == [ok.decrypt(c) for c in cts]
    phases = ck.decrypt_phase_host(cts)
    assert [int((int(p) + delta_of(space) // 2) // delta_of(space)) % mc for p in phases] == values
    ck.seed_encryption(ENC_SEED, 100)
    assert np.array_equal(np.stack([ck.encrypt_block(m) for m in values[:3]]), want[:3])
    before = ck.serialize()
    for call in (lambda: ck.encrypt_block(mc), lambda: ck.encrypt_blocks([0, mc]), lambda: ck.encrypt_rows_indexed_host([mc])):
        with pytest.raises(FheError) as e:
            call()
        assert e.value.code == -1
    assert ck.serialize() == before


@pytest.mark.parametrize("space", list(SPACES), ids=space_id)
def test_the_oracle_bootstraps_every_value(space):
    """the reference of the GPU file: fho_make_lut + fho_pbs_batch compute table[m] for every m and every table"""
    _, _, ok = keys(space)
    mc = mc_of(space)
    r = ok.rng(9)
    cts = np.stack([ok.encrypt(r, m) for m in range(mc)])
    for t in tables(mc):
        out = ok.pbs_batch(cts, ok.make_lut(t)[None, :], np.zeros(mc, np.uint32))
        assert [ok.decrypt(o) for o in out] == t


@pytest.mark.parametrize("space", list(SPACES), ids=space_id)
def test_oprf_accumulator_at_every_bits(space):
    p = product_params(space)
    top = oprf_max_bits(space)
    for bits in range(1, top + 1):
        assert np.array_equal(oprf_lut_host(bits, p), O.lut(bits, delta_of(space))), bits
    for bits in (0, top + 1):
        with pytest.raises(FheError) as e:
            oprf_lut_host(bits, p)
        assert e.value.code == -1


# ---------------------------------------------------------------- the radix layer's one rule, on the host
def _blobs():
    """one blob of each radix wire kind a host constructor makes, under the default space"""
    ck, _ = generate_keys(product_params(DEFAULT), seed=SEED)
    pk = CompactPublicKey.new(ck, seed=MASK_SEED)
    b = CompactCiphertextList.builder(pk)
    b.push(VALUE, 32)
    b.push_biguint(VALUE << 7)
    return {
        "seeded radix": (CompressedFheUint, CompressedFheUint32.try_encrypt(VALUE, ck, seed=MASK_SEED).serialize()),
        "seeded biguint": (CompressedBigUintFHE, CompressedBigUintFHE.new(VALUE << 7, ck, seed=MASK_SEED).serialize()),
        "compact": (CompactCiphertextList, b.build(seed=MASK_SEED).serialize()),
        "compact packed": (CompactCiphertextList, b.build_packed(seed=MASK_SEED).serialize()),
    }


@pytest.fixture(scope="module")
def blobs():
    return _blobs()


def test_default_space_is_untouched(blobs):
    """the control of the refusals below: under 4 x 4 every constructor runs, every blob reads back and decrypts"""
    ck, _ = generate_keys(product_params(DEFAULT), seed=SEED)
    for name, (cls, blob) in blobs.items():
        x = cls.deserialize(blob)
        assert x.serialize() == blob, name
        if cls is CompactCiphertextList:
            assert x.decrypt(ck) == [VALUE, VALUE << 7], name


@pytest.mark.parametrize("space", list(SPACES), ids=space_id)
def test_radix_constructors_refuse(space, blobs):
    ck, _, _ = keys(space)
    ck.seed_encryption(ENC_SEED, 100)
    pk = CompactPublicKey.new(ck, seed=MASK_SEED)  # the key itself is of any space: an encryption of zero
    assert (pk.params.message_modulus, pk.params.carry_modulus) == space
    stream = ck.serialize()  # parameters, keys and the ChaCha stream's whole state
    refused(lambda: CompressedFheUint32.try_encrypt(VALUE, ck, seed=MASK_SEED))
    refused(lambda: CompressedFheUint32.try_encrypt(VALUE, ck))
    refused(lambda: CompressedBigUintFHE.new(VALUE << 7, ck, seed=MASK_SEED))
    assert ck.serialize() == stream, "a refused seeded encryption drew from the client key's stream"
    # the compact list: refused at push and push_biguint, where the 2-bit digits would be cut; an empty list builds
    b = CompactCiphertextList.builder(pk)
    refused(lambda: b.push(VALUE, 32))
    refused(lambda: b.push_biguint(VALUE << 7))
    for empty in (b.build(seed=MASK_SEED), b.build_packed(seed=MASK_SEED)):
        assert len(empty) == 0 and empty.ncoef == 0
    assert ck.serialize() == stream
    # the readers, when the blob's parameters say so
    for name, (cls, blob) in blobs.items():
        bad = bytearray(blob)
        struct.pack_into("<II", bad, MSG_AT, *space)
        bad = P.refnv(bytes(bad))
        refused(lambda: cls.deserialize(bad))


# ---------------------------------------------------------------- stored lists: the degree byte against mc
def _comp_keys(ck):
    cp = compress_ref.SMALL_A
    return CompressionKeys.generate(ck, CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12))[1]


def _patched(blob, at, byte):
    bad = bytearray(blob)
    bad[at] = byte
    return P.refnv(bytes(bad))


@pytest.mark.parametrize("space", list(SPACES) + [DEFAULT], ids=space_id)
def test_stored_lists_refuse_a_degree_of_mc(space):
    """degree mc - 1 is the largest a block of the space can have; mc (15 < mc: accepted before as any byte below
    16 was, mc = 64: 16 .. 63 were refused) is not one"""
    if space == DEFAULT:
        ck, sk = generate_keys(product_params(DEFAULT), seed=SEED)
    else:
        ck, sk, _ = keys(space)
    mc = mc_of(space)
    ck.seed_encryption(ENC_SEED, 100)
    cts = ck.encrypt_blocks([m % mc for m in range(16)])
    ckey = _comp_keys(ck)
    degrees_at = {SwitchedCiphertextList: 80, CompressedCiphertextList: 108}
    for cls, key in ((SwitchedCiphertextList, sk), (CompressedCiphertextList, ckey)):
        ok_list = cls.compress_host(key, cts, mc - 1, RADIX, 32)
        blob = ok_list.serialize()
        at = degrees_at[cls]
        assert blob[at:at + 16] == bytes([mc - 1]) * 16, cls.__name__
        assert cls.deserialize(blob).serialize() == blob
        for deg in sorted({mc, 255} | ({15, 16} if mc < 16 else set())):
            with pytest.raises(FheError, match="degree") as e:
                cls.compress_host(key, cts, deg, RADIX, 32)
            assert e.value.code == -1, (cls.__name__, deg)
            for k in (0, 15):
                with pytest.raises(FheError, match="degree") as e:
                    cls.deserialize(_patched(blob, at + k, deg))
                assert e.value.code == -1, (cls.__name__, deg, k)


# ---------------------------------------------------------------- the OPRF helper
@pytest.mark.parametrize("space", [(2, 1), (8, 2), (16, 1), (64, 1), (8, 8)], ids=space_id)
def test_value_by_rotation_decodes_in_its_space(space):
    ck, _, _ = keys(space)
    lwe_sk = ck.export()[0]
    delta, mc = delta_of(space), mc_of(space)
    rws = O.rows(MASK_SEED, 16, 24)
    assert np.array_equal(oprf_rows_host(MASK_SEED, 16, 24), rws)
    for bits in sorted({1, oprf_max_bits(space)}):
        fast = [int(v) for v in O.values(rws, lwe_sk, bits)]
        assert [O.value_by_rotation(r, lwe_sk, bits, delta, mc) for r in rws] == fast
        assert max(fast) < (1 << bits)
        if bits > 4:  # the literal % 16 this helper had: these rows draw values it would have folded
            assert max(fast) >= 16
