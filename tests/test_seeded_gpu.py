"""Seeded (compressed) ciphertexts on the GPU: CompressedFheUint / CompressedBigUintFHE .decompress()
(csrc/seeded.hip k_expand_seeded through Engine::expand_seeded) against the host expansion, which
tests/test_seeded.py pins word for word to its own ChaCha20.  Every comparison is exact."""
import csv
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
from fhe_sign import (COMPAT, BigUintFHE, CompressedBigUintFHE, CompressedFheUint, CompressedFheUint32, Context, FheUint,
                      FheUint32, Schnorr, compute_nonce, generate_keys, multi_bit_params, set_server_key)
from fhe_sign._lib import FheError

pytestmark = pytest.mark.gpu
SEED_A, SEED_B = bytes(range(1, 33)), bytes(range(101, 133))


@pytest.fixture(scope="module")
def env():
    ck, sk = generate_keys(seed=0x5EED6)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    yield ck
    set_server_key(None)
    ctx.close()


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits)


def _refnv(blob):
    blob = bytearray(blob)
    payload = bytes(blob[32:]) + b"\0" * (-(len(blob) - 32) % 8)
    h = 0xCBF29CE484222325
    for (x,) in struct.iter_unpack("<Q", payload):
        h = ((h ^ x) * 0x100000001B3) & (2**64 - 1)
    blob[24:32] = struct.pack("<Q", h)
    return bytes(blob)


# 1: counter base; 2: the second block's counter offset of 256; 5: an odd count; 2048: the maximum width
@pytest.mark.parametrize("blocks", [1, 2, 5, 16, 128, 2048])
def test_radix_expansion_equals_host(env, blocks):
    c = CompressedFheUint.try_encrypt(_value(2 * blocks), env, bits=2 * blocks, seed=SEED_A)
    x = c.decompress()
    assert x.bits == 2 * blocks
    assert np.array_equal(x.export(), c.expand_host())


@pytest.mark.parametrize("limbs", [0, 1, 3, 8])
def test_biguint_expansion_equals_host(env, limbs):
    v = _value(32 * limbs) | (1 << (32 * limbs - 1)) if limbs else 0
    c = CompressedBigUintFHE.new(v, env, seed=SEED_B)
    x = c.decompress()
    host = c.expand_host()
    assert len(x) == limbs and host.shape == (16 * limbs, 2049)
    for i, d in enumerate(x.digits):
        assert np.array_equal(d.export(), host[16 * i: 16 * i + 16])
    assert x.to_biguint(env) == v


def test_multi_bit_parameters(env):
    from fhe_sign import integer
    keyed = integer._ctx()
    ck, sk = generate_keys(multi_bit_params(), seed=0x5EED7)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    try:
        c = CompressedFheUint32.try_encrypt(0xC0FFEE11, ck, seed=SEED_A)
        x = c.decompress()
        assert np.array_equal(x.export(), c.expand_host())
        assert (x + 5).decrypt(ck) == 0xC0FFEE16
        del x
    finally:
        set_server_key(keyed)
        ctx.close()


def test_recycled_slots_keep_no_stale_word(env):
    a = CompressedFheUint.try_encrypt(_value(64), env, bits=64, seed=SEED_A)
    b = CompressedFheUint.try_encrypt(_value(64, 1), env, bits=64, seed=SEED_B)
    x = a.decompress()
    assert np.array_equal(x.export(), a.expand_host())
    del x  # its slots go back to the pool and are handed out again
    y = b.decompress()
    assert np.array_equal(y.export(), b.expand_host())
    assert not np.array_equal(a.expand_host()[:, :2048], b.expand_host()[:, :2048])


def test_expansion_behind_a_pending_graph(env):
    vx, vy, vz = 0x9E3779B9, 0x7F4A7C15, 0x12345679
    x, y = FheUint32.try_encrypt(vx, env), FheUint32.try_encrypt(vy, env)
    p = x * y  # recorded, not launched
    c = CompressedFheUint32.try_encrypt(vz, env, seed=SEED_B)
    z = c.decompress()
    assert (p + z).decrypt(env) == (vx * vy + vz) % 2**32
    assert z.decrypt(env) == vz
    assert np.array_equal(z.export(), c.expand_host())


def test_decompressed_operands_compute(env):
    va, vb = 0xDEADBEEF, 0x0BADF00D
    a = CompressedFheUint32.try_encrypt(va, env).decompress()  # seeds from OS entropy
    b = CompressedFheUint32.try_encrypt(vb, env).decompress()
    assert isinstance(a, FheUint32)
    assert (a + b).decrypt(env) == (va + vb) % 2**32
    assert (a * b).decrypt(env) == (va * vb) % 2**32
    assert (a // 5).decrypt(env) == va // 5


def test_sign_with_a_stored_compressed_private_key(env):
    """the product's long-lived object: the owner stores Enc(d) in the seeded form, the signer expands it"""
    rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
    row = next(r for r in rows if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    stored = CompressedBigUintFHE.new(d, env).serialize()
    assert len(stored) <= 128 + 8 * 16 * 8
    d_fhe = CompressedBigUintFHE.deserialize(stored).decompress()
    sig = Schnorr().sign_fhe_with_k0(msg, compute_nonce(d, msg, aux), d, d_fhe, env, COMPAT)
    assert sig.hex().upper() == row["signature"].upper()


def test_boundary_errors(env):
    r = CompressedFheUint32.try_encrypt(7, env, seed=SEED_A)
    b = CompressedBigUintFHE.new(7, env, seed=SEED_B)
    as_big, as_radix = CompressedBigUintFHE(r.handle), CompressedFheUint(b.handle)  # the same handles, other call
    try:
        with pytest.raises(FheError, match="radix integer, not a BigUintFHE"):
            as_big.decompress()
        with pytest.raises(FheError, match="BigUintFHE, not a radix integer"):
            as_radix.decompress()
    finally:
        as_big._h = as_radix._h = None  # owned by r and b
    # the other serialized kinds, both ways
    full, full_big = FheUint32.try_encrypt(7, env).serialize(), BigUintFHE.new(7, env).serialize()
    for blob in (full, full_big):
        with pytest.raises(FheError, match="kind"):
            CompressedFheUint.deserialize(blob)
    with pytest.raises(FheError, match="kind"):
        FheUint.deserialize(r.serialize())
    with pytest.raises(FheError, match="kind"):
        BigUintFHE.deserialize(b.serialize())
    # a parameter field that differs from the installed key's: refused at expansion, by name
    blob = bytearray(r.serialize())
    struct.pack_into("<I", blob, 32 + 5 * 4, 16)  # glwe_noise_log2 17 -> 16
    altered = CompressedFheUint.deserialize(_refnv(blob))
    with pytest.raises(FheError, match="glwe_noise_log2"):
        altered.decompress()
    # a message space other than the radix layer's 4 x 4: the reader itself refuses it, by name
    blob = bytearray(r.serialize())
    struct.pack_into("<I", blob, 32 + 6 * 4, 2)  # message_modulus 4 -> 2
    with pytest.raises(FheError, match="message_modulus"):
        CompressedFheUint.deserialize(_refnv(blob))
    assert r.decompress().decrypt(env) == 7  # the context is as usable as before


def test_context_without_server_key_is_refused(env):
    from fhe_sign import integer
    c = CompressedFheUint32.try_encrypt(7, env, seed=SEED_A)
    keyed = integer._ctx()
    bare = Context(0)
    set_server_key(bare)
    try:
        with pytest.raises(FheError) as e:
            c.decompress()
        assert e.value.code == -3  # FHE_ERR_NO_KEY
    finally:
        set_server_key(keyed)
        bare.close()
