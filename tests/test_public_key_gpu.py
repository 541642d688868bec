"""Public-key encryption on the GPU: CompactCiphertextList.expand() (csrc/public_key.hip k_compact_extract
through Engine::expand_compact) against the host expansion, which tests/test_public_key.py pins word for word
to its own numpy restatement.  Every comparison of ciphertext words is exact."""
import csv
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
from fhe_sign import (COMPAT, BigUintFHE, CompactCiphertextList, CompactPublicKey, Context, FheUint, FheUint32, Schnorr,
                      compute_nonce, generate_keys, multi_bit_params, set_server_key, to_u32_digits)
from fhe_sign._lib import FheError, load

pytestmark = pytest.mark.gpu
SEED_A, SEED_B = bytes(range(1, 33)), bytes(range(101, 133))


@pytest.fixture(scope="module")
def env():
    ck, sk = generate_keys(seed=0x5EED9)
    pk = CompactPublicKey.deserialize(CompactPublicKey.new(ck).serialize())  # as a device without the secret holds it
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    yield ck, pk, ctx
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


def _block_meta(x):
    """(degree, noise) of every block of an FheUint, from its serialized form (kind 3: per block a tag byte,
    u32 degree, u32 noise, 2049 words)"""
    blob = x.serialize()
    bits, nb = struct.unpack_from("<II", blob, 32 + 36)
    assert bits == x.bits and nb == bits // 2
    out, off = [], 32 + 36 + 8
    for _ in range(nb):
        tag, degree, noise = struct.unpack_from("<BII", blob, off)
        assert tag == 1  # a ciphertext, not a trivial block
        out.append((degree, noise))
        off += 9 + 2049 * 8
    assert off == len(blob)
    return out


# ------------------------------------------------------------------ extraction, word for word
# 1: t = 0, every mask word but the first negated; 2, 3, 5: odd and even t; 128: a 256-bit value
@pytest.mark.parametrize("coefs", [1, 2, 3, 5, 16, 128])
def test_extraction_equals_host(env, coefs):
    _, pk, _ = env
    x = CompactCiphertextList.builder(pk).push(_value(2 * coefs), bits=2 * coefs).build(seed=SEED_A)
    assert x.ncoef == coefs
    assert np.array_equal(x.extract_rows(), x.expand_host())


# 2049 coefficients: a 4096-bit and a 2-bit value; 4097: two 4096-bit values and a 2-bit value.  Both cross a chunk
# boundary and hold t = 2047 (no mask word negated)
@pytest.mark.parametrize("widths", [(4096, 2), (4096, 4096, 2)])
def test_extraction_across_chunks_equals_host(env, widths):
    _, pk, _ = env
    b = CompactCiphertextList.builder(pk)
    for i, bits in enumerate(widths):
        b.push(_value(bits, i), bits=bits)
    x = b.build(seed=SEED_B)
    assert (x.ncoef, x.nchunks) == (sum(widths) // 2, len(widths))
    got, want = x.extract_rows(), x.expand_host()
    for t in (0, 1, 2046, 2047, 2048, x.ncoef - 1):
        assert np.array_equal(got[t], want[t]), t
    assert np.array_equal(got, want)


def test_extraction_of_a_packed_list_equals_host(env):
    _, pk, _ = env
    x = CompactCiphertextList.builder(pk).push(_value(10), bits=10).push_biguint(_value(64) | 1 << 63).build_packed(seed=SEED_A)
    assert x.ncoef == 3 + 16
    assert np.array_equal(x.extract_rows(), x.expand_host())


# ------------------------------------------------------------------ slots and the pending graph
def test_unpacked_expansion_equals_host(env):
    ck, pk, _ = env
    vals = [_value(64), _value(6, 1), _value(96, 2) | 1 << 95, 0]
    x = (CompactCiphertextList.builder(pk).push(vals[0], bits=64).push(vals[1], bits=6).push_biguint(vals[2])
         .push_biguint(0).build(seed=SEED_A))
    host = x.expand_host()
    a, b, c, z = x.expand()
    assert isinstance(a, FheUint) and a.bits == 64 and b.bits == 6 and len(c) == 3 and len(z) == 0
    assert np.array_equal(a.export(), host[:32])
    assert np.array_equal(b.export(), host[32:35])
    for i, d in enumerate(c.digits):
        assert np.array_equal(d.export(), host[35 + 16 * i: 35 + 16 * i + 16])
    assert _block_meta(a) == [(3, 1)] * 32
    assert [a.decrypt(ck), b.decrypt(ck), c.to_biguint(ck), z.to_biguint(ck)] == vals


def test_recycled_slots_keep_no_stale_word(env):
    _, pk, _ = env
    a = CompactCiphertextList.builder(pk).push(_value(64), bits=64).build(seed=SEED_A)
    b = CompactCiphertextList.builder(pk).push(_value(64, 1), bits=64).build(seed=SEED_B)
    (x,) = a.expand()
    assert np.array_equal(x.export(), a.expand_host())
    del x  # its slots go back to the pool and are handed out again
    (y,) = b.expand()
    assert np.array_equal(y.export(), b.expand_host())
    assert not np.array_equal(a.expand_host()[:, :2048], b.expand_host()[:, :2048])


@pytest.mark.parametrize("packed", [False, True])
def test_expansion_behind_a_pending_graph(env, packed):
    ck, pk, _ = env
    vx, vy, vz = 0x9E3779B9, 0x7F4A7C15, 0x12345679
    x, y = FheUint32.try_encrypt(vx, ck), FheUint32.try_encrypt(vy, ck)
    p = x * y  # recorded, not launched
    b = CompactCiphertextList.builder(pk).push(vz, bits=32)
    c = b.build_packed() if packed else b.build()
    (z,) = c.expand()
    assert (p + z).decrypt(ck) == (vx * vy + vz) % 2**32
    assert z.decrypt(ck) == vz
    if not packed:
        assert np.array_equal(z.export(), c.expand_host())


# ------------------------------------------------------------------ the packed form
@pytest.mark.parametrize("blocks", [1, 2, 3, 5, 128])
def test_packed_list_decrypts_with_clean_degrees(env, blocks):
    ck, pk, _ = env
    v = _value(2 * blocks) | 3 << (2 * blocks - 2)
    x = CompactCiphertextList.deserialize(CompactCiphertextList.builder(pk).push(v, bits=2 * blocks).build_packed().serialize())
    assert x.ncoef == (blocks + 1) // 2
    (r,) = x.expand()
    assert r.bits == 2 * blocks
    assert r.decrypt(ck) == v
    meta = _block_meta(r)
    assert all(d <= 3 and n <= 1 for d, n in meta), meta
    assert (r + 1).decrypt(ck) == (v + 1) % (1 << (2 * blocks))


def test_packed_blocks_equal_the_bootstrap_of_the_host_rows(env):
    """3 blocks: coefficient 0 holds blocks 0 and 1, coefficient 1 the lone block 2.  Blocks 0 and 1 are the
    bootstraps of host row 0 through x & 3 and x >> 2; block 2 is host row 1 itself (the identity rule)."""
    ck, pk, ctx = env
    v = 0b11_01_10
    x = CompactCiphertextList.builder(pk).push(v, bits=6).build_packed(seed=SEED_B)
    host = x.expand_host()
    assert host.shape == (2, 2049)
    (r,) = x.expand()
    got = r.export()
    lo, hi = ctx.lut([m & 3 for m in range(16)]), ctx.lut([m >> 2 for m in range(16)])
    want = ctx.pbs(np.stack([host[0], host[0]]), [lo, hi])
    assert np.array_equal(got[2], host[1])
    assert np.array_equal(got[:2], want)
    assert [ck.decrypt_block(b) for b in got] == [0b10, 0b01, 0b11]
    assert _block_meta(r) == [(3, 1)] * 3


# ------------------------------------------------------------------ parameters and end to end
def test_multi_bit_parameters(env):
    from fhe_sign import integer
    keyed = integer._ctx()
    ck, sk = generate_keys(multi_bit_params(), seed=0x5EEDA)
    pk = CompactPublicKey.new(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    try:
        u = CompactCiphertextList.builder(pk).push(0xC0FFEE11, bits=32).build(seed=SEED_A)
        (x,) = u.expand()
        assert np.array_equal(x.export(), u.expand_host())
        assert (x + 5).decrypt(ck) == 0xC0FFEE16
        (y,) = CompactCiphertextList.builder(pk).push(0xC0FFEE11, bits=32).build_packed().expand()
        assert (y + 5).decrypt(ck) == 0xC0FFEE16
        del x, y
    finally:
        set_server_key(keyed)
        ctx.close()


@pytest.mark.parametrize("packed", [False, True])
def test_expanded_operands_compute(env, packed):
    ck, pk, _ = env
    va, vb = 0xDEADBEEF, 0x0BADF00D
    bld = CompactCiphertextList.builder(pk).push(va, bits=32).push(vb, bits=32)
    a, b = (bld.build_packed() if packed else bld.build()).expand()  # seeds from OS entropy
    assert isinstance(a, FheUint32)
    assert (a + b).decrypt(ck) == (va + vb) % 2**32
    assert (a * b).decrypt(ck) == (va * vb) % 2**32
    assert (a // 5).decrypt(ck) == va // 5


def test_sign_with_a_private_key_that_arrived_as_a_packed_list(env):
    """the wallet owner's device encrypts d under the published key; the signer expands the serialized list"""
    ck, pk, _ = env
    rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
    row = next(r for r in rows if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    limbs = len(to_u32_digits(d))  # no leading zero limb: 8 coefficients per limb
    wire = CompactCiphertextList.builder(pk).push_biguint(d).build_packed().serialize()
    assert len(wire) == 76 + 8 + 8 * (2048 + 8 * limbs)
    (d_fhe,) = CompactCiphertextList.deserialize(wire).expand()
    assert isinstance(d_fhe, BigUintFHE) and len(d_fhe) == limbs
    sig = Schnorr().sign_fhe_with_k0(msg, compute_nonce(d, msg, aux), d, d_fhe, ck, COMPAT)
    assert sig.hex().upper() == row["signature"].upper()


# ------------------------------------------------------------------ refusals
def test_boundary_errors(env):
    ck, pk, ctx = env
    x = CompactCiphertextList.builder(pk).push(7, bits=32).push_biguint(7).build_packed(seed=SEED_A)
    lib, h = load(), C.c_void_p()
    # wrong form, both ways, and an index out of range: the message names the value
    assert lib.fhe_compact_list_expand_biguint(ctx.handle, x.handle, 0, C.byref(h)) == -1
    assert b"value 0 holds a radix integer, not a BigUintFHE" in lib.fhe_last_error()
    assert lib.fhe_compact_list_expand_radix(ctx.handle, x.handle, 1, C.byref(h)) == -1
    assert b"value 1 holds a BigUintFHE, not a radix integer" in lib.fhe_last_error()
    for fn in (lib.fhe_compact_list_expand_radix, lib.fhe_compact_list_expand_biguint):
        assert fn(ctx.handle, x.handle, 2, C.byref(h)) == -1
        assert b"value index 2 out of range" in lib.fhe_last_error()
    with pytest.raises(FheError, match="index 2 out of range"):
        x.expand_value(2)
    assert not h.value
    # the other serialized kinds, both ways
    for blob in (FheUint32.try_encrypt(7, ck).serialize(), BigUintFHE.new(7, ck).serialize()):
        with pytest.raises(FheError, match="kind"):
            CompactCiphertextList.deserialize(blob)
    with pytest.raises(FheError, match="kind"):
        FheUint.deserialize(x.serialize())
    # a parameter field that differs from the installed key's: refused at expansion, by name
    blob = bytearray(x.serialize())
    struct.pack_into("<I", blob, 32 + 5 * 4, 16)  # glwe_noise_log2 17 -> 16
    altered = CompactCiphertextList.deserialize(_refnv(blob))
    with pytest.raises(FheError, match="glwe_noise_log2"):
        altered.expand()
    with pytest.raises(FheError, match="glwe_noise_log2"):
        altered.extract_rows()
    # a message space other than the radix layer's 4 x 4: the reader itself refuses it, by name
    blob = bytearray(x.serialize())
    struct.pack_into("<I", blob, 32 + 6 * 4, 2)  # message_modulus 4 -> 2
    with pytest.raises(FheError, match="message_modulus"):
        CompactCiphertextList.deserialize(_refnv(blob))
    a, b = x.expand()  # the context is as usable as before
    assert a.decrypt(ck) == 7 and b.to_biguint(ck) == 7


def test_context_without_server_key_is_refused(env):
    from fhe_sign import integer
    _, pk, _ = env
    c = CompactCiphertextList.builder(pk).push(7, bits=32).build_packed(seed=SEED_A)
    keyed = integer._ctx()
    bare = Context(0)
    set_server_key(bare)
    try:
        for call in (c.expand, c.extract_rows):
            with pytest.raises(FheError) as e:
                call()
            assert e.value.code == -3  # FHE_ERR_NO_KEY
    finally:
        set_server_key(keyed)
        bare.close()
