"""The seeded (compressed) compression key on the GPU (csrc/seeded_compression.hip, fhe_set_compression_key_seeded)
against the host definition fhe_seeded_compression_key_expand_host, which tests/test_seeded_compression_key.py
pins word for word to tests/seeded_compression_ref.py.

Two contexts per parameter set: `seeded` installed from the bodies, `full` from decompress().  Their device
state -- byte planes, Fourier BSK, its E layout -- is compared word for word; compression byte for byte with
fhe_compress_host under the expanded key; decompression word for word between the two, and with the re-keyed
oracle at the small sets.  What each set reaches in k_expand_pksk_planes:
  (1, 8, 8, 4, 4)      cols 16: one tile, columns 0-7 generated, 8-15 bodies
  (2, 8, 5, 7, 4)      cols 24: tile 0 all generated (two polynomials, one ChaCha block each), tile 1 = 8 bodies +
                       8 zero padding columns; L < N'; 7-bit digits
  (2, 16, 16, 3, 5)    ell = 5: KT = 160, the row index j 5 + l is no power-of-two stride
  (1, 2048, 4, 4, 1)   a mask row fills its 256-block stride exactly, 128 mask tiles; words and bytes only (one
                       4-bit level cannot decode)
  (4, 256, 256, 4, 4)  the defaults
FHE_ERR_UNSUPPORTED of fhe_set_compression_key_seeded (body counts that do not match the parameters) cannot be
reached through the ABI -- the generator and the reader only make handles whose counts match -- and is not
tested."""
import csv
import ctypes as C
import os
import struct

import numpy as np
import pytest

import compress_ref as R
import seeded_compression_ref as SC
import seeded_key_ref as K
from conftest import ROOT
from fhe_sign import (FAST, BigUintFHE, CompressedCiphertextList, CompressedCompressionKey, CompressedServerKey,
                      CompressionKeys, CompressionParams, Context, FheUint, FheUint32, Schnorr, compute_nonce,
                      default_params, generate_keys, multi_bit_params, set_server_key)
from fhe_sign._lib import FheError, load
from lwe_dims import product_params

pytestmark = pytest.mark.gpu
SEED = 0x5EEDC0DE
MASK_SEED = bytes((29 * i + 5) % 256 for i in range(32))
RADIX = 0
NO_KEY, INVALID = -3, -1
SMALL = [R.SMALL_A, SC.MIXED, R.SMALL_B]


def c_params(cp):
    return CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12)


def set_id(cp):
    return f"k{cp.k}N{cp.N}L{cp.L}b{cp.beta}l{cp.ell}"


def ctx_with(sk, key):
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_compression_key(key)
    return ctx


class Env:
    def __init__(self, cp, params, full=True):
        self.cp = cp
        self.ck, self.sk = generate_keys(params, seed=SEED)
        self.priv, self.sck = CompressionKeys.generate_compressed(self.ck, c_params(cp), seed=MASK_SEED)
        self.key = self.sck.decompress()
        self.seeded = ctx_with(self.sk, self.sck)
        self.full = ctx_with(self.sk, self.key) if full else None

    def contexts(self):
        return [c for c in (self.seeded, self.full) if c is not None]

    def close(self):
        set_server_key(None)
        for c in self.contexts():
            c.close()

    def host(self, x, lst):
        """fhe_compress_host under the expanded key on the exported blocks, with the degrees the GPU list carries"""
        _, cnt, degrees, _ = R.parse_list(self.cp, lst.serialize())
        return CompressedCiphertextList.compress_host(self.key, x.export(), degrees, RADIX, cnt)


@pytest.fixture(scope="module", params=SMALL + [SC.STRIDE, R.DEFAULT], ids=set_id)
def env(request):
    """the small sets under a main key of LWE dimension k' N' (the re-keyed oracle then shares its big key),
    the stride set under n = 16"""
    cp = request.param
    params = default_params() if cp is R.DEFAULT else product_params(cp.k * cp.N if cp in SMALL else 16)
    e = Env(cp, params)
    yield e
    e.close()


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits)


def _words(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint8)


# ------------------------------------------------------------------ the install
def test_device_state_is_the_full_installs(env):
    got, want = env.seeded.export_compression_state(), env.full.export_compression_state()
    cp = env.cp
    assert got[0].size == 8 * ((R.cols(cp) + 15) // 16) * 32 * cp.ell * 1024
    for name, a, b in zip(("byte planes", "Fourier BSK", "Fourier BSK, E layout"), got, want):
        assert a.size == b.size and np.array_equal(_words(a), _words(b)), name
    assert got[0].any() and got[1].any() and got[2].any()


def test_compression_is_byte_identical_to_the_host(env):
    cp = env.cp
    set_server_key(env.seeded)
    for B in (1, 257 if cp is R.DEFAULT else cp.L + 1):
        v = _value(2 * B, 7)
        x = FheUint.try_encrypt(v, env.ck, bits=2 * B)
        lst = x.compress()
        assert lst.serialize() == env.host(x, lst).serialize()
        if cp is not SC.STRIDE:
            assert lst.decrypt(env.priv) == v


def test_decompression_words(env):
    """equal between the two contexts; at the defaults B = 1 is the latency kernel and 257 the throughput
    kernel; at the small sets the words are also the re-keyed oracle's under the expanded BSK"""
    cp = env.cp
    kn = cp.k * cp.N
    ok = None
    if cp in SMALL:
        ok = K.rekeyed_oracle(SEED, kn, 1, np.zeros(R.N_BIG * 5 * (kn + 1), np.uint64), env.key.export()[1])
    for B in (1, 257 if cp is R.DEFAULT else max(16, cp.L + 1) if cp in SMALL else cp.L + 1):
        vals = [(5 * i + 3) % 16 for i in range(B)]
        lst = CompressedCiphertextList.compress_host(env.key, env.ck.encrypt_blocks(vals), 15, RADIX, 2 * B)
        out = []
        for ctx in env.contexts():
            set_server_key(ctx)
            out.append(lst.decompress().export())
        assert np.array_equal(out[0], out[1])
        if ok is not None:
            rows = R.extract_rows(cp, R.parse_list(cp, lst.serialize())[3])
            assert np.array_equal(out[0], R.oracle_decompress(ok, rows))
        if cp is not SC.STRIDE:
            assert [env.ck.decrypt_block(c) for c in out[0]] == vals


# ------------------------------------------------------------------ keys
@pytest.fixture(scope="module")
def dflt():
    e = Env(R.DEFAULT, default_params())
    yield e
    e.close()


def _same_bytes(e, ctx):
    set_server_key(ctx)
    x = FheUint32.try_encrypt(0x9E3779B9, e.ck)
    lst = x.compress()
    assert lst.serialize() == e.host(x, lst).serialize()
    assert lst.decrypt(e.priv) == 0x9E3779B9
    assert lst.decompress().decrypt(e.ck) == 0x9E3779B9


def test_multi_bit_main_key_with_the_classic_seeded_key():
    e = Env(R.DEFAULT, multi_bit_params(), full=False)
    try:
        set_server_key(e.seeded)
        y = FheUint32.try_encrypt(0xC0FFEE11, e.ck)
        lst = y.compress()
        assert lst.serialize() == e.host(y, lst).serialize()
        assert lst.decrypt(e.priv) == 0xC0FFEE11
        assert (lst.decompress() + 5).decrypt(e.ck) == 0xC0FFEE16
    finally:
        e.close()


def test_rekeying_full_seeded_full_and_the_drop_by_a_server_key_install(dflt):
    e, ctx = dflt, dflt.full
    want = dflt.seeded.export_compression_state()
    for key in (e.key, e.sck, e.key, e.sck):
        ctx.set_compression_key(key)
        assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(ctx.export_compression_state(), want))
        _same_bytes(e, ctx)
    x = FheUint32.try_encrypt(7, e.ck)
    lst = x.compress()
    ctx.set_server_key(e.sk)  # drops the compression key
    x = FheUint32.try_encrypt(7, e.ck)
    try:
        for call in (x.compress, lst.decompress, ctx.export_compression_state):
            with pytest.raises(FheError, match="compression key") as err:
                call()
            assert err.value.code == NO_KEY
    finally:
        ctx.set_compression_key(e.sck)
    _same_bytes(e, ctx)
    ctx.set_compression_key(e.key)


def test_statuses_leave_the_installed_key_in_place(dflt):
    e, ctx, lib = dflt, dflt.seeded, load()
    assert lib.fhe_set_compression_key_seeded(ctx.handle, None) == INVALID
    assert lib.fhe_set_compression_key_seeded(None, e.sck.handle) == INVALID
    _same_bytes(e, ctx)
    other_ck, _ = generate_keys(product_params(16), seed=SEED)
    _, other = CompressionKeys.generate_compressed(other_ck, c_params(R.SMALL_A), seed=MASK_SEED)
    with pytest.raises(FheError, match="lwe_dimension") as err:
        ctx.set_compression_key(other)
    assert err.value.code == INVALID
    _same_bytes(e, ctx)
    mb_ck, _ = generate_keys(multi_bit_params(), seed=SEED)
    _, mb = CompressionKeys.generate_compressed(mb_ck, c_params(R.SMALL_A), seed=MASK_SEED)
    with pytest.raises(FheError, match="differs from the context's server key") as err:
        ctx.set_compression_key(mb)
    assert err.value.code == INVALID
    _same_bytes(e, ctx)
    bare = Context(0)
    try:
        with pytest.raises(FheError, match="server key") as err:
            bare.set_compression_key(e.sck)
        assert err.value.code == NO_KEY
        assert lib.fhe_ctx_export_compression_state(bare.handle, None, 0, None, 0, None, 0) == NO_KEY
    finally:
        bare.close()
    small = np.zeros(16, np.int8)
    assert lib.fhe_ctx_export_compression_state(ctx.handle, small.ctypes.data, small.size, None, 0, None, 0) == INVALID
    _same_bytes(e, ctx)


# ------------------------------------------------------------------ end to end
def test_client_to_bytes_to_server():
    """both keys leave the client in their seeded forms, with OS-entropy seeds, and are installed from bytes;
    the signer's value for BIP-340 vector 0 comes back compressed and decrypts without a context"""
    ck, _ = generate_keys(seed=SEED)
    sk_wire = CompressedServerKey.new(ck).serialize()
    priv, sck = CompressionKeys.generate_compressed(ck)
    ck_wire = sck.serialize()
    del sck
    assert len(sk_wire) == K.wire_len(834, 1) == 27_410_532
    assert len(ck_wire) == SC.wire_len(R.DEFAULT) == 50_331_776
    ctx = Context(0)
    try:
        ctx.set_server_key(CompressedServerKey.deserialize(sk_wire))
        ctx.set_compression_key(CompressedCompressionKey.deserialize(ck_wire))
        set_server_key(ctx)
        rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
        row = next(r for r in rows if r["index"] == "0")
        d = int(row["secret key"], 16)
        msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
        k, e, _ = Schnorr().sign_prologue(msg, compute_nonce(d, msg, aux), d)
        k, e = (int.from_bytes(bytes(v), "big") if not isinstance(v, int) else v for v in (k, e))
        s = BigUintFHE.new(e, ck).mul(BigUintFHE.new(d, ck), FAST).add(BigUintFHE.new(k, ck), FAST)
        wire = s.compress().serialize()
        assert len(wire) == c_params(R.DEFAULT).wire_bytes(16 * len(s))
        assert CompressedCiphertextList.deserialize(wire).decrypt(priv) == k + e * d
    finally:
        set_server_key(None)
        ctx.close()
