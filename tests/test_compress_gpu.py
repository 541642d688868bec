"""Compressed computed ciphertexts on the GPU (csrc/compress.hip through Engine::compress / decompress)
against the host definition fhe_compress_host, which tests/test_compress.py pins word for word to
tests/compress_ref.py.  Compression is compared byte for byte; decompression row for row with the numpy
sample extract, word for word with the re-keyed oracle at the small parameter sets and, at the defaults
(LWE dimension k' N' = 1024, every blind-rotate kernel), on 24 rows of a 1024-block list.  The contraction's
64-bit words, which the bytes cannot see below their 12 bits, are pinned in tests/test_pack_keyswitch_gpu.py.

Noise (test_noise_of_stored_values): m = 2^14 blocks, built as tests/test_noise_gpu.py builds its inputs --
8192 type-A combinations 4 s0 + 2 s1 + s2 + c (22 units, covering all 16 values) and 8192 type-B 4 s + 3 c
(25 units) of bootstrapped blocks -- compressed on the GPU, decoded both ways.  The condition is zero decode
failures; the measured sigma of the stored phase error is printed next to the model's.
Measured on an MI355X: sigma 7.46 and 7.81 in two runs (other encryption noise), zero failures both ways.  The
issue's model, 6.6, counts the packing key's noise once; every coefficient of a GLWE collects it from all
b_g blocks packed into it (256 x 0.056 = 14.3 here), which gives 7.7, and the test holds the measurement to
that, within 4 sampling errors of 0.34 (slots of one GLWE are correlated, see the printout)."""
import csv
import math
import os
import struct

import numpy as np
import pytest

import compress_ref as R
import seeded_key_ref as K
from conftest import ROOT
from fhe_sign import (FAST, BigUintFHE, CompressedCiphertextList, CompressionKeys, CompressionParams, Context, FheUint,
                      FheUint32, Schnorr, compute_nonce, generate_keys, multi_bit_params, set_server_key)
from fhe_sign._lib import FheError
from lwe_dims import product_params

pytestmark = pytest.mark.gpu
SEED = 0x5EEDC0DE
RADIX, BIGUINT = 0, 1


def c_params(cp):
    return CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12)


def main_bytes(n, grouping=1):
    return struct.pack("<9I", n, 23, 3, 5, 45, 17, 4, 4, grouping)


class Env:
    def __init__(self, cp, params):
        self.cp = cp
        self.ck, self.sk = generate_keys(params, seed=SEED)
        self.priv, self.key = CompressionKeys.generate(self.ck, c_params(cp))
        self.main = main_bytes(params.lwe_dimension, params.grouping)
        self.ctx = Context(0)
        self.ctx.set_server_key(self.sk)
        self.ctx.set_compression_key(self.key)

    def use(self):
        set_server_key(self.ctx)

    def close(self):
        set_server_key(None)
        self.ctx.close()

    def raw(self, cts, degree, noise=1):
        """an FheUint around given block ciphertexts (through the radix wire format)"""
        return FheUint.deserialize(R.raw_radix_blob(self.main, cts, degree, noise))

    def host(self, x, lst, form=RADIX, count=None):
        """fhe_compress_host on the exported blocks, with the degrees the GPU list carries"""
        blob = lst.serialize()
        _, cnt, degrees, _ = R.parse_list(self.cp, blob)
        cts = x.export() if isinstance(x, FheUint) else np.concatenate([d.export() for d in x.digits])
        return CompressedCiphertextList.compress_host(self.key, cts, degrees, form, cnt if count is None else count)


@pytest.fixture(scope="module")
def env_obj():
    from fhe_sign import default_params
    e = Env(R.DEFAULT, default_params())
    yield e
    e.close()


@pytest.fixture
def env(env_obj):
    env_obj.use()  # this thread's context: another fixture's may be the current one
    return env_obj


@pytest.fixture(scope="module", params=[R.SMALL_A, R.SMALL_B], ids=lambda cp: f"k{cp.k}N{cp.N}")
def small_obj(request):
    """the small sets, under a main key of LWE dimension k' N' (the re-keyed oracle then shares its big key)"""
    cp = request.param
    e = Env(cp, product_params(cp.k * cp.N))
    yield e
    e.close()


@pytest.fixture
def small(small_obj):
    small_obj.use()
    return small_obj


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits)


# ------------------------------------------------------------------ compression
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 515])
def test_compress_is_byte_identical_to_the_host(env, B):
    """1, 2: one partial GLWE; 255 / 256 / 257: around a full one; 515: two full and three (odd: padding)"""
    v = _value(2 * B)
    x = FheUint.try_encrypt(v, env.ck, bits=2 * B)
    lst = x.compress()
    blob = lst.serialize()
    assert blob == env.host(x, lst).serialize()
    assert len(blob) == c_params(env.cp).wire_bytes(B) == R.wire_len(env.cp, B)
    assert lst.decrypt(env.priv) == v


def _raw_rows(cp, B):
    """uniform random rows (no encryptions: nothing is decrypted), the digit edge rows first and last"""
    cts = np.random.default_rng(0xB16 + B).integers(0, 1 << 64, (B, R.BIG_CT), dtype=np.uint64)
    cts[:4] = cts[B - 4:] = R.edge_rows(cp.beta, cp.ell)
    return cts


@pytest.mark.parametrize("B", [2048, 2064, 2352])
def test_large_lists_are_byte_identical_to_the_host(env, B):
    """From 2048 blocks on the contraction is k_pk_mfma<4> (256 rows per workgroup): 2048 fills eight workgroups;
    2064 puts one 16-row tile into a ninth; 2352 leaves the last workgroup with three tiles in wave 0 and waves
    1-3 past the count, reading digit fragments no kernel wrote.  A radix integer ends at 2048 blocks (4096 bits)
    and a BigUintFHE is whole limbs of 16, so 2064 and 2352 are the lists nearest to 2049 and 2367 that a
    compressed list can hold; those two counts themselves are pinned word for word, before the rounding, in
    tests/test_pack_keyswitch_gpu.py.  Raw rows at degree 3, as the edge-row case hands them in"""
    cp, cts = env.cp, _raw_rows(env.cp, B)
    if B <= 2048:
        x, form, count = env.raw(cts, 3), RADIX, 2 * B
    else:
        x, form, count = BigUintFHE.deserialize(R.raw_biguint_blob(env.main, cts, 3)), BIGUINT, B // 16
    lst = x.compress()
    blob = lst.serialize()
    assert lst.nblocks == B
    assert blob == CompressedCiphertextList.compress_host(env.key, cts, 3, form, count).serialize()
    assert len(blob) == c_params(cp).wire_bytes(B) == R.wire_len(cp, B)


def test_large_list_of_real_encryptions_decrypts(env):
    """129 limbs = 2064 blocks (k_pk_mfma<4>, nine GLWEs, the last with 16 bodies): byte for byte the host's, and
    the client reads the value back"""
    v = _value(32 * 129, 11) | 1 << (32 * 129 - 1)  # the top limb is not zero: 129 limbs
    x = BigUintFHE.new(v, env.ck)
    assert len(x) == 129
    lst = x.compress()
    assert lst.nblocks == 2064
    assert lst.serialize() == env.host(x, lst, BIGUINT, 129).serialize()
    assert lst.decrypt(env.priv) == v


@pytest.mark.parametrize("which", ["1", "L+1"])
def test_compress_small_sets(small, which):
    cp = small.cp
    B = 1 if which == "1" else cp.L + 1
    v = _value(2 * B, 3)
    x = FheUint.try_encrypt(v, small.ck, bits=2 * B)
    lst = x.compress()
    assert lst.serialize() == small.host(x, lst).serialize()
    assert lst.decrypt(small.priv) == v


def test_every_block_value_and_degree(env):
    """blocks of all 16 values (degree 15) and the digit edge rows, handed in raw"""
    vals = [(7 * i + 2) % 16 for i in range(32)]
    x = env.raw(env.ck.encrypt_blocks(vals), 15)
    lst = x.compress()
    assert lst.serialize() == env.host(x, lst).serialize()
    assert R.decrypt_values(env.cp, R.parse_list(env.cp, lst.serialize())[3], env.priv.export())[0] == vals
    edges = env.raw(R.edge_rows(env.cp.beta, env.cp.ell), 3)
    le = edges.compress()
    assert le.serialize() == env.host(edges, le).serialize()


def test_trivial_blocks_go_through_as_zero_mask_ciphertexts(env):
    t = FheUint.encrypt_trivial(0x1B, bits=8)  # blocks 3, 2, 1, 0
    lst = t.compress()
    assert lst.serialize() == env.host(t, lst).serialize()
    assert lst.decrypt(env.priv) == 0x1B
    assert lst.decompress().decrypt(env.ck) == 0x1B


def test_recycled_slots_and_a_pending_graph(env):
    a = FheUint32.try_encrypt(0x9E3779B9, env.ck)
    la = a.compress()
    del a  # its slots go back to the pool and are handed out again
    b = FheUint32.try_encrypt(0x7F4A7C15, env.ck)
    lb = b.compress()
    assert lb.serialize() == env.host(b, lb).serialize() != la.serialize()
    x, y = FheUint32.try_encrypt(0x12345679, env.ck), FheUint32.try_encrypt(0x0BADF00D, env.ck)
    p = x * y  # recorded, not launched: compress flushes what p depends on
    lp = p.compress()
    assert lp.decrypt(env.priv) == (0x12345679 * 0x0BADF00D) % 2**32
    assert lp.serialize() == env.host(p, lp).serialize()
    assert la.decrypt(env.priv) == 0x9E3779B9 and lb.decrypt(env.priv) == 0x7F4A7C15


# ------------------------------------------------------------------ decompression
def test_unpack_rows_and_oracle_words_small_sets(small):
    cp = small.cp
    kn = cp.k * cp.N
    B = 2 * cp.L + 1
    vals = [(5 * i + 3) % 16 for i in range(B)]
    lst = CompressedCiphertextList.compress_host(small.key, small.ck.encrypt_blocks(vals), 15, RADIX, 2 * B)
    want_rows = R.extract_rows(cp, R.parse_list(cp, lst.serialize())[3])
    assert np.array_equal(lst.extract_rows(), want_rows)
    ok = K.rekeyed_oracle(SEED, kn, 1, np.zeros(R.N_BIG * 5 * (kn + 1), np.uint64), small.key.export()[1])
    x = lst.decompress()
    got = x.export()
    assert np.array_equal(got, R.oracle_decompress(ok, want_rows))
    assert [small.ck.decrypt_block(c) for c in got] == vals


def test_unpack_rows_at_the_defaults(env):
    B = 257
    lst = CompressedCiphertextList.compress_host(env.key, env.ck.encrypt_blocks([i % 16 for i in range(B)]), 15, RADIX, 2 * B)
    assert np.array_equal(lst.extract_rows(), R.extract_rows(env.cp, R.parse_list(env.cp, lst.serialize())[3]))
    # nine GLWEs, the last with 16 bodies: 129 limbs, the shortest list past 2048 blocks
    B = 2064
    lst = CompressedCiphertextList.compress_host(env.key, env.ck.encrypt_blocks([i % 16 for i in range(B)]), 15, BIGUINT, B // 16)
    glwes = R.parse_list(env.cp, lst.serialize())[3]
    assert [len(g) - env.cp.k * env.cp.N for g in glwes] == [256] * 8 + [16]
    assert np.array_equal(lst.extract_rows(), R.extract_rows(env.cp, glwes))


def test_decompress_latency_and_throughput_kernels(env):
    """B = 1: the latency kernel; 257 > wide_threshold: the throughput kernel; the same 257 again with the
    threshold raised: the latency kernel -- equal words"""
    one = FheUint.try_encrypt(2, env.ck, bits=2).compress()
    assert one.decompress().decrypt(env.ck) == 2
    vals = [(3 * i + 1) % 16 for i in range(257)]
    lst = CompressedCiphertextList.compress_host(env.key, env.ck.encrypt_blocks(vals), 15, RADIX, 514)
    thr = lst.decompress().export()
    assert [env.ck.decrypt_block(c) for c in thr] == vals
    env.ctx.set_wide_threshold(512)
    try:
        lat = lst.decompress().export()
    finally:
        env.ctx.set_wide_threshold(256)
    assert np.array_equal(lat, thr)


@pytest.fixture(scope="module")
def oracle_1024(env_obj):
    """the oracle re-keyed at n = k' N' = 1024 with the default set's decompression BSK (it shares the big key)"""
    kn = R.DEFAULT.k * R.DEFAULT.N
    return K.rekeyed_oracle(SEED, kn, 1, np.zeros(R.N_BIG * 5 * (kn + 1), np.uint64), env_obj.key.export()[1])


def test_decompress_words_at_the_defaults(env, oracle_1024):
    """The decompression bootstrap at the default set runs at LWE dimension k' N' = 1024, which no other test
    pins word for word.  1024 blocks of all 16 values, compressed on the GPU, decompressed four ways: as the
    product does (FHE_BR_AUTO: 1024 fills qz's rounds, the second Fourier layout), under FHE_BR_QY, with the wide
    threshold at 1024 (the latency kernel), and in centered modulus-switch mode (the rows are multiples of 2^52:
    centring changes nothing).  All words equal; the first, the middle (across the 512 seam) and the last eight
    rows equal the re-keyed oracle's"""
    cp, ctx, B = env.cp, env.ctx, 1024
    vals = [(11 * i + 5) % 16 for i in range(B)]
    x = env.raw(env.ck.encrypt_blocks(vals), 15)
    lst = x.compress()
    assert lst.serialize() == env.host(x, lst).serialize()
    rows = R.extract_rows(cp, R.parse_list(cp, lst.serialize())[3])
    assert rows.shape == (B, cp.k * cp.N + 1) and not (rows & np.uint64((1 << 52) - 1)).any()
    out = {}
    try:
        out["auto (qz)"] = lst.decompress().export()
        ctx.set_br_kernel(4)  # FHE_BR_QY
        out["qy"] = lst.decompress().export()
        ctx.set_br_kernel(7)  # FHE_BR_AUTO
        ctx.set_wide_threshold(1024)
        out["latency"] = lst.decompress().export()
        ctx.set_wide_threshold(256)
        ctx.set_modulus_switch("centered")
        out["centered"] = lst.decompress().export()
    finally:
        ctx.set_br_kernel(7)
        ctx.set_wide_threshold(256)
        ctx.set_modulus_switch("standard")
    assert len(out) == 4
    for name, words in out.items():
        assert words.shape == (B, R.BIG_CT)
        assert np.array_equal(words, out["auto (qz)"]), name
    sel = np.r_[0:8, 508:516, 1016:1024]
    want = R.oracle_decompress(oracle_1024, rows[sel])
    for name, words in out.items():
        bad = [int(i) for i, a, b in zip(sel, words[sel], want) if not np.array_equal(a, b)]
        assert not bad, f"{name}: rows {bad} differ from the oracle"
    assert [env.ck.decrypt_block(c) for c in out["auto (qz)"]] == vals


def test_multi_bit_main_key_with_a_classic_decompression_key(env):
    e = Env(R.DEFAULT, multi_bit_params())
    e.use()
    try:
        vals = list(range(16)) * 2
        x = e.raw(e.ck.encrypt_blocks(vals), 15)
        lst = CompressedCiphertextList.deserialize(x.compress().serialize())
        assert lst.serialize() == e.host(x, lst).serialize()
        assert [e.ck.decrypt_block(c) for c in lst.decompress().export()] == vals
        y = FheUint32.try_encrypt(0xC0FFEE11, e.ck)
        assert (y.compress().decompress() + 5).decrypt(e.ck) == 0xC0FFEE16
    finally:
        e.close()
        env.use()


# ------------------------------------------------------------------ keys and refusals
def test_compression_key_does_not_survive_a_server_key_install(env):
    x = FheUint32.try_encrypt(7, env.ck)
    lst = x.compress()
    env.ctx.set_server_key(env.sk)
    x = FheUint32.try_encrypt(7, env.ck)
    try:
        for call in (x.compress, lst.decompress):
            with pytest.raises(FheError, match="compression key") as e:
                call()
            assert e.value.code == -3  # FHE_ERR_NO_KEY
    finally:
        env.ctx.set_compression_key(env.key)
    assert x.compress().decompress().decrypt(env.ck) == 7


def test_refusals(env):
    other_ck, _ = generate_keys(product_params(16), seed=SEED)
    _, other = CompressionKeys.generate(other_ck, c_params(R.SMALL_A))
    with pytest.raises(FheError, match="lwe_dimension") as e:
        env.ctx.set_compression_key(other)
    assert e.value.code == -1
    bare = Context(0)
    try:
        with pytest.raises(FheError) as e:
            bare.set_compression_key(env.key)
        assert e.value.code == -3
    finally:
        bare.close()
    x = FheUint32.try_encrypt(7, env.ck)
    lst = x.compress()  # the installed key is untouched
    # a list of other compression parameters, or of the other form, is refused before anything is launched
    small_ck, _ = generate_keys(seed=SEED)
    _, small_key = CompressionKeys.generate(small_ck, c_params(R.SMALL_A))
    foreign = CompressedCiphertextList.compress_host(small_key, small_ck.encrypt_blocks([1] * 16), 3, RADIX, 32)
    with pytest.raises(FheError, match="compression parameters"):
        foreign.decompress()
    blob = bytearray(lst.serialize())
    struct.pack_into("<I", blob, 32 + 6 * 4, 2)  # message_modulus 4 -> 2
    with pytest.raises(FheError, match="message_modulus"):
        CompressedCiphertextList.deserialize(K.refnv(blob)).decompress()
    big = BigUintFHE.new(7, env.ck).compress()
    from fhe_sign._lib import load
    import ctypes as C
    h = C.c_void_p()
    assert load().fhe_compressed_expand_radix(env.ctx.handle, big.handle, C.byref(h)) == -1
    assert load().fhe_compressed_expand_biguint(env.ctx.handle, lst.handle, C.byref(h)) == -1
    assert lst.decompress().decrypt(env.ck) == 7


# ------------------------------------------------------------------ end to end
def test_signers_value_compressed_to_the_client_and_back(env):
    """BIP-340 vector 0: k + e d through the existing ops, compress + serialize on the server, deserialize +
    decrypt on the client (no context), then decompress and add 1 on the GPU"""
    rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
    row = next(r for r in rows if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    k, e, _ = Schnorr().sign_prologue(msg, compute_nonce(d, msg, aux), d)
    k, e = (int.from_bytes(bytes(v), "big") if not isinstance(v, int) else v for v in (k, e))
    s = BigUintFHE.new(e, env.ck).mul(BigUintFHE.new(d, env.ck), FAST).add(BigUintFHE.new(k, env.ck), FAST)
    wire = s.compress().serialize()
    nblocks = 16 * len(s)
    assert len(wire) == c_params(env.cp).wire_bytes(nblocks) == 108 + nblocks + R.glwe_bytes(env.cp, nblocks - 256 * ((nblocks - 1) // 256)) \
        + R.glwe_bytes(env.cp, 256) * ((nblocks - 1) // 256)
    got = CompressedCiphertextList.deserialize(wire)
    assert got.decrypt(env.priv) == k + e * d
    back = got.decompress()
    assert isinstance(back, BigUintFHE) and len(back) == len(s)
    assert back.add(BigUintFHE.new(1, env.ck), FAST).to_biguint(env.ck) == k + e * d + 1
    # the same as one 256-bit FheUint: 1,728 payload bytes + 128 degree bytes + the 108-byte header
    x = FheUint.try_encrypt((k + e * d) % 2**256, env.ck, bits=256)
    y = (x + 0).compress().serialize()
    assert len(y) == 108 + 128 + 1728
    assert CompressedCiphertextList.deserialize(y).decrypt(env.priv) == (k + e * d) % 2**256


# ------------------------------------------------------------------ noise
def test_noise_of_stored_values(env):
    C_ = 8192  # combinations of each type: m = 2 C_ = 2^14 blocks
    ck, ctx, cp = env.ck, env.ctx, env.cp
    rs = np.random.default_rng(0xF00D)
    sv, cv = rs.integers(0, 3, C_), rs.integers(0, 2, C_)
    # bootstrapped blocks of unit noise, as the radix layer's carry prefix sees them
    pool_s = ctx.pbs(ck.encrypt_blocks(sv), ctx.lut([x % 3 for x in range(16)]))
    pool_c = ctx.pbs(ck.encrypt_blocks(cv), ctx.lut([x % 2 for x in range(16)]))
    p = [rs.permutation(C_) for _ in range(5)]
    with np.errstate(over="ignore"):
        a = np.uint64(4) * pool_s[p[0]] + np.uint64(2) * pool_s[p[1]] + pool_s[p[2]] + pool_c[p[3]]  # 22 units
        b = np.uint64(4) * pool_s[p[1]] + np.uint64(3) * pool_c[p[4]]                                # 25 units
    m_a = 4 * sv[p[0]] + 2 * sv[p[1]] + sv[p[2]] + cv[p[3]]
    m_b = 4 * sv[p[1]] + 3 * cv[p[4]]
    vals = [int(v) for v in np.concatenate([m_a, m_b])]
    assert set(vals) == set(range(16))
    blob = R.raw_biguint_blob(env.main, np.concatenate([a, b]), 15, 25)
    x = BigUintFHE.deserialize(blob)
    lst = CompressedCiphertextList.deserialize(x.compress().serialize())
    assert lst.nblocks == 2 * C_
    got, phases = R.decrypt_values(cp, R.parse_list(cp, lst.serialize())[3], env.priv.export())
    err = (np.array(phases) - 128 * np.array(vals) + 2048) % 4096 - 2048
    sigma, worst = float(err.std()), int(np.abs(err).max())
    fails_direct = sum(g != v for g, v in zip(got, vals))
    back = lst.decompress()
    out = np.concatenate([d.export() for d in back.digits])
    fails_pbs = sum(ck.decrypt_block(c) != v for c, v in zip(out, vals))
    # the model of DESIGN.md 6c, from this run's own inputs: the modulus switch with s' actual weight, the
    # decomposition rounding, the packing key's noise ONCE PER BLOCK OF THE GLWE (every coefficient of G_g
    # collects the key noise of all b_g rotated T_i, here b_g = L), and the inputs' measured noise
    _, S = ck.export()
    cts = np.concatenate([a, b])
    with np.errstate(over="ignore"):
        ph_in = cts[:, 2048] - (cts[:, :2048] * S).sum(axis=1, dtype=np.uint64) - np.array(vals, np.uint64) * np.uint64(1 << 59)
    var_in = float((ph_in.astype(np.int64) / 2.0 ** 52).var())
    weight = int(env.priv.export().sum())
    var_ms = (1 + weight) / 12
    var_dec = 1024 * (2.0 ** 48) ** 2 / 12 / 2.0 ** 104
    var_key = 2048 * cp.ell * 21.5 * (2.0 ** 84 / 3) / 2.0 ** 104  # per block; E[d^2] = 21.5 for digits in [-8, 7]
    model = math.sqrt(var_ms + var_dec + cp.L * var_key + var_in)
    corr = 1 + (cp.L - 1) / 4  # sum over the other slots of the squared correlation 1/2
    samp = sigma * 0.5 * math.sqrt(2 * corr / (2 * C_))
    print(f"\ncompression noise: m = {2 * C_} blocks at 22 / 25 units, stored phase error sigma = {sigma:.2f} of a half "
          f"step of 64 (the issue's model, one block per GLWE: 6.6; with L = {cp.L} blocks per GLWE: {model:.2f} = sqrt("
          f"{var_ms:.2f} modulus switch at weight {weight} + {var_dec:.2f} rounding + {cp.L} x {var_key:.4f} packing key + "
          f"{var_in:.2f} input)), max |error| = {worst}, mean = {err.mean():.2f}; decode failures: direct {fails_direct}, "
          f"decompress {fails_pbs}; sampling error of sigma = {samp:.2f} (the slots of a GLWE share its mask's rounding "
          f"errors through a key of mean 1/2: neighbouring slots correlate by about 1/2, so m samples weigh as m / {corr:.0f})")
    assert fails_direct == 0 and fails_pbs == 0
    assert abs(sigma - model) < 4 * samp
