"""x mod (2^k - c) under encryption on the GPU, and the signer that reduces s mod n before anything is decrypted
(fhe_radix_rem_pseudo_mersenne, fhe_schnorr_sign_fhe_with_k0_reduced, fhe_schnorr_eval_s).  Values against
Python's % and the plaintext signer; bootstrap and level counts against the dry run (tests/test_mod_reduce.py
checks the algorithm itself on the CPU) and against the general `%` this specialisation has to beat."""
import csv
import ctypes as C
import os
import random

import pytest

import compress_ref as CR
from conftest import ROOT
from fhe_sign import (COMPAT, FAST, PUBLIC, SECP256K1_N_C, BigUintFHE, CompactPublicKey, CompressionKeys,
                      CompressionParams, Context, FheUint, FheUint32, FheUint256, Schnorr, _lib, compute_nonce,
                      generate_keys, multi_bit_params, public_key_x, set_server_key, stats)
from fhe_sign.schnorr import CURVE_ORDER as N
from test_mod_reduce import dry_rem

pytestmark = pytest.mark.gpu
ROWS = {r["index"]: r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))}


@pytest.fixture(scope="module", params=["classic", "multibit"])
def env_obj(request):
    """classic (grouping 1) and multi-bit (grouping 2) blind rotation, as tests/test_sign_gpu.py"""
    ck, sk = generate_keys(multi_bit_params() if request.param == "multibit" else None, seed=0x5167)
    ctx = Context(0)
    ctx.set_server_key(sk)
    yield ck, ctx
    set_server_key(None)
    ctx.close()


@pytest.fixture
def env(env_obj):
    set_server_key(env_obj[1])  # this thread's context: another fixture's may be the current one
    return env_obj


@pytest.fixture(scope="module")
def keyed():
    """classic keys with a public key (re-randomization) and a compression key installed"""
    ck, sk = generate_keys(seed=0x5168)
    cp = CR.DEFAULT
    priv, ckey = CompressionKeys.generate(ck, CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12))
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_public_key(CompactPublicKey.new(ck))
    ctx.set_compression_key(ckey)
    yield ck, ctx, priv, sk
    set_server_key(None)
    ctx.close()


def _vector(idx):
    row = ROWS[idx]
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    return msg, compute_nonce(d, msg, aux), d, row


def test_rem_32_to_16_bits(env):
    ck, _ = env
    n = 2**16 - 15
    values = [0, n, n - 1, 2 * n - 1, 2**32 - 1, random.Random(0x3216).getrandbits(32)]
    outs = [FheUint32.try_encrypt(v, ck).rem_pseudo_mersenne(16, 15) for v in values]
    assert [r.bits for r in outs] == [16] * 6
    assert [r.decrypt(ck) for r in outs] == [v % n for v in values]


@pytest.fixture(scope="module")
def dry512():
    d = dry_rem(512, 256, SECP256K1_N_C)
    assert d["folds"] == 3
    return d["pbs"], d["levels"]


@pytest.mark.parametrize("which", ["ones", "square", "random"])
def test_rem_512_to_256_beats_the_general_rem(env, dry512, which):
    """the same operand through the folds and through `%` (the general multiplier / residue division): equal
    values, and the folds strictly cheaper in bootstraps and in levels -- the condition for having them.  The
    counts are deterministic and equal the dry run's."""
    ck, ctx = env
    v = {"ones": 2**512 - 1, "square": (N - 1)**2 + (N - 1), "random": random.Random(0x512).getrandbits(512)}[which]
    x = FheUint.try_encrypt(v, ck, bits=512)
    s0 = stats(ctx)
    r = x.rem_pseudo_mersenne(256, SECP256K1_N_C)
    got = r.decrypt(ck)
    s1 = stats(ctx)
    want = (x % N).decrypt(ck)
    s2 = stats(ctx)
    folds = (s1[0] - s0[0], s1[1] - s0[1])
    general = (s2[0] - s1[0], s2[1] - s1[1])
    print(f"\n512 -> 256 mod n: folds {folds[0]} bootstraps / {folds[1]} levels, general % {general[0]} / {general[1]}")
    assert got == want == v % N
    assert isinstance(r, FheUint256) and r.export().shape == (128, 2049)
    assert folds[0] < general[0] and folds[1] < general[1]
    assert folds == dry512


@pytest.mark.parametrize("idx,mode", [("0", COMPAT), ("1", COMPAT), ("15", FAST), ("1", FAST), ("0", PUBLIC),
                                      ("1", PUBLIC)])
def test_reduced_signer_bip340(env, idx, mode):
    ck, _ = env
    msg, k0, d, row = _vector(idx)
    s = Schnorr()
    d_fhe = BigUintFHE.new(d, ck)
    sig = s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, mode, reduce=True)
    assert sig == s.sign_with_k0(msg, k0, d)
    assert sig.hex().upper() == row["signature"].upper()
    assert Schnorr.verify(msg, public_key_x(d), sig)
    # the server's half alone: Enc(s) and nothing else, 128 clean blocks
    k, e, _ = s.sign_prologue(msg, k0, d)
    if mode == PUBLIC:
        s_enc = s.eval_s(e, k, d_fhe, PUBLIC)
    else:
        s_enc = s.eval_s(BigUintFHE.new(e, ck), BigUintFHE.new(k, ck), d_fhe, mode)
    bits = C.c_uint32()
    assert _lib.load().fhe_radix_num_bits(s_enc.handle, C.byref(bits)) == 0 and bits.value == 256
    assert isinstance(s_enc, FheUint256) and s_enc.export().shape == (128, 2049)
    val = s_enc.decrypt(ck)
    assert val < N and val == int.from_bytes(sig[32:], "big")
    assert (s_enc + 1).decrypt(ck) == val + 1  # clean blocks: the existing ops take it as it is


def test_reduced_sign_fhe_and_call_site(env):
    ck, _ = env
    s = Schnorr()
    sig = s.sign_fhe(bytes(32), bytes(32), 3, ck, reduce=True)
    assert sig.hex().upper() == ROWS["0"]["signature"].upper()
    msg, k0, d, row = _vector("1")
    d_fhe = BigUintFHE.new(d, ck)
    assert s.sign_fhe_with_k0_callsite(msg, k0, d, d_fhe, ck, COMPAT, reduce=True).hex().upper() == row["signature"].upper()


@pytest.mark.parametrize("mode", [COMPAT, PUBLIC])
def test_reduced_batch_equals_single_calls(env, mode):
    ck, _ = env
    s = Schnorr()
    jobs = []
    for idx in ("0", "1"):
        msg, k0, d, _ = _vector(idx)
        jobs.append((msg, k0, d, BigUintFHE.new(d, ck)))
    got = s.sign_fhe_with_k0_batch(jobs, ck, mode, reduce=True)
    assert got == [s.sign_fhe_with_k0(m, k0, d, f, ck, mode, reduce=True) for m, k0, d, f in jobs]
    assert got == [s.sign_with_k0(m, k0, d) for m, k0, d, _ in jobs]


def test_combinations(keyed):
    """with rerandomize_domain=, through compress(), and under the centered modulus switch: the same bytes"""
    ck, ctx, priv, _ = keyed
    set_server_key(ctx)
    msg, k0, d, row = _vector("1")
    s = Schnorr()
    want = s.sign_with_k0(msg, k0, d)
    d_fhe = BigUintFHE.new(d, ck)
    before = d_fhe.digest()
    assert s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT, rerandomize_domain=b"tests/reduce", reduce=True) == want
    assert d_fhe.digest() == before
    k, e, _ = s.sign_prologue(msg, k0, d)
    s_enc = s.eval_s(e, k, d_fhe, PUBLIC)
    assert s_enc.compress().decrypt(priv) == int.from_bytes(want[32:], "big")
    assert s_enc.re_randomize(bytes(range(32))).decrypt(ck) == int.from_bytes(want[32:], "big")
    assert FheUint.deserialize(s_enc.serialize()).decrypt(ck) == int.from_bytes(want[32:], "big")
    ctx.set_modulus_switch("centered")
    try:
        assert s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, FAST, reduce=True) == want
        assert s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, PUBLIC, reduce=True) == want
    finally:
        ctx.set_modulus_switch("standard")


def test_reduced_signer_fanout_emulated_world_2(keyed):
    """the fan-out scatters slices by recording order: the reduced signer at an emulated world of 2 (levels of
    >= 257 bootstraps split, the production threshold) gives the same bytes"""
    ck, _, _, sk = keyed
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_fanout(min_level=257, emulate_ranks=2)
    set_server_key(ctx)
    try:
        msg, k0, d, row = _vector("1")
        s = Schnorr()
        d_fhe = BigUintFHE.new(d, ck)
        for mode in (COMPAT, PUBLIC):
            assert s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, mode, reduce=True).hex().upper() == row["signature"].upper()
        _, world, split = ctx.fanout_info()
        assert world == 2 and split > 0
        del d_fhe
    finally:
        set_server_key(None)
        ctx.close()
