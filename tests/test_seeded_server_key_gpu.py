"""The seeded (compressed) server key installed on the GPU: fhe_set_server_key_seeded
(csrc/seeded_key.hip k_expand_ksk / k_expand_bsk_fourier, then the common tail of fhe_set_server_key)
against the full install of the host-expanded key, which tests/test_seeded_server_key.py pins word for
word, and against the oracle re-keyed to the expanded words.  Every comparison is exact.

    n      grouping  reaches in k_expand_ksk (rows of n + 1 words, ChaCha blocks of 8)
    1      cl        one mask word: a lone 8-byte store next to the body; 7 spare words dropped
    7      cl        odd n below one block: three pairs and the straddling word
    8      cl        exactly one block, no spare word; rows of 9 words: every other row 16-byte aligned
    9      cl        one word into the second block
    2, 16  mb        even rows only; 3 GGSWs per pair of key bits in k_expand_bsk_fourier
    255    cl        rows of 256 words: every row aligned, the last pair straddles
    256    cl        32 blocks: two of wave 0's four stores full, two empty; rows of 257 words
    834    cl, mb    the default parameters: two waves a row, 105 blocks, 6 spare words
    2048   cl        a row fills its 256-block stride exactly: all four waves, no spare word
"""
import csv
import os
import random

import numpy as np
import pytest

import seeded_key_ref as K
from conftest import ROOT
from fhe_sign import (COMPAT, CompressedBigUintFHE, CompressedServerKey, Context, FheError, FheUint32,
                      Schnorr, compute_nonce, generate_keys, set_server_key)
from lwe_dims import CLASSIC, MULTIBIT, product_params

pytestmark = pytest.mark.gpu
SEED = 0x5EED5E7
MASK_SEED = bytes(range(101, 133))
SMALL = [(1, CLASSIC), (7, CLASSIC), (8, CLASSIC), (9, CLASSIC), (2, MULTIBIT), (16, MULTIBIT), (255, CLASSIC),
         (256, CLASSIC)]
LARGE = [(2048, CLASSIC), (834, CLASSIC), (834, MULTIBIT)]
TABLES = [list(range(16)), [(3 * m + 1) % 16 for m in range(16)], [(m * m + 7) % 16 for m in range(16)]]
PBS_COUNTS = (1, 257, 1024)  # the latency kernel, qy, qz (classic) under the default selection


def set_id(s):
    return f"n{s[0]}-{'mb' if s[1] == MULTIBIT else 'cl'}"


class Env:
    """one context pair per parameter set: `seeded` installed from the bodies on the GPU, `full` from the
    host-expanded key"""

    def __init__(self, n, g):
        self.n, self.g = n, g
        self.ck, _ = generate_keys(product_params(n, g), seed=SEED)
        self.ssk = CompressedServerKey.new(self.ck, seed=MASK_SEED)
        self.sk = self.ssk.decompress()
        self.seeded, self.full = Context(0), Context(0)
        self.seeded.set_server_key(self.ssk)
        self.full.set_server_key(self.sk)
        rng = np.random.default_rng(n)
        self.cts = self.ck.encrypt_blocks(rng.integers(0, 16, 37))
        self.cts.setflags(write=False)

    def close(self):
        self.seeded.close()
        self.full.close()


@pytest.fixture(scope="module", params=SMALL + LARGE, ids=set_id)
def env(request):
    e = Env(*request.param)
    yield e
    e.close()


def _same_words(got, want, what):
    bad = np.flatnonzero(got.reshape(-1).view(np.uint64) != want.reshape(-1).view(np.uint64))
    assert bad.size == 0, f"{what}: {bad.size} mismatching words, first at {bad[:5]}"


def test_fourier_bsk_equals_the_full_install(env):
    assert env.seeded.params.lwe_dimension == env.n and env.seeded.params.grouping == env.g
    got, want = env.seeded.export_fourier_bsk(), env.full.export_fourier_bsk()
    assert got.shape == want.shape == (K.ggsw_count(env.n, env.g) * 4 * 1024 * 2,)
    _same_words(got, want, f"n {env.n}: Fourier BSK")


def test_keyswitch_words_equal_the_rekeyed_oracle(env):
    """FHE_KS_VALU reads d_ksk, FHE_KS_MFMA the byte planes derived from it"""
    ksk, bsk = env.sk.export()
    ok = K.rekeyed_oracle(SEED, env.n, env.g, ksk, bsk, fourier=False)
    want = ok.keyswitch_batch(env.cts)
    try:
        for name, kind in (("valu", 0), ("mfma", 1)):
            env.seeded.set_ks_kernel(kind)
            _same_words(env.seeded.keyswitch(env.cts), want, f"n {env.n}: {name} keyswitch")
    finally:
        env.seeded.set_ks_kernel(1)


def test_bootstrapped_words(env):
    """counts 1, 257 and 1024.  Below n = 834 against the re-keyed oracle; at 834 and 2048 against the
    fully installed context (the oracle's bootstraps there are seconds of CPU each)."""
    ctx, d = env.seeded, 12
    ids = np.array([ctx.lut(t) for t in TABLES], np.uint32)
    assert [env.full.lut(t) for t in TABLES] == list(ids)
    lut_of = np.arange(d, dtype=np.uint32) % len(TABLES)
    if env.n < 834:
        ksk, bsk = env.sk.export()
        ok = K.rekeyed_oracle(SEED, env.n, env.g, ksk, bsk)
        want = ok.pbs_batch(env.cts[:d], np.stack([ok.make_lut(t) for t in TABLES]), lut_of)
    else:
        want = env.full.pbs(env.cts[:d], ids[lut_of])
    values = [env.ck.decrypt_block(c) for c in env.cts[:d]]
    assert [env.ck.decrypt_block(o) for o in want] == [TABLES[int(lut_of[i])][values[i]] for i in range(d)]
    for count in PBS_COUNTS:
        out = ctx.pbs(np.resize(env.cts[:d], (count, 2049)), ids[np.resize(lut_of, count)])
        _same_words(out, np.resize(want, (count, 2049)), f"n {env.n}: {count} bootstraps")


# ---------------------------------------------------------------- re-keying one context
def _radix_ok(ck, x, y):
    a, b = FheUint32.try_encrypt(x, ck), FheUint32.try_encrypt(y, ck)
    assert (a + b).decrypt(ck) == (x + y) % 2**32
    assert (a * b).decrypt(ck) == (x * y) % 2**32


def test_rekey_full_seeded_full():
    """full n = 834 -> seeded n = 16 -> the full key again, in one context: the d_ms stride follows n, a LUT
    registered under the first key bootstraps under each later one, FheUint32 add and mul decrypt"""
    rng = random.Random(834)
    ck834, sk834 = generate_keys(seed=SEED)
    ck16, _ = generate_keys(product_params(16), seed=SEED)
    ssk16 = CompressedServerKey.new(ck16, seed=MASK_SEED)
    ctx = Context(0)
    set_server_key(ctx)
    try:
        ctx.set_server_key(sk834)
        lid = ctx.lut(TABLES[1])
        for ck, key in ((ck834, None), (ck16, ssk16), (ck834, sk834)):
            if key is not None:
                ctx.set_server_key(key)
            assert ctx.lut(TABLES[1]) == lid
            cts = ck.encrypt_blocks(np.arange(16))
            assert [ck.decrypt_block(o) for o in ctx.pbs(np.resize(cts, (300, 2049)), lid)[:16]] == TABLES[1]
            _radix_ok(ck, rng.getrandbits(32), rng.getrandbits(32))
    finally:
        set_server_key(None)
        ctx.close()


def test_broadcast_from_a_root_installed_from_the_seeded_key():
    """fhe_ctx_broadcast_server_key reads the root's device state, which is the full install's: a receiver
    ends with the same Fourier BSK and keyswitch words (two ranks replayed in this process, as
    tests/test_lwe_dims_gpu.py does)"""
    from test_lwe_dims_gpu import _attach_replay
    ck, _ = generate_keys(product_params(16, MULTIBIT), seed=SEED)
    ssk = CompressedServerKey.new(ck, seed=MASK_SEED)
    cts = ck.encrypt_blocks(np.arange(16))
    root, recv, full = Context(0), Context(0), Context(0)
    try:
        root.set_server_key(ssk)
        full.set_server_key(ssk.decompress())
        log = []
        keep = _attach_replay(root, 0, log)
        root.broadcast_server_key(0)
        root.detach_comm()
        keep = _attach_replay(recv, 1, log)
        recv.broadcast_server_key(0)
        recv.detach_comm()
        del keep
        assert not log and recv.params.lwe_dimension == 16 and recv.params.grouping == MULTIBIT
        _same_words(recv.export_fourier_bsk(), full.export_fourier_bsk(), "received Fourier BSK")
        for kind in (0, 1):
            recv.set_ks_kernel(kind)
            full.set_ks_kernel(kind)
            _same_words(recv.keyswitch(cts), full.keyswitch(cts), f"received key, keyswitch kernel {kind}")
        lid = recv.lut(TABLES[1])
        assert [ck.decrypt_block(o) for o in recv.pbs(cts, lid)] == TABLES[1]
    finally:
        for c in (root, recv, full):
            c.close()


# ---------------------------------------------------------------- client -> wire -> server
def test_sign_from_a_compressed_key_and_a_compressed_operand():
    """the client sends CompressedServerKey and CompressedBigUintFHE(d) as bytes; the server installs and
    decompresses both on the GPU and signs BIP-340 vector 0"""
    rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
    row = next(r for r in rows if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    ck, _ = generate_keys(seed=SEED)
    wire_key = CompressedServerKey.new(ck).serialize()  # seeds from OS entropy
    wire_d = CompressedBigUintFHE.new(d, ck).serialize()
    assert len(wire_key) == 27_410_532

    ctx = Context(0)
    set_server_key(ctx)
    try:
        ctx.set_server_key(CompressedServerKey.deserialize(wire_key))
        d_fhe = CompressedBigUintFHE.deserialize(wire_d).decompress()
        sig = Schnorr().sign_fhe_with_k0(msg, compute_nonce(d, msg, aux), d, d_fhe, ck, COMPAT)
        assert sig.hex().upper() == row["signature"].upper()
        del d_fhe
    finally:
        set_server_key(None)
        ctx.close()


# ---------------------------------------------------------------- statuses
def test_statuses_leave_the_context_usable():
    from fhe_sign import _lib
    lib = _lib.load()
    ck, _ = generate_keys(product_params(8), seed=SEED)
    ssk = CompressedServerKey.new(ck, seed=MASK_SEED)
    cts = ck.encrypt_blocks(np.arange(16))
    ctx = Context(0)
    try:
        with pytest.raises(FheError) as e:  # no key yet
            ctx.keyswitch(cts)
        assert e.value.code == -3
        assert lib.fhe_set_server_key_seeded(ctx.handle, None) == -1
        assert lib.fhe_set_server_key_seeded(None, ssk.handle) == -1
        with pytest.raises(FheError) as e:  # still none
            ctx.keyswitch(cts)
        assert e.value.code == -3
        # parameters no kernel takes never become an object: the reader refuses them
        blob = bytearray(ssk.serialize())
        blob[32 + 4:32 + 8] = (22).to_bytes(4, "little")  # pbs_base_log
        with pytest.raises(FheError, match="unsupported parameters") as e:
            CompressedServerKey.deserialize(K.refnv(blob))
        assert e.value.code == -1
        ctx.set_server_key(ssk)
        lid = ctx.lut(TABLES[1])
        assert [ck.decrypt_block(o) for o in ctx.pbs(cts, lid)] == TABLES[1]
        assert lib.fhe_set_server_key_seeded(ctx.handle, None) == -1  # the installed key stays
        assert [ck.decrypt_block(o) for o in ctx.pbs(cts, lid)] == TABLES[1]
    finally:
        ctx.close()
