"""Re-randomization under the compact public key on the GPU: FheUint.re_randomize / BigUintFHE.re_randomize
(csrc/rerandomize.hip k_rerand_zero + k_rerand_add through Engine::rerandomize) against fhe_rerandomize_host,
which tests/test_rerandomize.py pins word for word to its own numpy restatement.  Every comparison of ciphertext
words is exact."""
import csv
import json
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
from fhe_sign import (COMPAT, BigUintFHE, CompactCiphertextList, CompactPublicKey, Context, FheUint, FheUint32, Schnorr,
                      compute_nonce, generate_keys, multi_bit_params, rerandomization_seed, rerandomize_host,
                      rerandomize_rows, set_server_key)
from fhe_sign._lib import FheError

pytestmark = pytest.mark.gpu
SEED_A, SEED_B = bytes(range(3, 35)), bytes(range(103, 135))
N = 2048


@pytest.fixture(scope="module")
def env():
    ck, sk = generate_keys(seed=0x5EED13)
    pk = CompactPublicKey.deserialize(CompactPublicKey.new(ck).serialize())  # as a server without the secret holds it
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    yield ck, pk, ctx, sk
    set_server_key(None)
    ctx.close()


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits)


def _block_meta(x):
    """(degree, noise) of every block of an FheUint, from its serialized form (kind 3: per block a tag byte,
    u32 degree, u32 noise, 2049 words); every block must be a ciphertext, not a trivial block"""
    blob = x.serialize()
    bits, nb = struct.unpack_from("<II", blob, 32 + 36)
    assert bits == x.bits and nb == bits // 2
    out, off = [], 32 + 36 + 8
    for _ in range(nb):
        tag, degree, noise = struct.unpack_from("<BII", blob, off)
        assert tag == 1
        out.append((degree, noise))
        off += 9 + 2049 * 8
    assert off == len(blob)
    return out


# ------------------------------------------------------------------ word for word
# 1: t = 0, every mask word but the first subtracted; 2, 3: odd and even t; 128: a 256-bit operand
@pytest.mark.parametrize("blocks", [1, 2, 3, 128])
def test_value_equals_host(env, blocks):
    ck, pk, _, _ = env
    v = _value(2 * blocks)
    x = FheUint.try_encrypt(v, ck, bits=2 * blocks)
    before = x.export()
    y = x.re_randomize(SEED_A)
    got = y.export()
    assert np.array_equal(got, rerandomize_host(pk, SEED_A, before))
    assert not np.array_equal(got[:, :N], before[:, :N])
    assert np.array_equal(x.export(), before)  # out of place: the source keeps every word
    assert y.decrypt(ck) == v and x.decrypt(ck) == v
    assert _block_meta(y) == _block_meta(x)


# 2049 and 4097 blocks cross a chunk boundary (t = 2047: nothing subtracted; the second and third chunks' R and
# noise positions); a radix integer stops at 2048 blocks, so the rows go through the device hook
@pytest.mark.parametrize("blocks", [2049, 4097])
def test_rows_across_chunks_equal_host(env, blocks):
    ck, pk, _, _ = env
    rows = ck.encrypt_blocks(np.arange(blocks) % 4)
    got, want = rerandomize_rows(SEED_B, rows), rerandomize_host(pk, SEED_B, rows)
    for t in (0, 1, 2046, 2047, 2048, blocks - 1):
        assert np.array_equal(got[t], want[t]), t
    assert np.array_equal(got, want)


def test_recycled_slots_keep_no_stale_word(env):
    ck, pk, _, _ = env
    x, z = FheUint.try_encrypt(_value(64), ck, bits=64), FheUint.try_encrypt(_value(64, 1), ck, bits=64)
    y = x.re_randomize(SEED_A)
    assert np.array_equal(y.export(), rerandomize_host(pk, SEED_A, x.export()))
    del y  # its slots go back to the pool and are handed out again
    w = z.re_randomize(SEED_B)
    assert np.array_equal(w.export(), rerandomize_host(pk, SEED_B, z.export()))


def test_behind_a_pending_graph(env):
    ck, pk, _, _ = env
    va, vb = 0x9E3779B9, 0x7F4A7C15
    a, b = FheUint32.try_encrypt(va, ck), FheUint32.try_encrypt(vb, ck)
    s = a + b  # recorded, not launched
    r = s.re_randomize(SEED_A)
    assert np.array_equal(r.export(), rerandomize_host(pk, SEED_A, s.export()))
    assert r.decrypt(ck) == (va + vb) % 2**32
    assert _block_meta(r) == _block_meta(s)


def test_trivial_operand_becomes_a_ciphertext(env):
    ck, pk, _, _ = env
    v = 0xC0FFEE11
    t = FheUint32.encrypt_trivial(v)
    rows = t.export()
    assert not rows[:, :N].any()
    r = t.re_randomize(SEED_B)
    got = r.export()
    assert np.array_equal(got, rerandomize_host(pk, SEED_B, rows))
    assert got[:, :N].any(axis=1).all()
    assert r.decrypt(ck) == v
    assert all(d == 3 for d, _ in _block_meta(r))  # tag 1 everywhere: no block is trivial any more
    assert (r + 5).decrypt(ck) == v + 5


def test_biguint_digits_in_order(env):
    ck, pk, _, _ = env
    v = _value(96, 2) | 1 << 95
    x = BigUintFHE.new(v, ck)
    y = x.re_randomize(SEED_A)
    rows = np.concatenate([d.export() for d in x.digits])
    assert np.array_equal(np.concatenate([d.export() for d in y.digits]), rerandomize_host(pk, SEED_A, rows))
    assert len(y) == 3 and y.to_biguint(ck) == v
    empty = BigUintFHE.from_encrypted_digits([])
    assert len(empty) == 0 and len(empty.re_randomize(SEED_A)) == 0


def test_default_seed_is_entropy(env):
    ck, _, _, _ = env
    x = FheUint32.try_encrypt(77, ck)
    a, b = x.re_randomize(), x.re_randomize()
    assert not np.array_equal(a.export()[:, :N], b.export()[:, :N])
    assert a.decrypt(ck) == b.decrypt(ck) == 77
    with pytest.raises(ValueError):
        x.re_randomize(b"short")


# ------------------------------------------------------------------ parameters and end to end
def test_multi_bit_parameters(env):
    from fhe_sign import integer
    keyed = integer._ctx()
    ck, sk = generate_keys(multi_bit_params(), seed=0x5EED14)
    pk = CompactPublicKey.new(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    try:
        x = FheUint32.try_encrypt(0xC0FFEE11, ck)
        y = x.re_randomize(SEED_A)
        assert np.array_equal(y.export(), rerandomize_host(pk, SEED_A, x.export()))
        assert (y + 5).decrypt(ck) == 0xC0FFEE16
        del x, y
    finally:
        set_server_key(keyed)
        ctx.close()


def test_rerandomized_operands_compute(env):
    ck, _, _, _ = env
    va, vb = 0xDEADBEEF, 0x0BADF00D
    a, b = FheUint32.try_encrypt(va, ck).re_randomize(), FheUint32.try_encrypt(vb, ck).re_randomize()
    assert isinstance(a, FheUint32)
    assert (a + b).decrypt(ck) == (va + vb) % 2**32
    assert (a * b).decrypt(ck) == (va * vb) % 2**32
    assert (a // 5).decrypt(ck) == va // 5


def test_expanded_packed_list_then_rerandomized(env):
    ck, pk, _, _ = env
    v = _value(64) | 3 << 62
    (x,) = CompactCiphertextList.builder(pk).push(v, bits=64).build_packed().expand()
    y = x.re_randomize(SEED_B)
    assert y.decrypt(ck) == v
    meta = _block_meta(y)
    assert all(d <= 3 and n <= 1 for d, n in meta), meta
    assert (y + 1).decrypt(ck) == (v + 1) % 2**64


def test_sign_with_a_rerandomized_private_key(env):
    ck, _, _, _ = env
    rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
    row = next(r for r in rows if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    d_fhe = BigUintFHE.new(d, ck).re_randomize(rerandomization_seed(b"bip340 vector", msg))
    sig = Schnorr().sign_fhe_with_k0(msg, compute_nonce(d, msg, aux), d, d_fhe, ck, COMPAT)
    assert sig.hex().upper() == row["signature"].upper()


# ------------------------------------------------------------------ refusals
def test_keys_and_refusals(env):
    from fhe_sign import integer
    ck, pk, _, sk = env
    keyed = integer._ctx()
    ctx = Context(0)
    set_server_key(ctx)
    try:
        with pytest.raises(FheError) as e:  # no server key: the public key has nothing to belong to
            ctx.set_public_key(pk)
        assert e.value.code == -3
        ctx.set_server_key(sk)
        x = FheUint32.try_encrypt(9, ck)
        with pytest.raises(FheError, match="no public key installed") as e:
            x.re_randomize(SEED_A)
        assert e.value.code == -3  # FHE_ERR_NO_KEY
        with pytest.raises(FheError) as e:
            BigUintFHE.new(9, ck).re_randomize(SEED_A)
        assert e.value.code == -3
        # a public key of other parameters: refused by name, nothing installed
        other = CompactPublicKey.new(generate_keys(multi_bit_params(), seed=0x5EED15)[0])
        with pytest.raises(FheError, match="grouping") as e:
            ctx.set_public_key(other)
        assert e.value.code == -1
        with pytest.raises(FheError, match="no public key installed"):
            x.re_randomize(SEED_A)
        ctx.set_public_key(pk)
        assert x.re_randomize(SEED_A).decrypt(ck) == 9
        ctx.set_public_key(pk)  # again: replaces
        assert x.re_randomize(SEED_A).decrypt(ck) == 9
        # re-keying the context drops it
        ctx.set_server_key(sk)
        x = FheUint32.try_encrypt(9, ck)
        with pytest.raises(FheError, match="no public key installed") as e:
            x.re_randomize(SEED_A)
        assert e.value.code == -3
        del x
    finally:
        set_server_key(keyed)
        ctx.close()


# ------------------------------------------------------------------ two ranks
def test_world2_rerandomize_gloo_transport():
    """TWO processes on one GPU through the test transport (tests/rerandomize_gloo_rank.py): both re-randomize
    the broadcast operand under the same derived seed and run the compat 256-bit product on it, levels split
    over the ranks.  The re-randomized words and the product's are equal on both ranks and equal to the unsplit
    run's; the source is untouched; a NULL seed is refused while the communicator is attached."""
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs, world = [], 2
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(ROOT, "tests", "rerandomize_gloo_rank.py")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    res = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=180)  # every process its own limit
            assert p.returncode == 0, e[-3000:]
            res.append(json.loads(o.strip().splitlines()[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    res = sorted(res, key=lambda x: x["rank"])
    print(*(json.dumps(r) for r in res), sep="\n")
    for r in res:
        assert r["null_refused"], r
        assert r["compat_ok"] and r["split_levels"] > 0, r
        assert r["rerand_sha"] == res[0]["unsplit_rerand_sha"] and r["rerand_sha"] != r["source_sha"], r
        assert r["compat_sha"] == res[0]["unsplit_sha"], r
    assert res[0]["unsplit_ok"]
