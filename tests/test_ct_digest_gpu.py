"""Ciphertext digests on the GPU (csrc/ct_digest.hip k_ct_digest through Engine::digest) and the seeds bound to
them: the kernel against fhe_ct_digest_host, which tests/test_ct_digest.py pins byte for byte to hashlib
(tests/ct_digest_ref.py); value digests, context seeds and the re-randomization they feed against the reference;
the signer that re-randomizes privkey_fhe itself.  Every comparison is exact."""
import csv
import json
import os
import struct

import numpy as np
import pytest

import ct_digest_ref as ref
from conftest import ROOT
from fhe_sign import (COMPAT, BigUintFHE, CompactPublicKey, Context, FheUint, FheUint32, ReRandomizationContext, Schnorr,
                      compute_nonce, ct_digest_host, ct_digest_rows, generate_keys, multi_bit_params, re_randomize_bound,
                      rerandomize_host, set_server_key)
from fhe_sign._lib import FheError

pytestmark = pytest.mark.gpu
ROW = 2049
SIZES = [1, 2, 63, 64, 65, 128, 2049]  # 2049 rows: more waves than the chip holds at once


@pytest.fixture(scope="module")
def env():
    ck, sk = generate_keys(seed=0x5EED16)
    pk = CompactPublicKey.new(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    yield ck, pk, ctx, sk
    set_server_key(None)
    ctx.close()


@pytest.fixture(scope="module")
def pool(env):
    """2049 rows, computed once: encrypted rows with the hand-built and bit-flip rows (ct_digest_ref.hand_rows)
    at the odd positions 1, 3, .. 19, so that every size from 2 on holds both; and their host digests"""
    ck = env[0]
    rows = ck.encrypt_blocks(np.arange(max(SIZES)) % 4)
    hand = ref.hand_rows()
    rows[1:2 * len(hand):2] = hand
    rows.setflags(write=False)
    want = ct_digest_host(rows)
    assert np.array_equal(want[1:2 * len(hand):2], ref.rows_digest(hand))
    assert bytes(want[1]).hex() == ref.ZERO_ROW_DIGEST and bytes(want[3]).hex() == ref.RAMP_ROW_DIGEST
    want.setflags(write=False)
    return rows, want


# ------------------------------------------------------------------ the kernel, byte for byte
@pytest.mark.parametrize("n", SIZES)
def test_rows_equal_host(env, pool, n):
    rows, want = pool
    got = ct_digest_rows(rows[:n])
    assert got.shape == (n, 32)
    assert np.array_equal(got, want[:n])


# ------------------------------------------------------------------ value digests
def _parse_blocks(blob, off):
    """one put_blocks record of a serialized value: (bits, [(tag, degree or value, noise)], next offset)"""
    bits, nb = struct.unpack_from("<II", blob, off)
    off += 8
    out = []
    for _ in range(nb):
        tag = blob[off]
        if tag == 0:
            (value,) = struct.unpack_from("<I", blob, off + 1)
            out.append((0, value, 0))
            off += 5
        else:
            assert tag == 1
            degree, noise = struct.unpack_from("<II", blob, off + 1)
            out.append((1, degree, noise))
            off += 9 + ROW * 8
    return bits, out, off


HEADER = 32 + 36  # the frame, then the parameters


def _ref_digest(x):
    """D(x) from the reference: x.export() for the rows, x.serialize() for the per-block fields"""
    blob = x.serialize()
    if isinstance(x, BigUintFHE):
        (nd,) = struct.unpack_from("<I", blob, HEADER)
        off, meta = HEADER + 4, []
        for _ in range(nd):
            bits, m, off = _parse_blocks(blob, off)
            assert bits == 32 and len(m) == 16
            meta += m
        kind, bits = 1, 32 * nd
        rows = np.concatenate([d.export() for d in x.digits]) if nd else np.zeros((0, ROW), np.uint64)
    else:
        bits, meta, off = _parse_blocks(blob, HEADER)
        kind, rows = 0, x.export()
        assert bits == x.bits
    assert off == len(blob) and len(meta) == rows.shape[0]
    return ref.value_digest(kind, bits, [(t, d, s, ref.row_digest(r)) for (t, d, s), r in zip(meta, rows)]), meta


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits)


@pytest.mark.parametrize("blocks", [1, 2, 3, 128])
def test_value_digest_equals_reference(env, blocks):
    ck = env[0]
    v = _value(2 * blocks)
    x = FheUint.try_encrypt(v, ck, bits=2 * blocks)
    before = x.export()
    want, meta = _ref_digest(x)
    assert all(t == 1 for t, _, _ in meta)
    assert x.digest() == want
    assert x.digest() == want  # deterministic
    assert np.array_equal(x.export(), before) and x.decrypt(ck) == v  # the blocks are untouched


def test_biguint_digest(env):
    ck = env[0]
    x = BigUintFHE.new(_value(256, 3) | 1 << 255, ck)
    assert len(x) == 8
    want, meta = _ref_digest(x)
    assert len(meta) == 128
    assert x.digest() == want
    assert x.to_radix(256).digest() != want  # the same blocks as a radix integer: another kind
    empty = BigUintFHE.from_encrypted_digits([])
    assert empty.digest() == ref.value_digest(1, 0, [])


def test_trivial_operand(env):
    t = FheUint32.encrypt_trivial(0xC0FFEE11)
    rows = t.export()
    assert not rows[:, :2048].any() and rows[:, 2048].any()
    want, meta = _ref_digest(t)
    assert all(tag == 0 for tag, _, _ in meta)
    assert t.digest() == want
    assert t.digest() != FheUint32.encrypt_trivial(0xC0FFEE12).digest()


def test_trivial_and_real_blocks_mixed(env):
    ck = env[0]
    x = BigUintFHE.new(_value(64, 4) | 1 << 63, ck).to_radix(96)  # 32 ciphertexts, then 16 trivial zeros
    want, meta = _ref_digest(x)
    assert [t for t, _, _ in meta] == [1] * 32 + [0] * 16
    assert x.digest() == want


def test_behind_a_pending_graph(env):
    ck = env[0]
    a, b = FheUint32.try_encrypt(0x9E3779B9, ck), FheUint32.try_encrypt(0x7F4A7C15, ck)
    s = a + b  # recorded, not launched
    got = s.digest()
    assert got == _ref_digest(s)[0]
    assert s.decrypt(ck) == (0x9E3779B9 + 0x7F4A7C15) % 2**32


def test_recycled_slots(env):
    ck = env[0]
    x = FheUint.try_encrypt(_value(64), ck, bits=64)
    dx = x.digest()
    assert dx == _ref_digest(x)[0]
    del x  # its slots go back to the pool and are handed out again
    z = FheUint.try_encrypt(_value(64, 1), ck, bits=64)
    dz = z.digest()
    assert dz == _ref_digest(z)[0] and dz != dx


def test_multi_bit_parameters(env):
    from fhe_sign import integer
    keyed = integer._ctx()
    ck, sk = generate_keys(multi_bit_params(), seed=0x5EED17)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    try:
        x = FheUint32.try_encrypt(0xC0FFEE11, ck)
        assert x.digest() == _ref_digest(x)[0]  # no public key installed: a digest needs none
        s = x + 5
        assert s.digest() == _ref_digest(s)[0]
        del x, s
    finally:
        set_server_key(keyed)
        ctx.close()


# ------------------------------------------------------------------ seeds bound to ciphertexts
def test_rerandomize_under_a_context_seed(env):
    ck, pk, _, _ = env
    v = _value(64, 5)
    x = FheUint.try_encrypt(v, ck, bits=64)
    rc = ReRandomizationContext(b"tests/ct-digest").add_bytes(b"request 1").add(x)
    seed_ref = ref.Context(b"tests/ct-digest").add_bytes(b"request 1").add_digest(_ref_digest(x)[0]).seed(0)
    assert rc.seed(0) == seed_ref
    y = x.re_randomize(rc.seed(0))
    assert np.array_equal(y.export(), rerandomize_host(pk, seed_ref, x.export()))
    assert y.decrypt(ck) == v
    with pytest.raises(FheError, match="seed"):
        rc.add(x)
    # re_randomize_bound: one context over all values, value i under seed(i)
    big = BigUintFHE.new(_value(64, 6) | 1 << 63, ck)
    r = ref.Context(b"bound").add_bytes(b"data").add_digest(_ref_digest(x)[0]).add_digest(_ref_digest(big)[0])
    rx, rbig = re_randomize_bound(b"bound", [x, big], b"data")
    assert np.array_equal(rx.export(), rerandomize_host(pk, r.seed(0), x.export()))
    rows = np.concatenate([d.export() for d in big.digits])
    assert np.array_equal(np.concatenate([d.export() for d in rbig.digits]), rerandomize_host(pk, r.seed(1), rows))


def _fnv1a_words(payload: bytes) -> int:
    """serial.cpp's frame checksum: FNV-1a over little-endian 64-bit words, the tail zero-padded"""
    payload += bytes(-len(payload) % 8)
    h = 0xcbf29ce484222325
    for (w,) in struct.iter_unpack("<Q", payload):
        h = ((h ^ w) * 0x100000001b3) % 2**64
    return h


def test_one_flipped_bit_changes_every_seed(env):
    ck = env[0]
    x, y = FheUint.try_encrypt(0x1234, ck, bits=16), FheUint.try_encrypt(0x5678, ck, bits=16)
    blob = bytearray(y.serialize())
    # one bit of a mask word of y's last block; the frame's checksum follows
    blob[len(blob) - 8 * 1000] ^= 0x10
    blob[24:32] = struct.pack("<Q", _fnv1a_words(bytes(blob[32:])))
    y2 = FheUint.deserialize(bytes(blob))
    assert int((y2.export() != y.export()).sum()) == 1

    def seeds(a, b):
        rc = ReRandomizationContext(b"flip").add(a).add(b)
        return [rc.seed(i) for i in range(4)]

    s0, s1 = seeds(x, y), seeds(x, y2)
    assert s0 == seeds(x, y)
    assert all(a != b for a, b in zip(s0, s1)) and len(set(s0 + s1)) == 8
    r = ref.Context(b"flip").add_digest(_ref_digest(x)[0]).add_digest(_ref_digest(y2)[0])
    assert s1 == [r.seed(i) for i in range(4)]


# ------------------------------------------------------------------ the signer
def test_sign_rerandomizes_the_private_key_itself(env):
    ck = env[0]
    rows = csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))
    row = next(r for r in rows if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    d_fhe = BigUintFHE.new(d, ck)
    before = d_fhe.digest()
    s = Schnorr()
    sig = s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT, rerandomize_domain=b"tests/sign")
    assert sig.hex().upper() == row["signature"].upper()
    assert sig == s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT)
    assert d_fhe.digest() == before  # the caller's ciphertext is untouched


def test_no_public_key_is_refused(env):
    from fhe_sign import integer
    ck, _, _, sk = env
    keyed = integer._ctx()
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    try:
        d_fhe = BigUintFHE.new(3, ck)
        with pytest.raises(FheError, match="no public key installed") as e:
            Schnorr().sign_fhe_with_k0(bytes(32), 5, 3, d_fhe, ck, COMPAT, rerandomize_domain=b"tests/sign")
        assert e.value.code == -3  # FHE_ERR_NO_KEY
        with pytest.raises(FheError, match="no public key installed") as e:
            re_randomize_bound(b"dom", [d_fhe])
        assert e.value.code == -3
        assert len(d_fhe.digest()) == 32  # a digest alone needs no public key
        del d_fhe
    finally:
        set_server_key(keyed)
        ctx.close()


# ------------------------------------------------------------------ two ranks
def test_world2_bound_rerandomize_gloo_transport():
    """TWO processes on one GPU through the test transport (tests/ct_digest_gloo_rank.py): both call
    re_randomize_bound on the broadcast operand with no seed passed anywhere.  The re-randomized rows are
    byte-identical on both ranks and to the single-process run, and differ from the source."""
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
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(ROOT, "tests", "ct_digest_gloo_rank.py")],
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
        assert r["digest"] == res[0]["digest"] and r["seed0"] == res[0]["seed0"], r
        assert r["rerand_sha"] == res[0]["unsplit_rerand_sha"] and r["rerand_sha"] != r["source_sha"], r
        assert r["value_ok"], r
    assert res[0]["unsplit_digest"] == res[0]["digest"]
