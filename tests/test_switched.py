"""Modulus-switched stored ciphertexts on the CPU (include/fhe_rocm.h): the host definitions --
fhe_switched_pack_host / _unpack_host, fhe_switched_compress_host, fhe_switched_decrypt, the wire kind -- and the
re-keying key (generation, stream accounting, expansion, wire) against tests/switched_ref.py, which is built from the
restatements the suite already pins.  No GPU.

Decode checks compare against the restatement on fixed seeds, not against a probability: at these dimensions the
restatement decodes every block of these inputs (asserted first, so a miss there names the test's inputs and not
the product)."""
import struct

import numpy as np
import pytest

import compress_ref as R
import seeded_key_ref as K
import switched_ref as S
from fhe_sign import (CompactPublicKey, FheError, RekeyKey, SwitchedCiphertextList, generate_keys, switched_pack_host,
                      switched_row_bytes, switched_unpack_host)
from fhe_sign.core import MS_PAD_WORD, SWITCHED_GAP_BYTE
from lwe_dims import CLASSIC, MULTIBIT, product_params

SEED = 0x5317C4ED
RADIX, BIGUINT = S.RADIX, S.BIGUINT
MODES = ("standard", "centered")
KEY_SETS = [(15, CLASSIC), (16, MULTIBIT), (256, CLASSIC)]


def strides(n):
    return (n + 1, S.ws_stride(n), S.ws_stride(n) + 5)


# ------------------------------------------------------------------ pack / unpack
def test_edge_words_round_as_stated():
    v = S.values(S.edge_words()[None, :], len(S.edge_words()) - 1)[0].reshape(len(S.EDGE_TOPS), len(S.EDGE_LOWS))
    for i, t in enumerate(S.EDGE_TOPS):
        assert list(v[i]) == [t, t, (t + 1) % 4096, (t + 1) % 4096, (t + 1) % 4096]
    assert v[3, 2] == 0  # 0xFFF over 2^51 wraps


@pytest.mark.parametrize("n", S.N_LIST)
def test_pack_host_equals_restatement(n):
    rows = S.edge_rows(n, 5)
    ref = S.pack_rows(rows, n)
    rb = S.row_bytes(n)
    assert rb == switched_row_bytes(n) == len(ref[0])
    for stride in strides(n):
        wide = np.full((5, stride), 0xFFFFFFFFFFFFFFFF, np.uint64)  # a reader of the padding would pack ones
        wide[:, :n + 1] = rows
        for bs in (rb, rb + 3):
            got = switched_pack_host(wide, n, bs)
            assert got.shape == (5, bs)
            for b in range(5):
                assert got[b, :rb].tobytes() == ref[b], f"n {n}, stride {stride}, row {b}"
            assert (got[:, rb:] == SWITCHED_GAP_BYTE).all(), "bytes between the rows were written"
    if (n + 1) % 2:
        assert all(r[-1] >> 4 == 0 for r in ref), "pad nibble"


@pytest.mark.parametrize("n", S.N_LIST)
def test_unpack_host_equals_restatement(n):
    packed = S.pack_rows(S.edge_rows(n, 5), n)
    rb = S.row_bytes(n)
    for bs in (rb, rb + 3):
        buf = np.full((5, bs), 0xFF, np.uint8)  # set bits behind a row: not the row's
        for b in range(5):
            buf[b, :rb] = np.frombuffer(packed[b], np.uint8)
        for stride in strides(n):
            got = switched_unpack_host(buf, n, stride)
            assert np.array_equal(got, S.unpack_rows(packed, n, stride)), f"n {n}, stride {stride}, byte stride {bs}"
            assert (got[:, n + 1:] == np.uint64(MS_PAD_WORD)).all()
            assert not (got[:, :n + 1] & np.uint64((1 << 52) - 1)).any(), "a stored word has a residue"
    # and back: packing the unpacked rows gives the bytes again
    again = switched_pack_host(S.unpack_rows(packed, n), n)
    assert [again[b].tobytes() for b in range(5)] == packed


def test_pack_refuses_bad_shapes():
    rows = np.zeros((1, 17), np.uint64)
    for n, bs in ((0, 8), (2049, 4000), (17, 27), (16, S.row_bytes(16) - 1)):
        with pytest.raises(FheError):
            switched_pack_host(rows if n != 2049 else np.zeros((1, 2056), np.uint64), n, bs)
    with pytest.raises(FheError):
        switched_unpack_host(np.zeros((1, 26), np.uint8), 16, 16)


# ------------------------------------------------------------------ compress, decrypt
_keys = {}


def keys(n, g):
    if (n, g) not in _keys:
        ck, sk = generate_keys(product_params(n, g), seed=SEED + n)
        _keys[(n, g)] = (ck, sk, sk.export()[0], ck.export()[0])
    return _keys[(n, g)]


def block_values(B, top):
    """values below `top`, every one of them present when B allows"""
    return [(5 * i + 3) % top for i in range(B)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,g", KEY_SETS, ids=lambda v: str(v))
def test_compress_host_equals_restatement(n, g, mode):
    ck, sk, ksk, _ = keys(n, g)
    vals = block_values(16, 16)
    cts = ck.encrypt_blocks(vals)
    cts[3, :] = np.uint64((1 << 64) - 1)  # all ones: every digit rounds up and wraps
    degrees = [max(v, 3) for v in vals]
    lst = SwitchedCiphertextList.compress_host(sk, cts, degrees, RADIX, 32, mode)
    assert (lst.nblocks, lst.bits, lst.params.lwe_dimension, lst.params.grouping) == (16, 32, n, g)
    ref = S.compress(ksk, n, cts, mode == "centered")
    blob = lst.serialize()
    assert blob == S.wire(S.main_bytes(n, g), RADIX, 32, degrees, ref)
    assert len(blob) == S.wire_len(n, 16)


def test_modes_differ():
    ck, sk, ksk, _ = keys(256, CLASSIC)
    cts = ck.encrypt_blocks(block_values(16, 4))
    a, b = (SwitchedCiphertextList.compress_host(sk, cts, 3, RADIX, 32, m).serialize() for m in MODES)
    assert a != b


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,g", KEY_SETS, ids=lambda v: str(v))
def test_decrypt_radix_with_carries(n, g, mode):
    ck, sk, ksk, lwe_sk = keys(n, g)
    vals = block_values(24, 16)  # degrees above 3: the blocks carry into their neighbours
    cts = ck.encrypt_blocks(vals)
    want = sum(v << (2 * k) for k, v in enumerate(vals)) % (1 << 48)
    ref_vals, _ = S.decrypt_values(S.compress(ksk, n, cts, mode == "centered"), n, lwe_sk)
    assert ref_vals == vals, "the restatement does not decode these inputs"
    lst = SwitchedCiphertextList.compress_host(sk, cts, 15, RADIX, 48, mode)
    assert lst.decrypt(ck) == want == S.assemble(ref_vals, RADIX, 48)
    assert SwitchedCiphertextList.deserialize(lst.serialize()).decrypt(ck) == want


@pytest.mark.parametrize("n,g", KEY_SETS, ids=lambda v: str(v))
def test_decrypt_biguint_with_carries(n, g):
    ck, sk, ksk, lwe_sk = keys(n, g)
    vals = block_values(48, 16)  # three limbs; a limb's carries stay inside it
    cts = ck.encrypt_blocks(vals)
    want = sum((sum(v << (2 * k) for k, v in enumerate(vals[i:i + 16])) % (1 << 32)) << (2 * i) for i in range(0, 48, 16))
    ref_vals, _ = S.decrypt_values(S.compress(ksk, n, cts, False), n, lwe_sk)
    assert ref_vals == vals, "the restatement does not decode these inputs"
    lst = SwitchedCiphertextList.compress_host(sk, cts, 15, BIGUINT, 3)
    assert lst.bits == 96
    assert lst.decrypt(ck) == want == S.assemble(ref_vals, BIGUINT, 96)


def test_decrypt_refuses_another_key():
    ck, sk, _, _ = keys(15, CLASSIC)
    other, _, _, _ = keys(256, CLASSIC)
    lst = SwitchedCiphertextList.compress_host(sk, ck.encrypt_blocks([1, 2]), 3, RADIX, 4)
    with pytest.raises(FheError, match="lwe_dimension"):
        lst.decrypt(other)


def test_compress_host_refusals():
    ck, sk, _, _ = keys(15, CLASSIC)
    cts = ck.encrypt_blocks([1, 2])
    for args in ((cts, 3, RADIX, 6), (cts, 16, RADIX, 4), (cts, 3, BIGUINT, 1), (cts, 3, 2, 4)):
        with pytest.raises(FheError):
            SwitchedCiphertextList.compress_host(sk, *args)
    with pytest.raises(FheError):
        SwitchedCiphertextList.compress_host(sk, cts, 3, RADIX, 4, "rounded")


# ------------------------------------------------------------------ the wire
def test_default_sizes():
    """the issue's figures: 1,253 bytes per block at n = 834, 160,384 for the 128 rows of a 256-bit value"""
    assert S.row_bytes(834) == switched_row_bytes(834) == 1253
    assert 128 * S.row_bytes(834) == 160384
    assert S.wire_len(834, 128) == 80 + 128 + 160384


@pytest.mark.parametrize("n", (15, 16))
def test_wire_round_trip_and_refusals(n):
    """n = 15: n + 1 even, no pad; n = 16: a pad nibble in every row"""
    rng = np.random.default_rng(n)
    rows = S.pack_rows(rng.integers(0, 1 << 64, (4, n + 1), dtype=np.uint64), n)
    degrees = [0, 3, 7, 15]
    main = S.main_bytes(n)
    blob = S.wire(main, RADIX, 8, degrees, rows)
    lst = SwitchedCiphertextList.deserialize(blob)
    assert lst.serialize() == blob and (lst.nblocks, lst.bits) == (4, 8)
    assert S.parse_list(n, blob) == (RADIX, 8, degrees, rows)
    big = S.wire(main, BIGUINT, 1, [3] * 16, rows * 4)
    assert SwitchedCiphertextList.deserialize(big).bits == 32

    def refused(b, what):
        with pytest.raises(FheError, match=what):
            SwitchedCiphertextList.deserialize(b)

    for cut in (0, 31, 40, S.HEADER - 1, S.HEADER + 2, len(blob) - 1):
        refused(blob[:cut], None)
    refused(blob + b"\0", "length")
    refused(K.frame(S.KIND_LIST, blob[32:-1]), "payload length")  # a well-formed frame around a short payload
    refused(K.frame(S.KIND_LIST, blob[32:] + b"\0"), "payload length")
    refused(blob[:-1] + bytes([blob[-1] ^ 1]), "checksum")
    refused(S.wire(main, RADIX, 8, [0, 3, 16, 15], rows), "degree")
    refused(S.wire(main, RADIX, 10, degrees, rows), "form / count")
    refused(S.wire(main, BIGUINT, 1, degrees, rows), "form / count")
    refused(S.wire(main, 2, 8, degrees, rows), "form")
    refused(K.frame(9, blob[32:]), "kind")
    for bad_n in (0, 2049):
        refused(S.wire(struct.pack("<I", bad_n) + main[4:], RADIX, 8, degrees, rows), "unsupported parameters")
    refused(S.wire(main[:32] + struct.pack("<I", 3), RADIX, 8, degrees, rows), "unsupported parameters")  # grouping 3
    if (n + 1) % 2:
        for b in range(4):
            bad = list(rows)
            bad[b] = bad[b][:-1] + bytes([bad[b][-1] | 0x10])
            refused(S.wire(main, RADIX, 8, degrees, bad), "pad")
    else:
        assert S.row_bytes(n) * 8 == 12 * (n + 1)


# ------------------------------------------------------------------ the re-keying key
RK_SEED = bytes(range(7, 39))
ENC_SEED, ENC_STREAM = 0xE5C0DE, 77
REKEY_SETS = [((16, CLASSIC), (15, CLASSIC)), ((256, CLASSIC), (255, CLASSIC)), ((256, CLASSIC), (256, MULTIBIT))]


def fresh_pair(src, dst):
    a, _ = generate_keys(product_params(*src), seed=SEED + 1)
    b, _ = generate_keys(product_params(*dst), seed=SEED + 2)
    b.seed_encryption(ENC_SEED, ENC_STREAM)
    return a, b


def test_rekey_stream_accounting():
    """the destination key's encryption stream advances by exactly 2048 * 5 words, the source's by none: the same
    as five public keys (2048 words each) drawn from a twin of the destination"""
    a, b = fresh_pair((16, CLASSIC), (15, CLASSIC))
    _, twin = fresh_pair((16, CLASSIC), (15, CLASSIC))
    before = a.serialize()
    assert b.serialize() == twin.serialize()
    RekeyKey.new(a, b, RK_SEED)
    assert a.serialize() == before
    assert b.serialize() != twin.serialize()
    for i in range(5):
        CompactPublicKey.new(twin, bytes([i]) * 32)
    assert b.serialize() == twin.serialize()


@pytest.mark.parametrize("src,dst", REKEY_SETS, ids=lambda v: str(v))
def test_rekey_expand_and_switch(src, dst):
    a, b = fresh_pair(src, dst)
    n = dst[0]
    key = RekeyKey.new(a, b, RK_SEED)
    assert (key.params.lwe_dimension, key.params.grouping) == dst
    noise = R.enc_stream(ENC_SEED, ENC_STREAM, 0, S.KSK_ROWS)
    s_dst, S_src = b.export()[0], a.export()[1]
    ref = S.rekey_ksk(RK_SEED, noise, s_dst, S_src)
    ksk = key.expand_host()
    assert np.array_equal(ksk.reshape(S.KSK_ROWS, n + 1), ref)
    # the wire: the destination's params, the seed, the bodies
    blob = key.serialize()
    assert blob == S.rekey_wire(S.main_bytes(*dst), RK_SEED, ref[:, n]) and len(blob) == 100 + 8 * S.KSK_ROWS
    assert np.array_equal(RekeyKey.deserialize(blob).expand_host(), ksk)
    # blocks under A, keyswitched with it, are rows under B's small key
    vals = [(5 * i + 3) % 16 for i in range(24)]
    cts = a.encrypt_blocks(vals)
    for centered in (False, True):
        rows = S.compress(ksk, n, cts, centered)
        assert S.decrypt_values(rows, n, s_dst)[0] == vals, "the restatement does not decode these inputs"
        lst = SwitchedCiphertextList.compress_host(key, cts, 15, RADIX, 48, MODES[centered])
        assert lst.serialize() == S.wire(S.main_bytes(*dst), RADIX, 48, [15] * 24, rows)
        assert lst.decrypt(b) == sum(v << (2 * k) for k, v in enumerate(vals)) % (1 << 48)
        with pytest.raises(FheError):
            lst.decrypt(a)


def test_rekey_refusals():
    a, b = fresh_pair((16, CLASSIC), (15, CLASSIC))
    # the shared fields a key generation lets differ (ks_base_log, ks_level and pbs_base_log are fixed by the kernels)
    for field, value in (("message_modulus", 2), ("carry_modulus", 2), ("glwe_noise_log2", 16)):
        p = product_params(15)
        setattr(p, field, value)
        other, _ = generate_keys(p, seed=SEED + 3)
        with pytest.raises(FheError, match=field):
            RekeyKey.new(a, other, RK_SEED)
        with pytest.raises(FheError, match=field):
            RekeyKey.new(other, b, RK_SEED)
    # the destination's own fields may differ
    for field, value in (("lwe_noise_log2", 44), ("lwe_dimension", 14)):
        p = product_params(15)
        setattr(p, field, value)
        other, _ = generate_keys(p, seed=SEED + 3)
        assert getattr(RekeyKey.new(a, other, RK_SEED).params, field) == value
    with pytest.raises(ValueError):
        RekeyKey.new(a, b, b"short")
    blob = RekeyKey.new(a, b, RK_SEED).serialize()
    for bad in (blob[:-8], blob[:50], blob[:-1] + bytes([blob[-1] ^ 1]), K.frame(S.KIND_REKEY, blob[32:] + b"\0" * 8),
                K.frame(S.KIND_LIST, blob[32:]), K.frame(S.KIND_REKEY, struct.pack("<I", 0) + blob[36:])):
        with pytest.raises(FheError):
            RekeyKey.deserialize(bad)
