"""The integer restatement tests/ks_ref.py against the oracle's keyswitch, word for word (CPU), and a
record of how much of a keyswitch word a bootstrap can see -- the reason tests/test_keyswitch_gpu.py
compares 64-bit words."""
import numpy as np
import pytest

import ks_ref
import oracle
from fhe_sign import _lib, generate_keys

SEED = 0xC0FFEE


@pytest.fixture(scope="module")
def keys():
    _, sk = generate_keys(seed=SEED)
    ok = oracle.OracleKeys(SEED)
    ksk, _ = sk.export()
    return ok, ksk, int(sk.params.lwe_dimension)


def _encryptions(ok, count, seed):
    r = ok.rng(seed)
    return np.stack([ok.encrypt(r, i % 16) for i in range(count)])


def test_product_ksk_is_the_oracles(keys):
    ok, ksk, n = keys
    assert n == ok.params.n and np.array_equal(ksk, ok.ksk)


def test_digits_closed_form_equals_the_carry_loop():
    """ks_ref.digits against the loop every implementation runs (oracle fho_keyswitch, k_ks_digits,
    k_keyswitch) on the edge rows and random words"""
    words = np.concatenate([ks_ref.edge_rows()[:, :2048].ravel(),
                            np.random.default_rng(1).integers(0, 1 << 64, 4096, dtype=np.uint64)])
    got = ks_ref.digits(words.reshape(-1, 2048))
    for a, d in zip(words.tolist(), got.reshape(-1, 5).tolist()):
        v = (((a >> 48) + 1) >> 1) & 0x7FFF
        ref = [0] * 5
        for l in range(4, -1, -1):
            dig = v & 7
            v >>= 3
            if dig >= 4:
                dig -= 8
                v += 1
            ref[l] = dig
        assert d == ref, hex(a)
    assert got.min() == -4 and got.max() == 3


def test_restatement_equals_oracle(keys):
    """keyswitch_np == oracle.keyswitch_batch on random encryptions and on the digit-edge rows, and the
    edge rows' closed answers: zero mask -> (0, .., 0, body); all ones -> zero digits"""
    ok, ksk, n = keys
    cts = np.concatenate([_encryptions(ok, 4, 4242), ks_ref.edge_rows()])
    ref = ok.keyswitch_batch(cts)
    got = ks_ref.keyswitch_np(ksk, n, cts)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{len(bad)} words differ, first (ciphertext, word) {bad[0]}"
    for row in (2, 3):
        e = ks_ref.edge_rows()[row]
        assert not ks_ref.digits(e).any()
        assert not ref[4 + row][:n].any() and ref[4 + row][n] == e[2048]
    assert np.array_equal(got[0], ks_ref.keyswitch_np(ksk, n, cts[0]))  # one row or a batch


def test_byte_planes_recombine(keys):
    _, ksk, _ = keys
    planes = ks_ref.byte_planes(ksk[: 5 * 835 * 16])
    assert planes.min() == -128 and planes.max() == 127
    acc = np.zeros(planes.shape[1], np.uint64)
    for b in range(8):
        acc += planes[b].astype(np.uint64) << np.uint64(8 * b)
    assert np.array_equal(acc, ksk[: 5 * 835 * 16])


def test_lincomb_np_wraps():
    blocks = np.arange(3 * 2049, dtype=np.uint64).reshape(3, 2049) * np.uint64(0x9E3779B97F4A7C15)
    terms = [(0, -7), (2, (1 << 33) + 1), (0, 4), (1, -(1 << 40) - 3)]
    got = ks_ref.lincomb_np(blocks, terms, (1 << 64) - 1)
    ref = [sum(c * int(blocks[s][j]) for s, c in terms) % (1 << 64) for j in (0, 1, 2047, 2048)]
    ref[3] = (ref[3] - 1) % (1 << 64)
    assert [int(got[j]) for j in (0, 1, 2047, 2048)] == ref


def test_bootstraps_cannot_see_the_low_byte_planes(keys):
    """Why tests/test_keyswitch_gpu.py compares 64-bit keyswitch words and not bootstrap outputs: the
    blind rotation reads a small LWE word only through the modulus switch (bits 51 and up), so a
    keyswitch that loses a low byte plane of the matrix-core contraction (ks_mfma.hip: 8 int8 GEMMs,
    |S_b| < 2^23) feeds every bootstrap the same values.  Here the plane-b partial sum S_b << 8 b is
    added back to the oracle's keyswitch of 8 ciphertexts -- the output of a kernel that dropped
    plane b: for b = 0 and 1 (error < 2^31 against a rounding step of 2^52) no modulus-switched value
    changes, for b = 5 (error ~2^56) most do."""
    ok, ksk, n = keys
    cts = _encryptions(ok, 8, 99)
    ref = ok.keyswitch_batch(cts)
    ms = ks_ref.modswitch(ref)
    planes = ks_ref.byte_planes(ksk)
    with np.errstate(over="ignore"):
        changed = {b: int(np.count_nonzero(ks_ref.modswitch(ref + ks_ref.plane_sum(planes[b], b, n, cts)) != ms))
                   for b in (0, 1, 5)}
        full = sum(ks_ref.plane_sum(planes[b], b, n, cts[0]) for b in range(8))
        full[n] -= cts[0, 2048]
        assert np.array_equal(np.uint64(0) - full, ref[0])  # the eight planes together are the keyswitch
    print(f"\nmodulus-switched values changed of {ms.size}: {changed}")
    assert changed[0] == 0 and changed[1] == 0
    assert changed[5] > ms.size // 2


def test_new_entries_refuse_a_null_context():
    """argument validation that needs no GPU (the rest needs a context: test_keyswitch_gpu.py)"""
    lib = _lib.load()
    assert lib.fhe_keyswitch_batch(None, None, 0, None) == -1
    assert lib.fhe_pbs_lincomb_batch(None, None, 0, None, None, None, None, None, 0, None, None) == -1
