"""The centered modulus switch on the GPU (k_ms_center, ms_center.hip; FHE_MS_CENTERED), word for word.

  rows      fhe_ms_center_rows == tests/ms_center_ref.py at every n, count and stride of tests/test_ms_center.py
            plus 257 and 1024 rows (more than one workgroup round), the padding marker intact, the extremes
  context   Context.keyswitch in centered mode == center_ref(the same context's rows in standard mode), on both
            keyswitch kernels; back in standard mode the parent's rows
  bootstrap every output word == the oracle's blind rotation + sample extraction of center_ref(oracle.keyswitch):
            latency and throughput kernel, multi-bit, the descriptor path (inline and wide), other dimensions
  radix     FheUint32 add / mul, BIP-340 vector 0, and a fanned-out mul == the unsplit one, all in centered mode
  margin    the modulus-switch error of 4096 keyswitched encryptions under the real small key, both modes:
            sigma within 5 % of sqrt(hw / 12 + 1 / 12) and sqrt(n / 48 + 1 / 12) (sampling error 1.1 %)
"""
import csv
import os

import numpy as np
import pytest

import ks_ref
import ms_center_ref as M
import oracle
from compress_ref import oracle_decompress
from conftest import ROOT
from fhe_sign import (COMPAT, BigUintFHE, Context, FheError, FheUint32, Schnorr, _lib, compute_nonce, generate_keys,
                      ms_stride, multi_bit_params, set_server_key)
from fhe_sign.core import MS_PAD_WORD
from lwe_dims import CLASSIC, MULTIBIT, oracle_params, product_params
from test_keyswitch_gpu import _assert_words, _pool
from test_ms_center import COUNTS, DIMS, _rows, check_extremes, check_layout

pytestmark = pytest.mark.gpu
SEED = 0x3C5C
TABLE = [(m * m + 3) % 16 for m in range(16)]
KS = {"valu": 0, "mfma": 1}

_envs = {}


def _env(n=834, g=CLASSIC):
    """(client key, server key, oracle keys, context in STANDARD mode) of one parameter set, made once"""
    if (n, g) not in _envs:
        if n == 834:
            pp = multi_bit_params() if g == MULTIBIT else None
            op = oracle.multibit_params() if g == MULTIBIT else None
        else:
            pp, op = product_params(n, g), oracle_params(n, g)
        ck, sk = generate_keys(pp, seed=SEED)
        ctx = Context(0)
        ctx.set_server_key(sk)
        _envs[(n, g)] = (ck, sk, oracle.OracleKeys(SEED, op), ctx)
    return _envs[(n, g)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    set_server_key(None)
    for _, _, _, ctx in _envs.values():
        ctx.close()
    _envs.clear()


@pytest.fixture
def centered():
    """switches a context to centered mode for the test and back whatever happens"""
    done = []

    def switch(ctx):
        ctx.set_modulus_switch("centered")
        done.append(ctx)
        return ctx

    yield switch
    for ctx in done:
        ctx.set_modulus_switch("standard")
        ctx.set_ks_kernel(1)
        ctx.set_wide_threshold(256)
        ctx.set_fanout(257, 0)


_fresh = {}


def _fresh37(ok):
    """37 distinct encryptions and their keyswitch by the oracle, once per key set"""
    key = (int(ok.params.n), int(ok.params.grouping))
    if key not in _fresh:
        r = ok.rng(4242)
        cts = np.stack([ok.encrypt(r, i % 16) for i in range(37)])
        small = ok.keyswitch_batch(cts)
        cts.setflags(write=False)
        small.setflags(write=False)
        _fresh[key] = (cts, small)
    return _fresh[key]


# ---------------------------------------------------------------- the kernel over host rows
@pytest.fixture(scope="module")
def bare():
    ctx = Context(0)  # no server key: the rows entry needs none
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", DIMS)
def test_rows_equal_reference(bare, n):
    for count in COUNTS + (257, 1024):
        rows = _rows(n, count)
        ref = M.center_ref(rows)
        for stride in (n + 1, ms_stride(n)):
            got = bare.ms_center_rows(rows, stride)
            assert got.shape == (count, stride)
            check_layout(got, rows, ref, n, f"n {n}, {count} rows, stride {stride}")
            if stride > n + 1:
                assert (got[:, n + 1:] == np.uint64(MS_PAD_WORD)).all()


def test_rows_extremes(bare):
    check_extremes(bare.ms_center_rows)


def test_rows_refuse_bad_shapes(bare):
    lib = _lib.load()
    buf = np.zeros(4100, np.uint64)
    for n, stride in ((0, 8), (2049, 2056), (16, 16)):
        assert lib.fhe_ms_center_rows(bare.handle, _lib.ptr(buf), 1, n, stride) == -1
    assert lib.fhe_ms_center_rows(bare.handle, _lib.ptr(buf), 0, 16, 17) == 0
    assert not buf.any()


def test_mode_setter_and_getter():
    _, _, _, ctx = _env()
    assert ctx.modulus_switch == "standard"  # the default
    lib = _lib.load()
    try:
        ctx.set_modulus_switch("centered")
        assert ctx.modulus_switch == "centered"
        for bad in (2, -1, 7):
            assert lib.fhe_ctx_set_modulus_switch(ctx.handle, bad) == -1  # FHE_ERR_INVALID
            assert b"unknown modulus switch mode" in lib.fhe_last_error()
        with pytest.raises(FheError) as e:
            ctx.set_modulus_switch("central")
        assert e.value.code == -1
        assert ctx.modulus_switch == "centered"  # a refusal changes nothing
    finally:
        ctx.set_modulus_switch("standard")
    assert ctx.modulus_switch == "standard"


# ---------------------------------------------------------------- the context's keyswitch
@pytest.mark.parametrize("ks", list(KS))
def test_keyswitch_centered_rows(centered, ks):
    _, _, ok, ctx = _env()
    base, small = _fresh37(ok)
    n = ok.params.n
    ctx.set_ks_kernel(KS[ks])
    try:
        for count in (1, 37, 300):
            cts = np.resize(base, (count, 2049))
            std = ctx.keyswitch(cts)
            _assert_words(std, np.resize(small, (count, n + 1)), f"{ks}: standard rows of {count}")
            centered(ctx)
            got = ctx.keyswitch(cts)
            _assert_words(got, M.center_ref(std), f"{ks}: centered rows of {count}")
            assert np.array_equal(got[:, :n], std[:, :n]) and (got[:, n] != std[:, n]).any()
            ctx.set_modulus_switch("standard")
            _assert_words(ctx.keyswitch(cts), std, f"{ks}: rows of {count} back in standard mode")
    finally:
        ctx.set_ks_kernel(1)


# ---------------------------------------------------------------- bootstraps
_br37 = {}


def _pbs_case(n, g, count, centered):
    _, _, ok, ctx = _env(n, g)
    base, small = _fresh37(ok)
    if (n, g) not in _br37:  # the oracle's blind rotation + sample extraction of the centered rows
        need = 37 if (n, g) == (834, CLASSIC) else 8
        _br37[(n, g)] = oracle_decompress(ok, M.center_ref(small)[:need], TABLE)
    ref = np.resize(_br37[(n, g)][:min(count, 37)], (count, 2049))
    lid = ctx.lut(TABLE)
    cts = np.resize(base[:min(count, 37)], (count, 2049))
    standard = ctx.pbs(cts, lid)
    centered(ctx)
    got = ctx.pbs(cts, lid)
    _assert_words(got, ref, f"n {n} grouping {g}: {count} centered bootstraps")
    rows = ctx.keyswitch(cts)
    _assert_words(rows, np.resize(M.center_ref(small)[:min(count, 37)], (count, n + 1)), f"n {n} grouping {g}: rows")
    return ok, cts, standard, got


@pytest.mark.parametrize("count", (8, 300), ids=("latency", "throughput"))
def test_pbs_centered_classic(centered, count):
    ok, cts, standard, got = _pbs_case(834, CLASSIC, count, centered)
    assert [ok.decrypt(c) for c in got[:37]] == [TABLE[i % 16] for i in range(min(count, 37))]
    # the centered bootstrap is another ciphertext of the same message
    assert not np.array_equal(got, standard)


def test_pbs_centered_multibit(centered):
    ok, _, _, got = _pbs_case(834, MULTIBIT, 8, centered)
    assert [ok.decrypt(c) for c in got] == [TABLE[i] for i in range(8)]


def test_pbs_lincomb_centered(centered):
    """the descriptor path: one inline item (4 terms) and one wide item (20 terms through the staged table)"""
    _, _, ok, ctx = _env()
    pool = _pool(ok)
    inline = ([(4, -7), (5, 4), (6, 3), (38, -1)], 5 * ok.delta())
    wide = ([((7 * t + 1) % 40, (-1) ** t * (t + 1)) for t in range(20)], (1 << 64) - 1)
    items = [inline, wide]
    comb = np.stack([ks_ref.lincomb_np(pool, t, c) for t, c in items])
    rows_ref = M.center_ref(ok.keyswitch_batch(comb))
    centered(ctx)
    small, out = ctx.pbs_lincomb(pool, items, ctx.lut(TABLE))
    _assert_words(small, rows_ref, "centered rows of the descriptor path")
    _assert_words(out, oracle_decompress(ok, rows_ref, TABLE), "centered bootstraps of the descriptor path")


@pytest.mark.parametrize("n,g", [(255, CLASSIC), (16, CLASSIC), (16, MULTIBIT), (2, CLASSIC), (2, MULTIBIT), (1, CLASSIC)],
                         ids=lambda v: str(v))
def test_other_dimensions(centered, n, g):
    _pbs_case(n, g, 8, centered)
    _, _, ok, ctx = _env(n, g)
    base, small = _fresh37(ok)
    for kind in KS.values():  # 37 rows: more than a workgroup's four, on both keyswitch kernels
        ctx.set_ks_kernel(kind)
        _assert_words(ctx.keyswitch(base), M.center_ref(small), f"n {n} grouping {g}: 37 centered rows, kernel {kind}")


# ---------------------------------------------------------------- radix layer
def test_radix_ops_centered(centered):
    ck, _, _, ctx = _env()
    centered(ctx)
    set_server_key(ctx)
    x, y = 0xDEADBEEF, 0x9E3779B9
    a, b = FheUint32.try_encrypt(x, ck), FheUint32.try_encrypt(y, ck)
    assert (a + b).decrypt(ck) == (x + y) % (1 << 32)
    assert (a * b).decrypt(ck) == (x * y) % (1 << 32)


def test_sign_vector0_centered(centered):
    ck, _, _, ctx = _env()
    centered(ctx)
    set_server_key(ctx)
    with open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")) as f:
        row = next(r for r in csv.DictReader(f) if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    sig = Schnorr().sign_fhe_with_k0(msg, k0, d, BigUintFHE.new(d, ck), ck, COMPAT)
    assert sig.hex().upper() == row["signature"].upper()


def test_fanout_mul_same_words_centered(centered):
    ck, _, _, ctx = _env()
    centered(ctx)
    set_server_key(ctx)
    x, y = 0xC0FFEE11, 0x0BADF00D

    def mul():
        ck.seed_encryption(91)  # identical inputs for both runs
        p = FheUint32.try_encrypt(x, ck) * FheUint32.try_encrypt(y, ck)
        return p.export(), p.decrypt(ck)

    words, value = mul()
    assert value == (x * y) % (1 << 32)
    ctx.set_fanout(min_level=1, emulate_ranks=2)
    split_words, split_value = mul()
    assert ctx.fanout_info()[1] == 2 and ctx.fanout_info()[2] > 0
    assert split_value == value and np.array_equal(split_words, words)
    # and the centered words are not the standard ones
    ctx.set_fanout(257, 0)
    ctx.set_modulus_switch("standard")
    assert not np.array_equal(mul()[0], words)


# ---------------------------------------------------------------- the measured margin
def test_measured_margin(centered):
    """4096 fresh encryptions through the GPU keyswitch in both modes; the modulus-switch error of a row is
    the phase of the switched row (every word rounded to the 2^52 grid) minus the phase of the 64-bit row the
    keyswitch wrote, under the small key, in grid steps.  The bounds are the two formulas +- 5 % (sampling error
    of a sigma over 4096 rows: 1 / sqrt(2 * 4096) = 1.1 %).  DESIGN.md 6g quotes the printed figures."""
    ck, _, ok, ctx = _env()
    n = ok.params.n
    key, _ = ck.export()
    assert np.array_equal(key, ok.lwe_sk) and set(np.unique(key).tolist()) <= {0, 1}
    hw = int(key.sum())
    r = ok.rng(0x51C)
    cts = np.stack([ok.encrypt(r, i % 16) for i in range(4096)])

    def phase(rows):
        return rows[:, n] - (rows[:, :n] * key[None, :]).sum(axis=1, dtype=np.uint64)

    def switched(rows):  # every word on the grid, as modswitch_2n leaves it (times 2^52)
        return rows - M.res(rows).astype(np.uint64)

    std = ctx.keyswitch(cts)
    centered(ctx)
    cen = ctx.keyswitch(cts)
    _assert_words(cen, M.center_ref(std), "centered rows of 4096")
    sig = {}
    for name, rows in (("standard", std), ("centered", cen)):
        err = (phase(switched(rows)) - phase(std)).astype(np.int64) / float(1 << 52)
        assert np.allclose(err, M.ms_error(std, key, centered=name == "centered"), rtol=0, atol=1e-9)
        sig[name] = float(err.std())
    f_std, f_cen = M.sigma_standard(hw), M.sigma_centered(n)
    print(f"\nmeasured margin, n {n}, hw {hw}, 4096 rows: standard sigma {sig['standard']:.3f} (formula {f_std:.3f}, "
          f"64 / sigma {64 / sig['standard']:.2f}); centered sigma {sig['centered']:.3f} (formula {f_cen:.3f}, "
          f"64 / sigma {64 / sig['centered']:.2f})")
    assert abs(sig["standard"] / f_std - 1) < 0.05
    assert abs(sig["centered"] / f_cen - 1) < 0.05
