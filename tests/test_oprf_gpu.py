"""Oblivious pseudo-random values on the GPU (oprf.hip, Engine::oprf; include/fhe_rocm.h "oblivious pseudo-random
values"), word for word.

  rows     Context.oprf_rows (k_oprf_rows) == tests/oprf_ref.py at every n of tests/test_oprf.py, at 1 .. 1024 rows,
           with the tight and the workspace stride, the padding marker intact
  blocks   Context.oprf_blocks == the oracle's fho_blind_rotate + fho_sample_extract of the reference rows through
           the reference accumulator, plus the body constant: every row at 1, 3 and 65 (latency kernel), 48 rows of
           320 and of 1024 (the throughput kernels), both `bits`, classic and multi-bit, n = 16 and 256; the same
           words in centered mode and with an emulated fan-out
  values   every block of 1024 decrypts to the reference's prediction, no exception: the counts are the CPU test's
  radix    FheUint.random / random_below / BigUintFHE.random decrypt to the assembled prediction, carry the right
           labels (sums and products of them decrypt), and leave a recorded, unflushed sum alone
  refusals no server key, bits out of range, a zero bound, a NULL seed under an attached transport
"""
import ctypes as C

import numpy as np
import pytest

import exact_pbs_ref as X
import oprf_ref as O
import oracle
from fhe_sign import (BigUintFHE, Context, FheError, FheUint8, FheUint32, FheUint64, _lib, generate_keys, ms_stride,
                      multi_bit_params, set_server_key, stats)
from fhe_sign.core import MS_PAD_WORD
from lwe_dims import CLASSIC, MULTIBIT, oracle_params, product_params
from test_oprf import BALANCE, BALANCE_ROWS, DIMS, KEY_SEED, SEED

pytestmark = pytest.mark.gpu
SEED2 = bytes(range(100, 132))
ROW_COUNTS = (1, 63, 64, 65, 257, 1024)

_envs = {}
_sks = {}


def _env(n=834, g=CLASSIC):
    """(client key, oracle keys, context) of one parameter set under KEY_SEED, made once"""
    if (n, g) not in _envs:
        if n == 834:
            pp = multi_bit_params() if g == MULTIBIT else None
            op = oracle.multibit_params() if g == MULTIBIT else None
        else:
            pp, op = product_params(n, g), oracle_params(n, g)
        ck, sk = generate_keys(pp, seed=KEY_SEED)
        ctx = Context(0)
        ctx.set_server_key(sk)
        ok = oracle.OracleKeys(KEY_SEED, op)
        assert np.array_equal(ck.export()[0], ok.lwe_sk)
        _envs[(n, g)] = (ck, ok, ctx)
        _sks[(n, g)] = sk
    return _envs[(n, g)]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    set_server_key(None)
    for _, _, ctx in _envs.values():
        ctx.close()
    _envs.clear()
    _sks.clear()


@pytest.fixture(scope="module")
def bare():
    ctx = Context(0)  # no server key: the rows entry needs none
    yield ctx
    ctx.close()


# ---------------------------------------------------------------- the row kernel
@pytest.mark.parametrize("n", DIMS)
def test_rows_equal_reference(bare, n):
    ws = ms_stride(n)
    ref = O.rows(SEED, n, max(ROW_COUNTS), ws)
    for count in ROW_COUNTS:
        wide = bare.oprf_rows(SEED, n, count, ws)
        assert wide.shape == (count, ws)
        bad = np.flatnonzero((wide != ref[:count]).any(axis=1))
        assert bad.size == 0, f"n {n}, {count} rows, stride {ws}: {bad.size} rows differ, first {bad[:5]}"
        assert (wide[:, n] == 0).all() and (wide[:, n + 1:] == np.uint64(MS_PAD_WORD)).all()
        tight = bare.oprf_rows(SEED, n, count, n + 1)
        assert np.array_equal(tight, ref[:count, :n + 1]), f"n {n}, {count} rows, stride n + 1"
    # a stride above the workspace's: the marker up to the end
    loose = bare.oprf_rows(SEED, n, 3, ws + 5)
    assert np.array_equal(loose[:, :ws], ref[:3]) and (loose[:, ws:] == np.uint64(MS_PAD_WORD)).all()


def test_rows_refuse_bad_shapes(bare):
    lib = _lib.load()
    buf = np.zeros(4100, np.uint64)
    for n, stride in ((0, 8), (2049, 2056), (16, 16)):
        assert lib.fhe_oprf_rows(bare.handle, SEED, n, 1, stride, _lib.ptr(buf)) == -1
    assert lib.fhe_oprf_rows(bare.handle, SEED, 16, 0, 17, _lib.ptr(buf)) == 0
    assert not buf.any()


# ---------------------------------------------------------------- blocks, word for word
def oracle_blocks(ok, rows, poly, const):
    """fho_blind_rotate + fho_sample_extract of the rows through an arbitrary polynomial (the way
    compress_ref.oracle_decompress drives the oracle), `const` added to the body: (len(rows), 2049) words"""
    lib = oracle.load()
    n = ok.params.n
    rows = np.ascontiguousarray(np.asarray(rows, np.uint64)[:, :n + 1])
    poly = np.ascontiguousarray(poly, np.uint64)
    out = np.zeros((rows.shape[0], 2049), np.uint64)

    def one(i):
        glwe = np.zeros(2 * 2048, np.uint64)
        lib.fho_blind_rotate(ok.ref, rows[i].ctypes.data_as(oracle.u64p), poly.ctypes.data_as(oracle.u64p),
                             glwe.ctypes.data_as(oracle.u64p))
        lib.fho_sample_extract(glwe.ctypes.data_as(oracle.u64p), out[i].ctypes.data_as(oracle.u64p))

    one(0)  # the oracle's shared tables are made by the first call, before the threads read them
    X.threads_map(one, range(1, rows.shape[0]), 8)
    with np.errstate(over="ignore"):
        out[:, 2048] += np.uint64(const)
    return out


def sample(count):
    """every row up to 65; above, 48 rows: the first, the last and 46 spread evenly between them (their step is
    no integer, so odd and even positions both occur)"""
    if count <= 65:
        return np.arange(count)
    return np.unique(np.r_[0, count - 1, 1 + np.arange(46) * (count - 3) // 45])


_oref = {}


def oracle_ref(n, g, bits, idx):
    """the oracle's blocks of the seed's rows idx, each row computed once per key set and bits"""
    _, ok, _ = _env(n, g)
    have = _oref.setdefault((n, g, bits), {})
    need = [int(i) for i in idx if int(i) not in have]
    if need:
        rows = O.rows(SEED, n, max(need) + 1)[need]
        blocks = oracle_blocks(ok, rows, O.lut(bits), O.body_const(bits))
        for i, b in zip(need, blocks):
            b.setflags(write=False)
            have[i] = b
    return np.stack([have[int(i)] for i in idx])


def assert_blocks(got, ref, what):
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(ref)} blocks differ, first {bad[:5]}"


@pytest.mark.parametrize("bits", (1, 2))
@pytest.mark.parametrize("g", (CLASSIC, MULTIBIT), ids=("classic", "multibit"))
@pytest.mark.parametrize("count", (1, 3, 65, 320, 1024))
def test_blocks_equal_oracle(count, g, bits):
    _, ok, ctx = _env(834, g)
    idx = sample(count)
    assert idx[0] == 0 and idx[-1] == count - 1 and len(idx) == min(count, 48 if count > 65 else 65)
    got = ctx.oprf_blocks(SEED, count, bits)
    assert got.shape == (count, 2049)
    assert_blocks(got[idx], oracle_ref(834, g, bits, idx), f"grouping {g}, bits {bits}, {count} blocks")
    if count == 65:  # an ordinary block of the declared degree: every one decrypts below 2^bits
        assert all(ok.decrypt(c) < (1 << bits) for c in got)


@pytest.mark.parametrize("n,g", [(16, CLASSIC), (16, MULTIBIT), (256, CLASSIC), (256, MULTIBIT)], ids=lambda v: str(v))
def test_blocks_other_dimensions(n, g):
    _, ok, ctx = _env(n, g)
    for bits, count in ((2, 65), (1, 3), (2, 320)):
        idx = sample(count)
        got = ctx.oprf_blocks(SEED, count, bits)
        assert_blocks(got[idx], oracle_ref(n, g, bits, idx), f"n {n} grouping {g}, bits {bits}, {count} blocks")


def test_same_words_centered_and_fanned_out():
    _, _, ctx = _env()
    base = {count: ctx.oprf_blocks(SEED, count, 2) for count in (65, 320)}
    assert_blocks(base[65], oracle_ref(834, CLASSIC, 2, np.arange(65)), "the base run")
    try:
        ctx.set_modulus_switch("centered")
        for count, ref in base.items():
            assert np.array_equal(ctx.oprf_blocks(SEED, count, 2), ref), f"centered mode changed {count} blocks"
        ctx.set_modulus_switch("standard")
        ctx.set_fanout(257, 2)
        for count, ref in base.items():
            assert np.array_equal(ctx.oprf_blocks(SEED, count, 2), ref), f"emulated fan-out changed {count} blocks"
    finally:
        ctx.set_modulus_switch("standard")
        ctx.set_fanout(257, 0)


def test_chunked_call_equals_unchunked():
    """more rows than the workspace holds go in chunks of it: 4096 + 37 rows on a fresh context (workspace 4096)
    give, at the sampled rows, the words a call that ends there gives"""
    _env()
    ctx = Context(0)
    try:
        ctx.set_server_key(_sks[(834, CLASSIC)])
        big = ctx.oprf_blocks(SEED, 4096 + 37, 2)
        assert_blocks(big[:65], oracle_ref(834, CLASSIC, 2, np.arange(65)), "the head of a chunked call")
        tail = np.arange(4090, 4096 + 37)
        assert_blocks(big[tail], oracle_ref(834, CLASSIC, 2, tail), "across the chunk boundary")
    finally:
        ctx.close()


# ---------------------------------------------------------------- values
def decode_all(blocks, glwe_sk):
    phase = X.lwe_phase(blocks, glwe_sk)
    with np.errstate(over="ignore"):
        return ((phase + np.uint64(O.DELTA // 2)) // np.uint64(O.DELTA)) % np.uint64(16)


@pytest.mark.parametrize("bits", (1, 2))
@pytest.mark.parametrize("g", (CLASSIC, MULTIBIT), ids=("classic", "multibit"))
def test_values_equal_prediction(g, bits):
    ck, ok, ctx = _env(834, g)
    got = decode_all(ctx.oprf_blocks(SEED, BALANCE_ROWS, bits), ok.glwe_sk).astype(np.int64)
    want = O.values(O.rows(SEED, 834, BALANCE_ROWS), ok.lwe_sk, bits)
    bad = np.flatnonzero(got != want)
    print(f"grouping {g}, bits {bits}: {bad.size} exceptions, counts {np.bincount(got, minlength=1 << bits).tolist()}")
    assert bad.size == 0, f"{bad.size} blocks off the prediction, first {bad[:5]}"
    assert np.bincount(got, minlength=1 << bits).tolist() == BALANCE[bits]


# ---------------------------------------------------------------- radix layer
@pytest.fixture
def keyed():
    ck, ok, ctx = _env()
    set_server_key(ctx)
    return ck, ok, ctx


def test_radix_random(keyed):
    ck, ok, ctx = keyed
    want32, _ = O.radix_value(SEED, ok.lwe_sk, 32, 32)
    x = FheUint32.random(SEED)
    assert x.decrypt(ck) == want32
    want13, blocks13 = O.radix_value(SEED, ok.lwe_sk, 32, 13)
    y = FheUint32.random(SEED, random_bits=13)
    assert y.decrypt(ck) == want13 < (1 << 13)
    words = y.export()
    assert not words[7:].any(), "the blocks above random_bits are trivial zeros"
    assert all(words[i].any() for i in range(7)), "the random blocks are ciphertexts"
    assert [ok.decrypt(words[i]) for i in range(7)] == blocks13[:7] and blocks13[6] in (0, 1)
    assert np.array_equal(words[:6], x.export()[:6]), "the full blocks are the rows of their index"
    # row 6 at one bit is another ciphertext than row 6 at two
    assert not np.array_equal(words[6], x.export()[6])
    # one seed repeats word for word, two seeds differ
    assert np.array_equal(FheUint32.random(SEED).export(), x.export())
    z = FheUint32.random(SEED2)
    assert z.decrypt(ck) == O.radix_value(SEED2, ok.lwe_sk, 32, 32)[0] != want32
    # OS entropy: a value of the width, two draws differ (64 random bits)
    assert FheUint64.random().decrypt(ck) != FheUint64.random().decrypt(ck)


def test_radix_labels(keyed):
    """degree 3 / 1 and noise 1 are what the block is: sums and products of random values decrypt"""
    ck, ok, _ = keyed
    a, b = O.radix_value(SEED, ok.lwe_sk, 8, 8)[0], O.radix_value(SEED2, ok.lwe_sk, 8, 8)[0]
    x, y = FheUint8.random(SEED), FheUint8.random(SEED2)
    assert (x + y).decrypt(ck) == (a + b) % 256
    assert (x * 3).decrypt(ck) == (a * 3) % 256
    assert (x * y).decrypt(ck) == (a * b) % 256
    odd = FheUint8.random(SEED, random_bits=5)
    assert (odd + odd).decrypt(ck) == 2 * O.radix_value(SEED, ok.lwe_sk, 8, 5)[0]


def test_pending_graph_is_left_alone(keyed):
    ck, ok, ctx = keyed
    a, b = FheUint32.try_encrypt(0xDEADBEEF, ck), FheUint32.try_encrypt(0x9E3779B9, ck)
    s = a + b  # recorded, not flushed
    pbs0, levels0 = stats(ctx)
    r = FheUint32.random(SEED)
    # 16 bootstraps counted, no level launched: the sum is still pending
    assert stats(ctx) == (pbs0 + 16, levels0)
    assert s.decrypt(ck) == (0xDEADBEEF + 0x9E3779B9) % (1 << 32)
    assert r.decrypt(ck) == O.radix_value(SEED, ok.lwe_sk, 32, 32)[0]


def test_biguint_random(keyed):
    ck, ok, _ = keyed
    x = BigUintFHE.random(64, SEED)
    want = O.radix_value(SEED, ok.lwe_sk, 64, 64)[0]
    assert x.decrypt_limbs(ck) == [want & 0xFFFFFFFF, want >> 32]


def test_random_below(keyed):
    ck, ok, ctx = keyed
    r16 = O.radix_value(SEED, ok.lwe_sk, 16, 16)[0]
    assert O.random_below_bits(200, 8) == 16
    got = FheUint8.random_below(200, SEED, extra_bits=8).decrypt(ck)
    assert got == O.random_below(r16, 200, 16) == (r16 * 200) >> 16 and got < 200
    assert FheUint8.random_below(1, SEED, extra_bits=8).decrypt(ck) == 0
    assert FheUint8.random_below(1, SEED).decrypt(ck) == 0  # the default 64 extra bits
    m = O.random_below_bits(256, 8)
    assert FheUint8.random_below(256, SEED, extra_bits=8).decrypt(ck) == \
        O.random_below(O.radix_value(SEED, ok.lwe_sk, 16, m)[0], 256, m)
    with pytest.raises(FheError) as e:
        FheUint8.random_below(0, SEED)
    assert e.value.code == -1 and "bound" in str(e.value)
    with pytest.raises(FheError) as e:  # values below 257 do not fit eight bits
        FheUint8.random_below(257, SEED)
    assert e.value.code == -1
    with pytest.raises(FheError) as e:  # 12 + 4090 + 13 bits: more than a radix integer holds
        FheUint32.random_below(4097, SEED, extra_bits=4090)
    assert e.value.code == -1


# ---------------------------------------------------------------- refusals
def test_refusals(keyed):
    ck, ok, ctx = keyed
    lib = _lib.load()
    buf = np.zeros(2049 * 2, np.uint64)
    h = C.c_void_p()
    for bits in (0, 3):
        assert lib.fhe_oprf_blocks(ctx.handle, SEED, 2, bits, _lib.ptr(buf)) == -1  # FHE_ERR_INVALID
        assert b"bits" in lib.fhe_last_error()
    assert not buf.any()
    for width, rb in ((7, 3), (0, 0), (8, 0), (8, 9), (4098, 8)):
        assert lib.fhe_radix_random(ctx.handle, SEED, width, rb, C.byref(h)) == -1
    assert lib.fhe_biguint_random(ctx.handle, SEED, 48, C.byref(h)) == -1
    assert h.value is None
    # no server key
    bare = Context(0)
    try:
        assert lib.fhe_oprf_blocks(bare.handle, SEED, 2, 2, _lib.ptr(buf)) == -3  # FHE_ERR_NO_KEY
        assert lib.fhe_radix_random(bare.handle, SEED, 8, 8, C.byref(h)) == -3
        assert lib.fhe_biguint_random(bare.handle, SEED, 32, C.byref(h)) == -3
        one = np.array([5], np.uint64)
        assert lib.fhe_radix_random_below(bare.handle, SEED, 8, _lib.ptr(one), 1, 8, C.byref(h)) == -3
    finally:
        bare.close()


def test_null_seed_refused_under_a_transport(keyed):
    """a stub transport of two ranks in one process: nothing it carries is ever called, the refusal comes first"""
    ck, ok, ctx = keyed
    lib = _lib.load()
    cbs = (_lib.TX_BCAST(lambda *a: 1), _lib.TX_ALLGATHER(lambda *a: 1), _lib.TX_MIN_U8(lambda *a: 1))
    tx = _lib.TestTransport(None, *cbs)
    _lib.check(lib.fhe_ctx_attach_test_transport(ctx.handle, C.byref(tx), 2, 0))
    try:
        for call in (lambda: FheUint8.random(), lambda: FheUint8.random_below(5), lambda: BigUintFHE.random(32)):
            with pytest.raises(FheError) as e:
                call()
            assert e.value.code == -1 and "communicator" in str(e.value)
    finally:
        ctx.detach_comm()
    assert FheUint8.random(SEED).decrypt(ck) == O.radix_value(SEED, ok.lwe_sk, 8, 8)[0]
