"""Both keyswitch kernels and the fused linear prologue of the radix layer's descriptors against the
oracle WORD FOR WORD (fhe_keyswitch_batch, fhe_pbs_lincomb_batch).

Every other GPU check of the keyswitch goes through a bootstrap, and the blind rotation reads a small
LWE word only through the modulus switch (bits 51 and up): tests/test_keyswitch_ref.py records that
losing byte planes 0-3 of the matrix-core contraction, or a low-bit error of the prologue, changes no
bootstrap.  Here every comparison is exact equality of 64-bit words; a failure reports how many words
differ, the first (ciphertext, word) and the XOR of the two words, whose set bits name the byte plane.
"""
import ctypes as C

import numpy as np
import pytest

import ks_ref
import oracle
from fhe_sign import Context, FheError, _lib, generate_keys, multi_bit_params
from test_pbs_gpu import _luts

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
KS = {"valu": 0, "mfma": 1}
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

_envs = {}


def _make_env(kind):
    if kind not in _envs:
        mb = kind == "multibit"
        ck, sk = generate_keys(multi_bit_params() if mb else None, seed=SEED)
        ok = oracle.OracleKeys(SEED, oracle.multibit_params() if mb else None)
        ctx = Context(0)
        ctx.set_server_key(sk)
        _envs[kind] = (ck, sk, ok, ctx)
    return _envs[kind]


@pytest.fixture(scope="module")
def env():
    """classic keys (the keyswitching key does not depend on the blind rotation)"""
    yield _make_env("classic")
    for _, _, _, ctx in _envs.values():
        ctx.close()
    _envs.clear()


@pytest.fixture(scope="module", params=["classic", "multibit"])
def env_br(request, env):
    """both blind rotations, as tests/test_pbs_gpu.py's env: classic (grouping 1) and multi-bit
    (grouping 2); the classic one is `env`'s context"""
    return _make_env(request.param)


@pytest.fixture(params=list(KS))
def ks(request, env):
    ctx = env[3]
    ctx.set_ks_kernel(KS[request.param])
    yield request.param
    ctx.set_ks_kernel(1)


def _assert_words(got, ref, what):
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad = np.argwhere(got != ref)
    if len(bad):
        i, j = (int(v) for v in bad[0])
        x = int(got[i, j]) ^ int(ref[i, j])
        pytest.fail(f"{what}: {len(bad)} of {got.size} words differ, first at (ciphertext {i}, word {j}): "
                    f"{int(got[i, j]):#018x} != {int(ref[i, j]):#018x}, xor {x:#018x}")


# ---------------------------------------------------------------- contiguous input: batch sizes
_base = {}


def _base131(ok):
    """131 distinct encryptions and their keyswitch by the oracle, computed once"""
    if "cts" not in _base:
        r = ok.rng(4242)
        _base["cts"] = np.stack([ok.encrypt(r, i % 16) for i in range(131)])
        _base["ref"] = ok.keyswitch_batch(_base["cts"])
        for a in _base.values():
            a.setflags(write=False)
    return _base["cts"], _base["ref"]


# Launch shapes behind the counts (n + 1 = 835 output words):
#  ks_mfma.hip launch_keyswitch_mfma: 53 column tiles of 16; a workgroup column holds 64 CW
#    ciphertexts, CW = 2 below KS_CW_BIG_FROM = 4096 and 4 from there; the contraction is split 1, 2,
#    4, 8 or 16 ways (KS_MAX_SPLITS), the fewest that give >= 768 workgroups, and a split launch
#    subtracts atomically from the row k_ks_digits initialised:
#      count    1: 1 column  x 53 -> 16 splits      count 1000:  8 columns x 53 -> 2 splits
#      count  129: 2 columns x 53 ->  8 splits      count 1930: 16 columns x 53 -> 1 split (plain store)
#      count  513: 5 columns x 53 ->  4 splits      count 4097: CW = 4, 17 columns (the last holds one
#                                                               ciphertext) x 53 = 901 -> 1 split
#    16 and 17 straddle a 16-row digit tile (16 splits both).
#  pbs_kernels.hip launch_keyswitch: KS_C = 16 ciphertexts x 256 words per workgroup, base =
#    ceil(count / 16) * 4 workgroups, ks_splits doubles up to 64 while base * splits * 2 <= 1024, and a
#    split launch adds atomically into a row cleared by a memset:
#      1, 16 -> 64   17 -> 64 (two ciphertext groups)   129 -> 16   513, 1000 -> 4   1930 -> 2   4097 -> 1
# Large, small, large, small: a row an earlier launch left initialised (or not) would show.
COUNTS = (1930, 1, 16, 17, 129, 513, 1000, 4097, 1)


def test_keyswitch_words_equal_oracle(env, ks):
    _, _, ok, ctx = env
    base, ref = _base131(ok)
    for count in COUNTS:
        got = ctx.keyswitch(np.resize(base, (count, 2049)))
        _assert_words(got, np.resize(ref, (count, ref.shape[1])), f"{ks} keyswitch of {count}")


def test_keyswitch_digit_edges(env, ks):
    """hand-built rows with the rounding bit and every digit carry chain at their edges
    (ks_ref.edge_rows) among ordinary encryptions, against the integer restatement and the oracle"""
    _, sk, ok, ctx = env
    base, base_ref = _base131(ok)
    rows = ks_ref.edge_rows()
    ksk, _ = sk.export()
    n = ok.params.n
    by_oracle = ok.keyswitch_batch(rows)
    by_ref = ks_ref.keyswitch_np(ksk, n, rows)
    assert np.array_equal(by_oracle, by_ref)
    assert not by_ref[3][:n].any() and by_ref[3][n] == rows[3][2048]  # zero mask: (0, .., 0, body)
    assert not by_ref[2][:n].any() and by_ref[2][n] == rows[2][2048]  # all ones: zero digits
    got = ctx.keyswitch(rows)
    _assert_words(got, by_ref, f"{ks} keyswitch of the edge rows")
    # and inside a 16-row tile of other ciphertexts
    mixed = np.concatenate([base[:7], rows, base[7:20]])
    got = ctx.keyswitch(mixed)
    _assert_words(got, np.concatenate([base_ref[:7], by_oracle, base_ref[7:20]]), f"{ks} keyswitch, edge rows in a tile")


def test_keyswitch_empty_batch_and_no_key(env):
    _, _, ok, ctx = env
    assert ctx.keyswitch(np.zeros((0, 2049), np.uint64)).shape == (0, ok.params.n + 1)
    bare = Context(0)
    try:
        with pytest.raises(FheError) as e:
            bare.keyswitch(np.zeros((1, 2049), np.uint64))
        assert e.value.code == -3  # FHE_ERR_NO_KEY
        with pytest.raises(FheError) as e:
            bare.pbs_lincomb(np.zeros((1, 2049), np.uint64), [([(0, 1)], 0)], 0)
        assert e.value.code == -3
    finally:
        bare.close()


# ---------------------------------------------------------------- descriptors: the linear prologue
def _pool(ok):
    """40 blocks: 38 encryptions, a trivial block (mask 0) and an all-ones block"""
    r = ok.rng(1234)
    pool = np.zeros((40, 2049), np.uint64)
    for i in range(38):
        pool[i] = ok.encrypt(r, (5 * i + 2) % 16)
    pool[38, 2048] = np.uint64(3 * ok.delta())
    pool[39, :] = np.uint64((1 << 64) - 1)
    return pool


def _items(delta):
    """([(src, coef), ...], cst): 1 to 6 terms use the descriptor's inline form (int32 coefficients),
    7 to 32 a staged term table (int64 coefficients)"""
    wide7 = [(3 + 2 * t, t - 3) for t in range(7)]
    wide7[0] = (3, -((1 << 40) + 3))  # int64 coefficients: a 32-bit read would lose them
    wide7[6] = (38, 1 << 33)
    wide20 = [((7 * t + 1) % 40, (-1) ** t * (t + 1)) for t in range(20)]
    wide20[19] = (39, -((1 << 40) + 3))
    wide32 = [(t, 3 - (t % 7)) for t in range(32)]  # coefficient 0 included
    wide32[31] = (0, 1 << 33)  # repeats source 0; the last entry of the largest table
    return [
        ([(0, 1)], 0),
        ([(1, -1)], 5 * delta),
        ([(2, 2), (39, -3)], (1 << 64) - 1),
        ([(4, -7), (5, 4), (6, INT32_MIN), (7, INT32_MAX), (4, 1), (38, -1)], 5 * delta),  # repeats source 4
        (wide7, 0),
        (wide20, (1 << 64) - 1),
        (wide32, 5 * delta),
    ]


_lin = {}


def _lincomb_reference(ok, count):
    """(pool, items, combined inputs, keyswitched words by the oracle) for the item list repeated to `count`"""
    key = int(ok.params.grouping)
    if key not in _lin:
        pool = _pool(ok)
        items = _items(ok.delta())
        comb = np.stack([ks_ref.lincomb_np(pool, t, c) for t, c in items])
        _lin[key] = (pool, items, comb, ok.keyswitch_batch(comb))
        for a in (pool, comb, _lin[key][3]):
            a.setflags(write=False)
    pool, items, comb, small = _lin[key]
    reps = [i % len(items) for i in range(count)]
    return pool, [items[i] for i in reps], comb[reps], small[reps]


def test_lincomb_keyswitch_words(env, ks):
    """k_ks_digits<true> / k_keyswitch<true>: the inline and the wide descriptor form at sign-extension,
    table-length and constant edges, at 1, 37 and 300 items"""
    _, _, ok, ctx = env
    ident = ctx.lut(list(range(16)))
    for count in (1, 37, 300):
        pool, items, _, ref = _lincomb_reference(ok, count)
        small, out = ctx.pbs_lincomb(pool, items, ident, want_small=True, want_out=False)
        assert out is None
        _assert_words(small, ref, f"{ks} keyswitch of {count} linear combinations")


def _radix_items(ok, ctx):
    """eight inputs of the radix layer's largest shape, 4 s0 + 2 s1 + s2 + c (carry_prefix), over 32
    identity-bootstrapped unit-noise blocks, as tests/test_pbs_gpu.py::test_noise_budget_at_radix_limit
    builds them: (blocks, items over those blocks, their messages)"""
    rs = np.random.default_rng(5)
    s = rs.integers(0, 3, size=(3, 8))
    c = rs.integers(0, 2, size=8)
    r = ok.rng(77)
    fresh = np.stack([ok.encrypt(r, int(v)) for v in np.concatenate([s.ravel(), c])])
    unit = ctx.pbs(fresh, ctx.lut(list(range(16))))
    items = [([(i, 4), (8 + i, 2), (16 + i, 1), (24 + i, 1)], 0) for i in range(8)]
    return unit, items, 4 * s[0] + 2 * s[1] + s[2] + c


def test_lincomb_pbs_words(env_br):
    """the whole descriptor path as Engine::flush runs it -- fused prologue, keyswitch, blind rotate
    writing through desc.dst -- against the oracle's bootstrap of the integer linear combination, on the
    latency kernel, qy and (classic) qy2, with every LUT; the radix-shaped items also decrypt to
    their carry"""
    _, _, ok, ctx = env_br
    classic = ok.params.grouping <= 1
    tables = _luts() + [[1 if v >= 8 else 0 for v in range(16)]]
    ids = [ctx.lut(t) for t in tables]
    pool, items, comb, small_ref = _lincomb_reference(ok, 37)
    unit, ritems, msgs = _radix_items(ok, ctx)
    blocks = np.concatenate([pool, unit])
    items = items + [([(40 + s, k) for s, k in t], c) for t, c in ritems]
    lut_of = np.array([i % 5 for i in range(37)] + [5] * 8, np.uint32)
    comb = np.concatenate([comb, np.stack([ks_ref.lincomb_np(unit, t, c) for t, c in ritems])])
    ref = ok.pbs_batch(comb, np.stack([ok.make_lut(t) for t in tables]), lut_of)
    assert [ok.decrypt(o) for o in ref[37:]] == [int(m >= 8) for m in msgs]
    paths = [("latency", 1 << 30, 7), ("qy", 0, 4)] + ([("qy2", 0, 5)] if classic else [])
    try:
        for name, threshold, kind in paths:
            ctx.set_wide_threshold(threshold)
            ctx.set_br_kernel(kind)
            small, out = ctx.pbs_lincomb(blocks, items, [ids[k] for k in lut_of])
            _assert_words(small[:37], small_ref, f"{name}: keyswitched words")
            _assert_words(out, ref, f"{name}: bootstrapped words")
            assert [ok.decrypt(o) for o in out[37:]] == [int(m >= 8) for m in msgs]
    finally:
        ctx.set_wide_threshold(256)
        ctx.set_br_kernel(7)


def test_lincomb_refuses_bad_arguments(env):
    """every refusal is FHE_ERR_INVALID and leaves the context usable"""
    _, _, ok, ctx = env
    ident = ctx.lut(list(range(16)))
    pool = _pool(ok)[:4]

    def refused(items, lut=ident):
        with pytest.raises(FheError) as e:
            ctx.pbs_lincomb(pool, items, lut)
        return e.value.code == -1

    assert refused([([], 0)])                                        # no term
    assert refused([([(0, 1)], 0), ([], 0), ([(1, 1)], 0)])          # ... in the middle
    assert refused([([(t % 4, 1) for t in range(33)], 0)])           # more than 32 terms
    assert refused([([(4, 1)], 0)])                                  # block index out of range
    assert refused([([(t % 4, 1) for t in range(7)] + [(4, 1)], 0)])  # ... in a wide item
    assert refused([([(0, INT32_MAX + 1)], 0)])                      # inline coefficient outside int32
    assert refused([([(0, 1), (1, INT32_MIN - 1)], 0)])
    assert refused([([(0, 1)], 0)], lut=1 << 20)                     # unknown LUT id
    # term_off decreasing / not starting at 0: only expressible below the Python wrapper
    lib = _lib.load()
    src, coef = np.zeros(4, np.uint32), np.ones(4, np.int64)
    cst, ids = np.zeros(2, np.uint64), np.full(2, ident, np.uint32)
    small = np.zeros((2, ok.params.n + 1), np.uint64)
    for off in ([0, 2, 1], [1, 2, 3]):
        off = np.array(off, np.uint32)
        rc = lib.fhe_pbs_lincomb_batch(ctx.handle, _lib.ptr(pool), 4, _lib.ptr(off, C.c_uint32), _lib.ptr(src, C.c_uint32),
                                       _lib.ptr(coef, C.c_int64), _lib.ptr(cst), _lib.ptr(ids, C.c_uint32), 2,
                                       _lib.ptr(small), None)
        assert rc == -1
    # a 7-term item may carry what an inline one may not, and the context still works
    wide = [([(t % 4, INT32_MAX + 1) for t in range(7)], 0)]
    got, _ = ctx.pbs_lincomb(pool, wide, ident, want_out=False)
    _assert_words(got, ok.keyswitch_batch(ks_ref.lincomb_np(pool, *wide[0])[None, :]), "wide item after refusals")
    assert ctx.pbs_lincomb(pool, [], ident)[0].shape == (0, ok.params.n + 1)
