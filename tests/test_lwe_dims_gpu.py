"""Every kernel at LWE dimensions other than the default 834, and re-keying a context between them.

The C ABI accepts any lwe_dimension in [1, 2048] that the grouping divides (Params::from_c) and every
kernel takes n at run time, but the word-for-word pins of test_pbs_gpu.py, test_keyswitch_gpu.py and
test_keygen_gpu.py all hold at n = 834, where n + 1 = 835 pads to a row stride of 840, the matrix-core
keyswitch has 53 column tiles with 3 live columns in the last, the VALU keyswitch has gridDim.y = 4,
and n is even, so the classic blind rotations always end on a reduced accumulator update.  The sets of
tests/lwe_dims.py (cl = classic, mb = multi-bit) reach what 834 does not:

    n     grouping  reaches
    1     cl        one CMUX; the mask prefetch clamps onto the body; 2-word rows at stride 8; one MFMA
                    tile with 2 live columns
    2     cl, mb    mb: a single group, the "next group" loads never execute
    15    cl        n + 1 = 16: stride == n + 1, one exactly full MFMA tile; odd n: the classic epilogue
                    converts an unreduced accumulator
    16    cl, mb    n + 1 = 17: a second tile with one live column; stride 24
    255   cl        n + 1 = 256: VALU gridDim.y = 1 with every thread active; odd; k_ksk_bodies reduces a
                    row in one partial pass
    256   cl, mb    VALU gridDim.y = 2 with one active thread in the last block
    833   cl        odd n at production depth: the unreduced final update after 833 CMUXes
    2048  cl, mb    the largest dimension: stride 2056, 129 tiles with one live column in the last, VALU
                    gridDim.y = 9, the largest key offsets, 2048 (cl) / 3072 (mb) GGSWs

All comparisons are exact equality of 64-bit words against the oracle (oracle/tfhe_oracle.c).
"""
import ctypes as C
import random
import time

import numpy as np
import pytest

import ks_ref
import oracle
import ref_semantics as R
from fhe_sign import COMPAT, BigUintFHE, Context, FheError, FheUint32, _lib, generate_keys, set_server_key
from lwe_dims import CLASSIC, MULTIBIT, SETS, oracle_params, product_params, set_id
from test_keyswitch_gpu import _assert_words, _items, _pool
from test_pbs_gpu import _luts

pytestmark = pytest.mark.gpu
SEED = 0xD1A5
KS = (("valu", 0), ("mfma", 1))

# key sets the re-key test shares with the per-set environments (host + oracle keygen of n = 2048 is
# seconds of CPU); dropped at the end of the module
_KEEP = {(16, CLASSIC), (2048, CLASSIC)}
_kept = {}


def _keys(n, g):
    if (n, g) in _kept:
        return _kept[(n, g)]
    ck, sk = generate_keys(product_params(n, g), seed=SEED)
    ok = oracle.OracleKeys(SEED, oracle_params(n, g))
    if (n, g) in _KEEP:
        _kept[(n, g)] = (ck, sk, ok)
    return ck, sk, ok


@pytest.fixture(scope="module", autouse=True)
def _drop_kept_keys():
    yield
    _kept.clear()


class Env:
    def __init__(self, n, g):
        self.n, self.g = n, g
        self.ck, self.sk, self.ok = _keys(n, g)
        self.ctx = Context(0)
        self.ctx.set_server_key(self.sk)


@pytest.fixture(scope="module", params=SETS, ids=set_id)
def env(request):
    """host keys, oracle keys and a context with the key installed, one per parameter set"""
    e = Env(*request.param)
    yield e
    e.ctx.close()


# ---------------------------------------------------------------- device keygen
def test_device_keygen_and_fourier_bsk(env):
    """k_chacha_u64, k_ksk_bodies (rows of n words over 256 threads: below, at and above one pass) and
    k_bsk_bodies == the host's and the oracle's key words; the installed Fourier BSK == the oracle's"""
    ck_d, sk_d = generate_keys(product_params(env.n, env.g), seed=SEED, device=env.ctx)
    ok = env.ok
    lwe, glwe = ck_d.export()
    assert np.array_equal(lwe, ok.lwe_sk) and np.array_equal(glwe, ok.glwe_sk)
    ksk_d, bsk_d = sk_d.export()
    ksk_h, bsk_h = env.sk.export()
    assert ksk_d.shape == ksk_h.shape == ok.ksk.shape and bsk_d.shape == bsk_h.shape == ok.bsk.shape
    assert np.array_equal(ksk_d, ok.ksk) and np.array_equal(ksk_h, ok.ksk)
    assert np.array_equal(bsk_d, ok.bsk) and np.array_equal(bsk_h, ok.bsk)
    gpu = env.ctx.export_fourier_bsk()
    ref = oracle.fourier_bsk_gpu_layout(ok.bsk_f, ok.ggsw_count)
    assert gpu.shape == ref.shape
    bad = np.flatnonzero(gpu.view(np.uint64) != ref.view(np.uint64))
    assert bad.size == 0, f"{bad.size} mismatching doubles, first at {bad[:5]}"


# ---------------------------------------------------------------- keyswitch words, contiguous input
# The two split rules, restated (the test below checks its own table against them):
#  ks_mfma.hip launch_keyswitch_mfma: tiles = ceil((n + 1) / 16) column tiles; a workgroup column
#    holds 64 CW ciphertexts, CW = 2 below 4096 and 4 from there; the contraction is split the fewest
#    of 1, 2, 4, 8, 16 ways that give columns * tiles * splits >= 768 workgroups; a split launch
#    subtracts atomically from the row k_ks_digits initialised, a single split stores.
#  pbs_kernels.hip launch_keyswitch: base = ceil(count / 16) * ceil((n + 1) / 256) workgroups, splits
#    double up to 64 while base * splits * 2 <= 1024; a split launch adds atomically into a row a memset
#    cleared, a single split stores.
def _mfma_shape(n, count):
    cw = 4 if count >= 4096 else 2
    tiles, xb = (n + 16) // 16, (count + 64 * cw - 1) // (64 * cw)
    splits = 1
    while splits < 16 and xb * tiles * splits < 768:
        splits *= 2
    return cw, xb, tiles, splits


def _valu_shape(n, count):
    groups, ys = (count + 15) // 16, (n + 256) // 256
    splits = 1
    while splits < 64 and groups * ys * splits * 2 <= 1024:
        splits *= 2
    return groups, ys, splits


# Counts per n, large, small, large: a row the previous launch left initialised (or not) would show.
# Reachable with at most 4200 ciphertexts (the largest batch a test here affords) and reached:
#     n          tiles  ys  count: MFMA splits (CW, columns) / VALU splits
#     1, 2, 15   1      1   1300: 16 (2, 11) / 8    1: 16 / 64    17: 16 / 64    600: 16 (2, 5) / 16
#                           -- 1 tile: MFMA always the maximum split; VALU never a single split
#     16         2      1   4097: 16 (CW 4, 17 columns, the last with one ciphertext) / 2    1: 16 / 64
#                           17: 16 / 64    1300: 16 / 8    -- MFMA always the maximum split
#     255        16     1   3000: 2 (2, 24) / 4    1: 16 / 64    17: 16 / 64    700: 8 (2, 6) / 16
#     256        17     2   4097: 4 (CW 4, 17) / 1 (plain store)    1: 16 / 64    17: 16 / 64
#                           700: 8 (2, 6) / 8    3000: 2 (2, 24) / 2   -- MFMA: no single split below 4200
#     833        53     4   2100: 1 (plain store; 2, 17) / 1    1: 16 / 64    17: 16 / 64    513: 4 / 4
#     2048       129    9   4096: 1 (CW 4, 16) / 1    1: 8 / 64    17: 8 / 32    300: 2 (2, 3) / 4
#                           700: 1 (2, 6) / 2   -- 129 tiles: 8 is the maximum split any count reaches
KS_COUNTS = {
    1: (1300, 1, 17, 600), 2: (1300, 1, 17, 600), 15: (1300, 1, 17, 600),
    16: (4097, 1, 17, 1300),
    255: (3000, 1, 17, 700),
    256: (4097, 1, 17, 700, 3000),
    833: (2100, 1, 17, 513),
    2048: (4096, 1, 17, 300, 700),
}
MAX_COUNT = 4200


def test_keyswitch_counts_reach_every_split_case():
    """the table above against the restated split rules (CPU arithmetic only): per n, the maximum split
    any batch of up to MAX_COUNT reaches, an intermediate one where there is one, the single-split
    plain-store path where such a batch reaches it, on both kernels; CW = 4 at n = 16 and n = 2048"""
    for n, counts in KS_COUNTS.items():
        for shape, pos in ((_mfma_shape, 3), (_valu_shape, 2)):
            reachable = {shape(n, c)[pos] for c in range(1, MAX_COUNT + 1)}
            got = {shape(n, c)[pos] for c in counts}
            assert max(reachable) in got and (1 in got or 1 not in reachable), (n, shape.__name__, reachable, got)
            assert got - {max(reachable), 1} or not reachable - {max(reachable), 1}, (n, shape.__name__, reachable, got)
        assert max(counts) <= MAX_COUNT and counts[0] > counts[1] < counts[-1]
    for n in (16, 2048):
        assert any(_mfma_shape(n, c)[0] == 4 for c in KS_COUNTS[n])


def _base(env):
    """37 distinct encryptions (two 16-row digit tiles and 5) and their keyswitch by the oracle"""
    if not hasattr(env, "ks_base"):
        r = env.ok.rng(4242)
        cts = np.stack([env.ok.encrypt(r, i % 16) for i in range(37)])
        ref = env.ok.keyswitch_batch(cts)
        cts.setflags(write=False)
        ref.setflags(write=False)
        env.ks_base = (cts, ref)
    return env.ks_base


def test_keyswitch_words_equal_oracle(env):
    ctx, n = env.ctx, env.n
    base, ref = _base(env)
    assert ref.shape == (37, n + 1)
    try:
        for name, kind in KS:
            ctx.set_ks_kernel(kind)
            for count in KS_COUNTS[n]:
                got = ctx.keyswitch(np.resize(base, (count, 2049)))
                _assert_words(got, np.resize(ref, (count, n + 1)), f"n {n}: {name} keyswitch of {count}")
            if n in (15, 2048):  # the rounding bit and every digit carry chain at their edges
                rows = ks_ref.edge_rows()
                by_oracle = env.ok.keyswitch_batch(rows)
                assert not by_oracle[3][:n].any() and by_oracle[3][n] == rows[3][2048]
                _assert_words(ctx.keyswitch(rows), by_oracle, f"n {n}: {name} keyswitch of the edge rows")
                mixed = np.concatenate([base[:7], rows, base[7:20]])
                _assert_words(ctx.keyswitch(mixed), np.concatenate([ref[:7], by_oracle, ref[7:20]]),
                              f"n {n}: {name} keyswitch, edge rows in a tile")
    finally:
        ctx.set_ks_kernel(1)


def test_lincomb_prologue_words(env):
    """k_ks_digits<true> / k_keyswitch<true>: one inline item (6 terms) and one wide item (7 terms,
    int64 coefficients) of tests/test_keyswitch_gpu.py, keyswitched to n + 1 words"""
    ctx, ok = env.ctx, env.ok
    pool = _pool(ok)
    items = _items(ok.delta())[3:5]
    assert [len(t) for t, _ in items] == [6, 7]
    comb = np.stack([ks_ref.lincomb_np(pool, t, c) for t, c in items])
    ref = ok.keyswitch_batch(comb)
    ident = ctx.lut(list(range(16)))
    try:
        for name, kind in KS:
            ctx.set_ks_kernel(kind)
            small, out = ctx.pbs_lincomb(pool, items, ident, want_small=True, want_out=False)
            assert out is None
            _assert_words(small, ref, f"n {env.n}: {name} keyswitch of an inline and a wide item")
    finally:
        ctx.set_ks_kernel(1)


# ---------------------------------------------------------------- bootstrapped words
BATCHES = (1, 2, 3, 5, 37)  # the pair (qy2) and quad (8-wave form) residues


def _pbs_case(ok, distinct):
    """`distinct` encryptions of i % 16 through LUT i % 5 and their bootstraps by the oracle"""
    tables = _luts()
    r = ok.rng(777)
    cts = np.stack([ok.encrypt(r, i % 16) for i in range(distinct)])
    lut_of = np.arange(distinct, dtype=np.uint32) % len(tables)
    ref = ok.pbs_batch(cts, np.stack([ok.make_lut(t) for t in tables]), lut_of)
    want = [tables[int(lut_of[i])][i % 16] for i in range(distinct)]
    assert [ok.decrypt(o) for o in ref] == want  # the reference itself computes f(m) at this n
    return tables, cts, lut_of, ref, want


def _paths(g):
    """(name, wide threshold, blind-rotate kind): the latency kernel, qy, and for classic qy2 and its
    8-wave form"""
    paths = [("latency", 1 << 30, 7), ("qy", 0, 4)]
    return paths + ([("qy2", 0, 5), ("qy4", 0, 6)] if g == CLASSIC else [])


def _check_pbs(ctx, ok, g, case, batches, what):
    tables, cts, lut_of, ref, want = case
    ids = np.array([ctx.lut(t) for t in tables], np.uint32)
    try:
        for name, threshold, kind in _paths(g):
            ctx.set_wide_threshold(threshold)
            ctx.set_br_kernel(kind)
            for b in batches:
                out = ctx.pbs(np.resize(cts, (b, 2049)), ids[np.resize(lut_of, b)])
                _assert_words(out, np.resize(ref, (b, 2049)), f"{what}: {name}, batch of {b}")
                assert [ok.decrypt(o) for o in out] == [want[i % len(want)] for i in range(b)]
    finally:
        ctx.set_wide_threshold(256)
        ctx.set_br_kernel(7)


def test_bootstrapped_words_every_path(env):
    """37 distinct ciphertexts below n = 833; from there 12, tiled (the oracle's bootstraps are the cost)"""
    distinct = 12 if env.n >= 833 else 37
    _check_pbs(env.ctx, env.ok, env.g, _pbs_case(env.ok, distinct), BATCHES, f"n {env.n}")


# ---------------------------------------------------------------- the radix layer at n = 16
@pytest.mark.parametrize("g", [CLASSIC, MULTIBIT], ids=["cl", "mb"])
def test_radix_layer_at_n16(g):
    """decrypt-level: FheUint32 add, mul and >> by an encrypted amount, and a 2 x 2-limb BigUintFHE
    compat mul (src/biguint.rs:194-265), on a key with n = 16"""
    ck, sk, _ = _keys(16, g)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    try:
        rng = random.Random(16 + g)
        x, y, s = rng.getrandbits(32), rng.getrandbits(32), rng.randrange(1, 32)
        a, b = FheUint32.try_encrypt(x, ck), FheUint32.try_encrypt(y, ck)
        assert (a + b).decrypt(ck) == (x + y) % 2**32
        assert (a * b).decrypt(ck) == (x * y) % 2**32
        assert (a >> FheUint32.try_encrypt(s, ck)).decrypt(ck) == x >> s
        al, bl = [rng.getrandbits(32) | 1 << 31 for _ in range(2)], [rng.getrandbits(32) | 1 << 31 for _ in range(2)]
        got = BigUintFHE.new(R.from_limbs(al), ck).mul(BigUintFHE.new(R.from_limbs(bl), ck), COMPAT).decrypt_limbs(ck)
        assert got == R.biguint_mul(al, bl)
    finally:
        set_server_key(None)
        ctx.close()


# ---------------------------------------------------------------- dense small sweep
def test_dense_sweep_small_dimensions():
    """n = 1 .. 33 classic and every even n of that range multi-bit, on one context re-keyed 49 times:
    every residue of the row stride mod 8 and both tile boundaries (16, 32) of the matrix-core
    keyswitch; per n the keyswitch words of both kernels at 1 and 17 ciphertexts and 3 bootstraps on
    the latency kernel.  Measured wall time on an MI355X: 0.8 s (the test prints it)."""
    t0 = time.perf_counter()
    ctx = Context(0)
    tables = _luts()[:3]
    try:
        for g in (CLASSIC, MULTIBIT):
            for n in range(g, 34, g):
                ck, sk = generate_keys(product_params(n, g), seed=SEED + n)
                ok = oracle.OracleKeys(SEED + n, oracle_params(n, g))
                ctx.set_server_key(sk)
                r = ok.rng(n)
                cts = np.stack([ok.encrypt(r, (3 * i + n) % 16) for i in range(17)])
                ref = ok.keyswitch_batch(cts)
                for name, kind in KS:
                    ctx.set_ks_kernel(kind)
                    for count in (17, 1):
                        _assert_words(ctx.keyswitch(cts[:count]), ref[:count], f"n {n} g {g}: {name} keyswitch of {count}")
                ctx.set_ks_kernel(1)
                ids = np.array([ctx.lut(t) for t in tables], np.uint32)
                lut_of = np.arange(3, dtype=np.uint32)
                want = ok.pbs_batch(cts[:3], np.stack([ok.make_lut(t) for t in tables]), lut_of)
                out = ctx.pbs(cts[:3], ids[lut_of])
                _assert_words(out, want, f"n {n} g {g}: 3 bootstraps")
                assert [ok.decrypt(o) for o in out] == [tables[i][(3 * i + n) % 16] for i in range(3)]
    finally:
        ctx.set_ks_kernel(1)
        ctx.close()
    print(f"dense sweep: {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- re-keying one context
def _rekey_checks(ctx, ok, ids, tables, ks_count, pbs_count, what):
    """keyswitch words of `ks_count` ciphertexts on both kernels and `pbs_count` bootstraps through the
    LUT ids registered BEFORE this key was installed, against the oracle under this key"""
    n = ok.params.n
    r = ok.rng(99)
    base = np.stack([ok.encrypt(r, i % 16) for i in range(min(ks_count, 12))])
    ks_want = ok.keyswitch_batch(base)
    try:
        for name, kind in KS:
            ctx.set_ks_kernel(kind)
            got = ctx.keyswitch(np.resize(base, (ks_count, 2049)))
            _assert_words(got, np.resize(ks_want, (ks_count, n + 1)), f"{what}: {name} keyswitch of {ks_count}")
    finally:
        ctx.set_ks_kernel(1)
    d = min(pbs_count, 12)
    lut_of = np.arange(d, dtype=np.uint32) % len(tables)
    want = ok.pbs_batch(base[:d], np.stack([ok.make_lut(t) for t in tables]), lut_of)
    out = ctx.pbs(np.resize(base[:d], (pbs_count, 2049)), ids[np.resize(lut_of, pbs_count)])
    _assert_words(out, np.resize(want, (pbs_count, 2049)), f"{what}: {pbs_count} bootstraps")
    assert [ok.decrypt(o) for o in out[:d]] == [tables[int(lut_of[i])][i % 16] for i in range(d)]
    return out


def test_rekey_between_dimensions():
    """One context through n = 16 -> 834 -> 2048 -> 16.  The d_ms workspace's row stride follows n
    (fhe_ctx::adopt_key_params drops it at every install): a stride of 24 kept for n = 834 would
    overlap the keyswitch's rows of 835 words.  The LUT tables survive a re-key that leaves the message
    space and delta unchanged -- ids registered under the first key bootstrap under every later one,
    and registering a table again returns its id -- and are dropped when the message space changes:
    an old id beyond the new table count is FHE_ERR_INVALID, and registering works again."""
    tables = _luts()
    ctx = Context(0)
    try:
        _, sk16, ok16 = _keys(16, CLASSIC)
        ctx.set_server_key(sk16)
        ids = np.array([ctx.lut(t) for t in tables], np.uint32)
        first = _rekey_checks(ctx, ok16, ids, tables, 300, 300, "n 16")  # d_ms: 300 rows at stride 24
        _, sk834 = generate_keys(seed=SEED)
        ctx.set_server_key(sk834)
        _rekey_checks(ctx, oracle.OracleKeys(SEED), ids, tables, 300, 37, "n 16 -> 834")
        _, sk2048, ok2048 = _keys(2048, CLASSIC)
        ctx.set_server_key(sk2048)
        _rekey_checks(ctx, ok2048, ids, tables, 8, 8, "n 834 -> 2048")
        ctx.set_server_key(sk16)
        again = _rekey_checks(ctx, ok16, ids, tables, 300, 300, "n 2048 -> 16")
        assert np.array_equal(first, again)
        assert [ctx.lut(t) for t in tables] == list(ids)
        # another message space (2 bits: message 2, carry 2): the tables are dropped
        p = product_params(16)
        p.message_modulus = p.carry_modulus = 2
        ck4, sk4 = generate_keys(p, seed=SEED)
        ctx.set_server_key(sk4)
        cts = np.stack([ck4.encrypt_block(m) for m in range(4)])
        with pytest.raises(FheError) as e:
            ctx.pbs(cts, int(ids[1]))
        assert e.value.code == -1  # FHE_ERR_INVALID: no table registered under this key yet
        inc = [(m + 1) % 4 for m in range(4)]
        lid = ctx.lut(inc)
        assert lid == 0
        with pytest.raises(FheError) as e:
            ctx.pbs(cts, int(ids[1]))
        assert e.value.code == -1
        assert [ck4.decrypt_block(o) for o in ctx.pbs(cts, lid)] == inc
    finally:
        ctx.close()


def _attach_replay(ctx, rank, log):
    """Test transport (fhe_ctx_attach_test_transport) of a two-rank world whose ranks run one after the
    other in this process: the root's broadcasts are recorded in `log`, the receiver's are served from
    it in order; the one-byte agreements see only the live rank (its own value is the minimum).
    Returns what must stay referenced while attached."""
    def bcast(user, host, nbytes, root):
        try:
            if rank == root:
                log.append(C.string_at(host, nbytes))
            else:
                data = log.pop(0)
                if len(data) != nbytes:
                    return 1
                C.memmove(host, data, nbytes)
            return 0
        except Exception:  # noqa: BLE001 -- reported to the engine as a failed collective
            return 1

    cbs = (_lib.TX_BCAST(bcast), _lib.TX_ALLGATHER(lambda user, host, seg: 1), _lib.TX_MIN_U8(lambda user, host, n: 0))
    tx = _lib.TestTransport(None, *cbs)
    _lib.check(_lib.load().fhe_ctx_attach_test_transport(ctx.handle, C.byref(tx), 2, rank))
    return tx, cbs


def test_rekey_through_broadcast_install():
    """the other key-install path: a context that RECEIVES its keys (fhe_ctx_broadcast_server_key,
    ranks != root) first at n = 16, then at n = 834, with 300 bootstraps in between sizing d_ms at
    stride 24 -- the same checks as above, the LUT ids of the first key kept"""
    tables = _luts()
    root, recv = Context(0), Context(0)
    try:
        ids = None
        steps = [(_keys(16, CLASSIC)[1], _keys(16, CLASSIC)[2], 300, "received n 16"),
                 (generate_keys(seed=SEED)[1], oracle.OracleKeys(SEED), 37, "received n 16 -> 834")]
        for sk, ok, pbs_count, what in steps:
            log = []
            root.set_server_key(sk)
            keep = _attach_replay(root, 0, log)
            root.broadcast_server_key(0)
            root.detach_comm()
            assert len(log) == 3  # header, KSK, Fourier BSK
            keep = _attach_replay(recv, 1, log)
            recv.broadcast_server_key(0)
            recv.detach_comm()
            del keep
            assert not log and recv.params.lwe_dimension == ok.params.n
            if ids is None:
                ids = np.array([recv.lut(t) for t in tables], np.uint32)
            _rekey_checks(recv, ok, ids, tables, 300, pbs_count, what)
    finally:
        root.close()
        recv.close()


def _broadcast_log(sk):
    """what a root holding `sk` sends: header, KSK, Fourier BSK"""
    log = []
    root = Context(0)
    try:
        root.set_server_key(sk)
        keep = _attach_replay(root, 0, log)
        root.broadcast_server_key(0)
        root.detach_comm()
        del keep
    finally:
        root.close()
    assert len(log) == 3
    return log


def test_broadcast_install_drops_the_receivers_dependants():
    """a receiver that holds a compression key, a public key and a re-keying key: the received server key
    drops all three, as a direct install does (fhe_ctx::adopt_key_params) -- their entry points answer
    FHE_ERR_NO_KEY -- and bootstraps under the received key are the oracle's words"""
    from fhe_sign import CompactPublicKey, CompressionKeys, CompressionParams, RekeyKey
    import compress_ref

    tables = _luts()
    ck, sk, ok = _keys(16, CLASSIC)
    cp = compress_ref.SMALL_A
    recv = Context(0)
    try:
        recv.set_server_key(sk)
        recv.set_compression_key(CompressionKeys.generate(ck, CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12))[1])
        recv.set_public_key(CompactPublicKey.new(ck))
        recv.set_rekey_key(RekeyKey.new(ck, generate_keys(product_params(15), seed=SEED)[0], bytes(range(9, 41))))
        set_server_key(recv)
        x = FheUint32.try_encrypt(7, ck)
        dependants = (x.compress, lambda: x.re_randomize(bytes(range(3, 35))), lambda: x.compress_switched(rekey=True))
        for call in dependants:
            call()  # installed: each one runs
        log = _broadcast_log(sk)
        keep = _attach_replay(recv, 1, log)
        recv.broadcast_server_key(0)
        recv.detach_comm()
        del keep
        assert not log
        for call in dependants:
            with pytest.raises(FheError) as e:
                call()
            assert e.value.code == -3  # FHE_ERR_NO_KEY
        del x
        ids = np.array([recv.lut(t) for t in tables], np.uint32)
        _rekey_checks(recv, ok, ids, tables, 8, 8, "received over dependants")
    finally:
        set_server_key(None)
        recv.close()


def test_failed_broadcast_leaves_the_installed_key():
    """the root's last message (the Fourier BSK) never arrives: the transport reports a failed collective,
    broadcast_server_key raises, and the receiver's installed key, its row space (sized by 300 bootstraps) and
    its lookup tables are what they were -- the same words, the same ids.  The key on the wire is another one
    of the same parameters, so a half-installed key would show as different words."""
    tables = _luts()
    _, sk, ok = _keys(16, CLASSIC)
    recv = Context(0)
    try:
        recv.set_server_key(sk)
        ids = np.array([recv.lut(t) for t in tables], np.uint32)
        before = _rekey_checks(recv, ok, ids, tables, 300, 300, "installed key")
        log = _broadcast_log(generate_keys(product_params(16), seed=SEED + 1)[1])
        log.pop()
        keep = _attach_replay(recv, 1, log)
        with pytest.raises(FheError):
            recv.broadcast_server_key(0)
        recv.detach_comm()
        del keep
        after = _rekey_checks(recv, ok, ids, tables, 8, 8, "installed key after a failed broadcast")
        assert np.array_equal(after, before[:8])
        assert [recv.lut(t) for t in tables] == list(ids)
    finally:
        recv.close()
