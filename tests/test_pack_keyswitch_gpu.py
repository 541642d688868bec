"""The packing keyswitch's matrix-core contraction (csrc/compress.hip k_pk_digits + k_pk_mfma) on the GPU,
WORD FOR WORD: every 64-bit word P[row][column] = sum_{j, l} d[row, j, l] PKSK[j][l] mod 2^64 through the test
hook fhe_pack_keyswitch_words, against tests/compress_ref.py's digits + contract (exact: float64 limb sums
below 2^53), and the installed byte planes against a numpy restatement of their layout.

Why the words and not the stored bytes: k_pk_pack keeps the top 12 bits of a sum of up to 256 such words, and
tests/test_compress.py test_stored_bytes_cannot_see_the_low_planes shows that the compressed list does not
change when the low 16 bits of every key word do.  An error in byte planes 0-2, in their << 8 b recombination or
in the balanced-byte carries of k_pksk_to_planes is invisible to every byte comparison of the compressed list;
here it changes a compared word.

Inputs: uniform random 64-bit rows from a fixed seed (they need not be encryptions), the digit edge rows
(compress_ref.edge_rows) as the first four rows and, from 8 rows on, as the last four.  A row's words depend on
that row alone, so the reference is computed once per parameter set, over the pool of rows, and every count's
expectation is a selection of its rows.

What each count reaches (launch_pack_keyswitch: k_pk_mfma<1>, 64 rows per workgroup, below 2048 rows;
k_pk_mfma<4>, 256 rows per workgroup, from 2048 on):
  1, 16, 17       one row; a full 16-row tile; one row in the next tile
  64, 65          a full 4-wave workgroup; one row in the next workgroup
  2048            RW = 4, every workgroup full
  2049            one row in a ninth workgroup
  2367            the last workgroup: wave 0 has three tiles and 15 rows, waves 1-3 lie past `count` and read
                  digit fragments no kernel wrote (their words must not be stored anywhere)
Parameter sets: the defaults; (1, 8, 8, 4, 4) one column tile; (2, 16, 16, 3, 5) ell = 5, KT = 160, 3-bit
digits; (2, 8, 5, 7, 4) 24 columns = a padded column tile, 7-bit digits -64 .. 63."""
import ctypes as C

import numpy as np
import pytest

import compress_ref as R
import seeded_compression_ref as SC
from fhe_sign import CompressionKeys, CompressionParams, Context, default_params, generate_keys, set_server_key
from fhe_sign._lib import FheError, load
from lwe_dims import product_params

pytestmark = pytest.mark.gpu
SEED = 0x5EEDC0DE
ROW_SEED = 0x9A11E7
NO_KEY, INVALID = -3, -1
SETS = [R.DEFAULT, R.SMALL_A, R.SMALL_B, SC.MIXED]
SMALL_COUNTS = {R.DEFAULT: [1, 16, 17, 64, 65]}
LARGE_COUNTS = {R.DEFAULT: [2048, 2049, 2367]}


def small_counts(cp):
    return SMALL_COUNTS.get(cp, [1, 17, 65])


def large_counts(cp):
    return LARGE_COUNTS.get(cp, [2049])


def set_id(cp):
    return f"k{cp.k}N{cp.N}L{cp.L}b{cp.beta}l{cp.ell}"


class Env:
    """one context per parameter set, the main key of LWE dimension k' N' at the small sets (as
    tests/test_compress_gpu.py builds them), and the reference words of the row pool"""

    def __init__(self, cp):
        self.cp = cp
        params = default_params() if cp is R.DEFAULT else product_params(cp.k * cp.N)
        self.ck, self.sk = generate_keys(params, seed=SEED)
        self.priv, self.key = CompressionKeys.generate(self.ck, CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12))
        self.pksk = self.key.export()[0]
        self.ctx = Context(0)
        self.ctx.set_server_key(self.sk)
        self.ctx.set_compression_key(self.key)
        self.edges = R.edge_rows(cp.beta, cp.ell)
        self.pool = np.random.default_rng(ROW_SEED + cp.N).integers(0, 1 << 64, (max(large_counts(cp)), R.BIG_CT), dtype=np.uint64)
        self.ref_pool = R.contraction_words(cp, self.pksk, self.pool)
        self.ref_edges = R.contraction_words(cp, self.pksk, self.edges)

    def close(self):
        set_server_key(None)
        self.ctx.close()

    def rows(self, count):
        """(the input rows, their reference words): pool rows 0 .. count - 1 with the edge rows over the first
        four and, from 8 rows on, over the last four"""
        cts, ref = self.pool[:count].copy(), self.ref_pool[:count].copy()
        head = min(4, count)
        cts[:head], ref[:head] = self.edges[:head], self.ref_edges[:head]
        if count >= 8:
            cts[count - 4:], ref[count - 4:] = self.edges, self.ref_edges
        return cts, ref


_envs = {}


def _env(cp):
    if cp not in _envs:
        _envs[cp] = Env(cp)
    return _envs[cp]


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for e in _envs.values():
        e.close()
    _envs.clear()


@pytest.fixture(scope="module", params=SETS, ids=set_id)
def env(request):
    return _env(request.param)


@pytest.fixture(scope="module")
def dflt():
    return _env(R.DEFAULT)


@pytest.fixture(scope="module", params=SETS[1:], ids=set_id)
def small(request):
    return _env(request.param)


def _assert_words(got, want, what):
    """equality of every word; the first difference named by row, column and lowest differing byte plane"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, what
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    r, c = (int(x) for x in bad[0])
    x = int(got[r, c]) ^ int(want[r, c])
    plane = ((x & -x).bit_length() - 1) // 8
    raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ ({len(set(bad[:, 0]))} rows); first at row {r}, "
                         f"column {c}: got {int(got[r, c]):#018x}, want {int(want[r, c]):#018x}, lowest differing byte plane {plane}")


def _check(env, count, what=""):
    cts, ref = env.rows(count)
    P, body = env.ctx.pack_keyswitch_words(cts)
    _assert_words(P, ref, f"{set_id(env.cp)} count {count}{what}")
    assert np.array_equal(body, cts[:, R.N_BIG]), f"{set_id(env.cp)} count {count}{what}: bodies"
    return P


# ------------------------------------------------------------------ the installed key
def test_byte_planes_are_the_layout_restated_in_numpy(env):
    """fhe_set_compression_key's k_pksk_to_planes against compress_ref.plane_layout: the balanced bytes, the
    level-major k order, the lane / byte order inside a fragment, and zero bytes in the padding columns"""
    cp = env.cp
    got = env.ctx.export_compression_state()[0]
    want = R.plane_layout(cp, env.pksk)
    assert got.dtype == np.int8 and got.size == want.size == 8 * ((R.cols(cp) + 15) // 16) * 32 * cp.ell * 1024
    got = got.reshape(want.shape)
    if not np.array_equal(got, want):
        b, tt, kt, lane, jj = (int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError(f"{set_id(cp)}: {int((got != want).sum())} plane bytes differ; first at plane {b}, column tile {tt}, "
                             f"k-tile {kt}, lane {lane}, byte {jj}: got {int(got[b, tt, kt, lane, jj])}, want {int(want[b, tt, kt, lane, jj])}")
    words, padding = R.words_of_planes(cp, got)
    assert np.array_equal(words, env.pksk) and not padding.any()
    assert padding.size == 8 * cp.ell * R.N_BIG * (-R.cols(cp) % 16)


# ------------------------------------------------------------------ the words
@pytest.mark.parametrize("count", small_counts(R.DEFAULT) + large_counts(R.DEFAULT))
def test_contraction_words_at_the_defaults(dflt, count):
    _check(dflt, count)


@pytest.mark.parametrize("count", small_counts(R.SMALL_A) + large_counts(R.SMALL_A))
def test_contraction_words_at_the_small_sets(small, count):
    _check(small, count)


def test_small_large_small_on_one_context(env):
    """the counts in the order small, large, small: the workspace grows once, then the small runs reuse a digit
    buffer that holds the large run's fragments and a capacity above their count.  Every run equals the
    reference, so the repeated small runs give the words of the first ones"""
    first = {c: _check(env, c, " (first pass)") for c in small_counts(env.cp)}
    for c in large_counts(env.cp):
        _check(env, c, " (large pass)")
    for c in small_counts(env.cp):
        again = _check(env, c, " (after the large runs)")
        assert np.array_equal(again, first[c])


# ------------------------------------------------------------------ the hook's statuses
def test_refusals_of_the_hook(small):
    env, cp, lib = small, small.cp, load()
    cts, ref = env.rows(5)
    P = np.zeros((5, R.cols(cp)), np.uint64)
    body = np.zeros(5, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    p = lambda a: a.ctypes.data_as(u64p)
    h = env.ctx.handle
    # no compression key: a context with the server key alone, and one without any key
    for with_key in (True, False):
        bare = Context(0)
        try:
            if with_key:
                bare.set_server_key(env.sk)
            assert lib.fhe_pack_keyswitch_words(bare.handle, p(cts), 5, p(P), P.size, p(body)) == NO_KEY
            assert lib.fhe_pack_keyswitch_words(bare.handle, None, 0, None, 0, None) == NO_KEY
            with pytest.raises(FheError) as e:
                bare.pack_keyswitch_words(cts)
            assert e.value.code == NO_KEY
        finally:
            bare.close()
    assert lib.fhe_pack_keyswitch_words(None, p(cts), 5, p(P), P.size, p(body)) == INVALID
    # p_words one short, and each pointer null with count > 0: nothing is written
    assert lib.fhe_pack_keyswitch_words(h, p(cts), 5, p(P), P.size - 1, p(body)) == INVALID
    assert lib.fhe_pack_keyswitch_words(h, p(cts), 5, p(P), 0, p(body)) == INVALID
    assert lib.fhe_pack_keyswitch_words(h, None, 5, p(P), P.size, p(body)) == INVALID
    assert lib.fhe_pack_keyswitch_words(h, p(cts), 5, None, P.size, p(body)) == INVALID
    assert lib.fhe_pack_keyswitch_words(h, p(cts), 5, p(P), P.size, None) == INVALID
    assert not P.any() and not body.any()
    # count == 0: fine, with or without pointers
    assert lib.fhe_pack_keyswitch_words(h, None, 0, None, 0, None) == 0
    assert lib.fhe_pack_keyswitch_words(h, p(cts), 0, p(P), P.size, p(body)) == 0
    assert not P.any() and not body.any()
    got_P, got_body = env.ctx.pack_keyswitch_words(np.zeros((0, R.BIG_CT), np.uint64))
    assert got_P.shape == (0, R.cols(cp)) and got_body.shape == (0,)
    # the exact size is accepted, and the context still computes the reference
    assert lib.fhe_pack_keyswitch_words(h, p(cts), 5, p(P), P.size, p(body)) == 0
    _assert_words(P, ref, "after the refusals")
    assert np.array_equal(body, cts[:, R.N_BIG])
