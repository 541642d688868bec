"""k_blind_rotate_qz (FHE_BR_QZ = 9; br_qy.hip: two ciphertexts per workgroup, one wave per polynomial in
the transform phases, no lane transposes) word for word against k_blind_rotate_qy (kind 4) and the oracle:
the pair residues and the run-twice-store-once case of an odd batch, the LWE dimensions at which the
mask prefetch clamps onto the body, a single CMUX runs, and an odd n ends on an unreduced update, the
descriptor path, and the kernel FHE_BR_AUTO picks at 3072 bootstraps.  Exact equality of 64-bit words."""
import numpy as np
import pytest

import ks_ref
import oracle
from fhe_sign import Context, generate_keys
from lwe_dims import CLASSIC, oracle_params, product_params
from test_keyswitch_gpu import _assert_words, _lincomb_reference, _radix_items
from test_lwe_dims_gpu import _pbs_case
from test_pbs_gpu import _luts

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
QY, AUTO, QZ = 4, 7, 9


@pytest.fixture(scope="module")
def env():
    """classic keys at the default n = 834"""
    ck, sk = generate_keys(seed=SEED)
    ok = oracle.OracleKeys(SEED)
    ctx = Context(0)
    ctx.set_server_key(sk)
    yield ck, ok, ctx
    ctx.close()


def test_pair_residues_equal_qy_and_oracle(env):
    """batches 1, 2, 3, 5, 6, 258, 515 with every LUT: an odd batch runs its last ciphertext in both pair
    slots and stores it once; 258 and 515 span more than one round of workgroups per CU pair slot"""
    _, ok, ctx = env
    tables = _luts()
    ids = np.array([ctx.lut(t) for t in tables], np.uint32)
    r = ok.rng(991)
    cts = np.stack([ok.encrypt(r, (3 * i + 1) % 16) for i in range(515)])
    lut_of = (np.arange(515) % len(tables)).astype(np.uint32)
    rows = np.array([0, 1, 2, 514])
    ref = ok.pbs_batch(np.ascontiguousarray(cts[rows]), np.stack([ok.make_lut(t) for t in tables]), lut_of[rows])
    batches = (1, 2, 3, 5, 6, 258, 515)
    got = {}
    try:
        ctx.set_wide_threshold(0)
        for kind in (QY, QZ):
            ctx.set_br_kernel(kind)
            got[kind] = {b: ctx.pbs(cts[:b], ids[lut_of[:b]]) for b in batches}
    finally:
        ctx.set_wide_threshold(256)
        ctx.set_br_kernel(AUTO)
    for b in batches:
        _assert_words(got[QZ][b], got[QY][b], f"kind 9 against kind 4, batch of {b}")
    _assert_words(got[QZ][515][rows], ref, "kind 9, rows 0, 1, 2, 514 of 515 against the oracle")
    _assert_words(got[QZ][3], ref[:3], "kind 9, batch of 3 against the oracle")


@pytest.mark.parametrize("n", [1, 2, 15, 16, 833])
def test_small_and_odd_dimensions_equal_oracle(n):
    """n = 1: one CMUX, the prefetch of mask words 1 and 2 clamps onto the body; 2: no deferred reduction
    is ever consumed; 15, 833: odd n, the epilogue converts an unreduced accumulator; 16: even"""
    ck, sk = generate_keys(product_params(n, CLASSIC), seed=SEED)
    ok = oracle.OracleKeys(SEED, oracle_params(n, CLASSIC))
    ctx = Context(0)
    ctx.set_server_key(sk)
    try:
        tables, cts, lut_of, ref, want = _pbs_case(ok, 5)
        ids = np.array([ctx.lut(t) for t in tables], np.uint32)
        ctx.set_wide_threshold(0)
        ctx.set_br_kernel(QZ)
        for b in (1, 2, 3, 5):
            out = ctx.pbs(cts[:b], ids[lut_of[:b]])
            _assert_words(out, ref[:b], f"n {n}: kind 9, batch of {b}")
            assert [ok.decrypt(o) for o in out] == want[:b]
    finally:
        ctx.close()


def test_descriptor_path_equals_oracle(env):
    """the fused linear-combination PBS of test_keyswitch_gpu.py::test_lincomb_pbs_words (prologue,
    keyswitch, blind rotate writing through desc.dst; 45 items, an odd count) on kind 9"""
    _, ok, ctx = env
    tables = _luts() + [[1 if v >= 8 else 0 for v in range(16)]]
    ids = [ctx.lut(t) for t in tables]
    pool, items, comb, small_ref = _lincomb_reference(ok, 37)
    unit, ritems, msgs = _radix_items(ok, ctx)
    blocks = np.concatenate([pool, unit])
    items = items + [([(40 + s, k) for s, k in t], c) for t, c in ritems]
    lut_of = np.array([i % 5 for i in range(37)] + [5] * 8, np.uint32)
    comb = np.concatenate([comb, np.stack([ks_ref.lincomb_np(unit, t, c) for t, c in ritems])])
    ref = ok.pbs_batch(comb, np.stack([ok.make_lut(t) for t in tables]), lut_of)
    try:
        ctx.set_wide_threshold(0)
        ctx.set_br_kernel(QZ)
        small, out = ctx.pbs_lincomb(blocks, items, [ids[k] for k in lut_of])
    finally:
        ctx.set_wide_threshold(256)
        ctx.set_br_kernel(AUTO)
    _assert_words(small[:37], small_ref, "kind 9: keyswitched words")
    _assert_words(out, ref, "kind 9: bootstrapped words")
    assert [ok.decrypt(o) for o in out[37:]] == [int(m >= 8) for m in msgs]


def test_auto_at_3072_equals_qy(env):
    """whatever kernel FHE_BR_AUTO launches for a level of 3072 bootstraps gives kind 4's words"""
    ck, _, ctx = env
    B = 3072
    ck.seed_encryption(23)
    cts = ck.encrypt_blocks(np.arange(B) % 16)
    inc = ctx.lut([(m + 1) % 16 for m in range(16)])
    try:
        auto = ctx.pbs(cts, inc)
        ctx.set_br_kernel(QY)
        qy = ctx.pbs(cts, inc)
    finally:
        ctx.set_br_kernel(AUTO)
    _assert_words(auto, qy, "FHE_BR_AUTO against kind 4 at 3072")
    assert [ck.decrypt_block(auto[i]) for i in range(0, B, 97)] == [(i % 16 + 1) % 16 for i in range(0, B, 97)]
