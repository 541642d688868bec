"""The blind-rotate kernels against exact integer arithmetic (tests/exact_pbs_ref.py), without the oracle.

Every other GPU test pins ciphertext words to oracle/tfhe_oracle.c, whose f64 arithmetic was chosen with
the kernels; tests/test_exact_pbs.py holds that oracle to the exact reference on the CPU, and this file
holds the kernels to it directly, through keys and secrets exported from the product (ClientKey.export,
ServerKey.export) and the caps the CPU file established (tests/exact_pbs_sets.py):

  sharp tier       n = 1 classic, n = 2 multi-bit: one update of an exactly representable accumulator, so
                   each of the 2049 output words of 37 ciphertexts (a ragged count: the two-per-workgroup
                   kernels run a half-empty pair) is within WORD_CAP of the exact word and below the 2^46
                   tfhe_oracle.c claims -- on the latency kernel and kinds 4, 5, 6, 7, 9 (classic), the
                   latency kernel and kind 4 (multi-bit), and for one descriptor batch of fused linear
                   combinations (4, 2, 1, 1) + constant, combined exactly in u64 on the host
  multi-step tier  n = 2, 3 classic, n = 4 multi-bit, 64 ciphertexts: decode, R and the worst
                   |kernel - exact| phase in exact sigmas, on the latency kernel and the default
                   throughput selection

The inputs are the CPU file's (same key seed, same encryption stream, word-identical), so the figures
printed here are the oracle's wherever the words are."""
import numpy as np
import pytest

import exact_pbs_ref as X
import exact_pbs_sets as S
import ks_ref
from exact_pbs_sets import CLASSIC, MULTIBIT, N
from fhe_sign import Context, generate_keys
from lwe_dims import product_params

pytestmark = pytest.mark.gpu
DELTA = 1 << 59
SHARP_COUNT = 37
LATENCY = ("latency", 1 << 30, 7)
AUTO = ("auto", 0, 7)


def _paths(grouping):
    """(name, wide threshold, blind-rotate kind)"""
    if grouping == MULTIBIT:
        return [LATENCY, ("qy", 0, 4)]
    return [LATENCY, ("qy", 0, 4), ("qy2", 0, 5), ("qy4", 0, 6), AUTO, ("qz", 0, 9)]


class Env:
    def __init__(self, n, g, count):
        self.n, self.g = n, g
        ck, sk = generate_keys(product_params(n, g), seed=S.KEY_SEED)
        self.lwe_sk, self.glwe_sk = ck.export()
        self.ksk, self.bsk = sk.export()
        ck.seed_encryption(S.SEEDS[0], 100)
        self.cts = ck.encrypt_blocks(S.messages(count))
        self.luts = np.stack([X.lut_poly(S.table_of(i), N) for i in range(count)])
        self.ctx = Context(0)
        self.ctx.set_server_key(sk)
        self.ids = np.array([self.ctx.lut(t) for t in S.TABLES], np.uint32)
        self.lut_ids = self.ids[np.arange(count) % len(S.TABLES)]

    def exact(self, cts):
        """(smalls, accumulators, outputs) of the exact bootstrap of `cts`, row i through table i % 3"""
        return X.bootstrap_batch(self.ksk, self.bsk, self.n, cts, self.luts[:len(cts)], self.g)

    def run(self, path, fn):
        _, threshold, kind = path
        try:
            self.ctx.set_wide_threshold(threshold)
            self.ctx.set_br_kernel(kind)
            return fn()
        finally:
            self.ctx.set_wide_threshold(256)
            self.ctx.set_br_kernel(7)


def _assert_words_near(got, exact, s, what):
    assert got.shape == exact.shape
    with np.errstate(over="ignore"):
        diff = np.abs(X.signed(got - exact))
    worst = int(diff.max())
    print(f"\n{what}: |kernel - exact| over {diff.size} words: max 2^{S.log2(worst):.2f}, rms 2^{S.log2(S.rms(diff)):.2f}; "
          f"cap 2^{S.log2(S.WORD_CAP[s]):.2f}")
    i, j = (int(v) for v in np.unravel_index(int(diff.argmax()), diff.shape))
    assert worst < S.WORD_CLAIM, f"{what}: ciphertext {i}, word {j}: {int(got[i, j]):#018x} against {int(exact[i, j]):#018x}"
    assert worst <= S.WORD_CAP[s], f"{what}: ciphertext {i}, word {j}: {int(got[i, j]):#018x} against {int(exact[i, j]):#018x}"


# ---------------------------------------------------------------- sharp tier
@pytest.fixture(scope="module", params=S.SHARP_SETS, ids=S.set_id)
def sharp(request):
    e = Env(*request.param, SHARP_COUNT)
    e.exact_out = e.exact(e.cts)[2]
    e.exact_out.setflags(write=False)
    yield e
    e.ctx.close()


def test_sharp_words_every_path(sharp):
    e = sharp
    for path in _paths(e.g):
        got = e.run(path, lambda: e.ctx.pbs(e.cts, e.lut_ids))
        _assert_words_near(got, e.exact_out, (e.n, e.g), f"sharp {S.set_id((e.n, e.g))}, {path[0]}")


def test_sharp_words_descriptor_batch(sharp):
    """item i = 4 ct[i] + 2 ct[i + 1] + ct[i + 2] + ct[i + 5] + constant (indices mod 37): the fused linear
    prologue in front of the same single update; the combination itself is exact u64 arithmetic"""
    e = sharp
    items = [([(i, 4), ((i + 1) % SHARP_COUNT, 2), ((i + 2) % SHARP_COUNT, 1), ((i + 5) % SHARP_COUNT, 1)],
              ((3 * i + 1) << 55) + i) for i in range(SHARP_COUNT)]
    comb = np.stack([ks_ref.lincomb_np(e.cts, t, c) for t, c in items])
    smalls, _, exact_out = e.exact(comb)
    for path in (LATENCY, AUTO):
        small, out = e.run(path, lambda: e.ctx.pbs_lincomb(e.cts, items, e.lut_ids))
        assert np.array_equal(small, smalls)  # integer on both sides
        _assert_words_near(out, exact_out, (e.n, e.g), f"sharp {S.set_id((e.n, e.g))}, descriptors, {path[0]}")


# ---------------------------------------------------------------- multi-step tier
GPU_MULTI_SETS = ((2, CLASSIC), (3, CLASSIC), (4, MULTIBIT))


@pytest.fixture(scope="module", params=GPU_MULTI_SETS, ids=S.set_id)
def multi(request):
    """the ideal output phases and the exact path's errors against them, once per set"""
    assert S.MULTI_SETS[request.param] == 64
    e = Env(*request.param, 64)
    smalls, _, out = e.exact(e.cts)
    e.ideal = np.array([X.ideal_rotation(s, e.lwe_sk, l)[0] for s, l in zip(smalls, e.luts)])
    with np.errstate(over="ignore"):
        e.err_exact = X.signed(X.lwe_phase(out, e.glwe_sk) - e.ideal)
    yield e
    e.ctx.close()


@pytest.mark.parametrize("path", [LATENCY, AUTO], ids=lambda p: p[0])
def test_multi_step_phase_within_caps(multi, path):
    e = multi
    s = (e.n, e.g)
    ideal, err_exact = e.ideal, e.err_exact
    got = e.run(path, lambda: e.ctx.pbs(e.cts, e.lut_ids))
    with np.errstate(over="ignore"):
        phase = X.lwe_phase(got, e.glwe_sk)
        se, sf, ratio, worst = S.phase_figures(err_exact, X.signed(phase - ideal))
    print(f"\nmulti-step {S.set_id(s)}, {path[0]}: phase error rms exact 2^{S.log2(se):.2f}, kernel 2^{S.log2(sf):.2f}, "
          f"R = {ratio:.4f} (cap {S.RATIO_CAP[s]:.3f}), worst |kernel - exact| = {worst:.4f} sigma (cap {S.DIFF_CAP[s]:.3f})")
    want = [S.table_of(i)[m] for i, m in enumerate(S.messages(64))]
    assert [((int(p) + DELTA // 2) // DELTA) % 32 for p in phase] == want
    assert ratio <= S.RATIO_CAP[s]
    assert worst <= S.DIFF_CAP[s]
