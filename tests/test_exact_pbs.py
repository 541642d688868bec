"""The oracle's f64 blind rotation against exact integer arithmetic (tests/exact_pbs_ref.py), on the CPU.

Every GPU ciphertext word is pinned to oracle/tfhe_oracle.c, whose f64 operation order, tables and
unreduced-accumulator schedule were chosen together with the kernels: a loss of precision made on both
sides at once passes every word-for-word test.  Here the oracle itself is held to a reference that has
no floating point in it:

  a. the reference's own pieces against slower, plainer statements of the same thing;
  b. sharp tier -- n = 1 classic and n = 2 multi-bit are a single update of an exactly representable
     accumulator, so both sides take the same digits and all 4096 accumulator words agree to the f64
     error of one update: every word within WORD_CAP and within the 2^46 tfhe_oracle.c claims;
  c. multi-step tier -- from the second update on digits flip and the words decorrelate; what stays
     comparable is the phase.  Per set: the rms phase error of both paths against the ideal rotated
     LUT, their ratio R and the largest |f64 - exact| in exact sigmas, against the caps of
     tests/exact_pbs_sets.py, and every decode.

`PYTHONPATH=oracle python tests/test_exact_pbs.py` prints the figures of all three seeds (what the caps were set from)."""
import ctypes as C
import functools
import random
import time

import numpy as np
import pytest

import exact_pbs_ref as X
import exact_pbs_sets as S
import ks_ref
import oracle
from exact_pbs_sets import CLASSIC, MULTIBIT, N

DELTA = 1 << 59
_u64p = C.POINTER(C.c_uint64)


def _p(a):
    return a.ctypes.data_as(_u64p)


def oracle_params(n, grouping):
    p = oracle.default_params()
    p.n = n
    p.grouping = grouping
    return p


@functools.lru_cache(maxsize=2)
def keys(n, grouping):
    return oracle.OracleKeys(S.KEY_SEED, oracle_params(n, grouping))


def inputs(ok, count, seed):
    """`count` encryptions of i % 16 and the LUT polynomial of table i % 3 for each"""
    r = ok.rng(seed)
    cts = np.stack([ok.encrypt(r, m) for m in S.messages(count)])
    luts = np.stack([X.lut_poly(S.table_of(i), N) for i in range(count)])
    return cts, luts


def oracle_glwe(ok, small, lut):
    """the (2, 2048) accumulator fho_blind_rotate returns"""
    out = np.zeros(2 * N, np.uint64)
    oracle.load().fho_blind_rotate(ok.ref, _p(np.ascontiguousarray(small, np.uint64)),
                                   _p(np.ascontiguousarray(lut, np.uint64)), _p(out))
    return out.reshape(2, N)


def decode(phase):
    return ((int(phase) + DELTA // 2) // DELTA) % 32


# ---------------------------------------------------------------- a. the reference against itself
def _schoolbook(small, big):
    n = len(big)
    out = [0] * n
    for i, s in enumerate(small):
        if s:
            for j, b in enumerate(big):
                k = i + j
                if k < n:
                    out[k] += s * b
                else:
                    out[k - n] -= s * b
    return [v % (1 << 64) for v in out]


@pytest.mark.parametrize("n", [8, 64, 2048])
def test_negmul_against_bigint_schoolbook(n):
    rnd = random.Random(n)
    for _ in range(1 if n == 2048 else 8):
        small = [rnd.randint(-(1 << 22), 1 << 22) for _ in range(n)]
        big = [rnd.getrandbits(64) for _ in range(n)]
        small[0], small[1], big[0], big[1] = 1 << 22, -(1 << 22), (1 << 64) - 1, 1 << 63
        got = X.negmul(np.array(small, np.int64), np.array(big, np.uint64))
        assert [int(v) for v in got] == _schoolbook(small, big)


@pytest.mark.parametrize("n", [32, 2048])
def test_rotation_identities(n):
    rnd = random.Random(n + 1)
    p = np.array([rnd.getrandbits(64) for _ in range(n)], np.uint64)
    neg = np.uint64(0) - p
    assert np.array_equal(X.rotate(p, 0), p) and np.array_equal(X.rotate(p, n), neg)
    assert np.array_equal(X.rotate(p, 1), np.concatenate([neg[-1:], p[:-1]]))
    assert np.array_equal(X.rotate(p, 2 * n - 1), np.concatenate([p[1:], neg[:1]]))
    for r in (0, 1, n - 1, n, n + 1, 2 * n - 1):
        mono = np.zeros(n, np.int64)
        mono[r % n] = 1 if r < n else -1
        assert np.array_equal(X.rotate(p, r), X.negmul(mono, p)), r
        assert np.array_equal(X.rotate(X.rotate(p, r), (2 * n - r) % (2 * n)), p), r
        assert np.array_equal(X.rotate(X.rotate(p, r), n), np.uint64(0) - X.rotate(p, r)), r


def test_digit_tie_rule_is_the_oracles():
    """the one place where two exact definitions could differ: both roundings at their ties, the ends
    of the digit range and of the signed word, against fho_tor_digit on the same signed value"""
    lib = oracle.load()
    vals = []
    for k in (-(1 << 22), -(1 << 22) + 1, -3, -2, -1, 0, 1, 2, 3, (1 << 22) - 1):
        for low in (-(1 << 40), -(1 << 40) + 1024, 0, (1 << 40) - 1024, 1 << 40):  # g = k +- 1/2: ties to even
            vals.append((k << 41) + low)
    for q in (-1, 0):  # g = q 2^23 + 2^22: the digit tie, +2^22 on the even q, -2^22 on the odd one
        vals.append(((q << 23) + (1 << 22)) << 41)
    vals += [-(1 << 63), (1 << 63) - 1024, (1 << 62), -(1 << 62) + (1 << 40)]
    vals = [v for v in vals if -(1 << 63) <= v < (1 << 63)]
    got = X.digit(np.array([v % (1 << 64) for v in vals], np.uint64))
    for v, d in zip(vals, got):
        assert float(v) == v  # representable: the oracle sees the same value
        want = lib.fho_tor_digit(float(v), 23)
        assert want == int(want) and int(d) == int(want), (hex(v), int(d), want)
        assert -(1 << 22) <= int(d) <= 1 << 22 and (v - (int(d) << 41) + (1 << 40)) % (1 << 64) <= 1 << 41
    assert int(X.digit(np.array([1 << 63], np.uint64))[0]) == -(1 << 22)
    assert {int(d) for d in got} >= {-(1 << 22), 1 << 22}


def test_small_pieces_are_the_oracles():
    """modulus switch, LUT polynomial and sample extraction, restated here, against the oracle's"""
    lib = oracle.load()
    ok = keys(1, CLASSIC)
    edge = [0, 1, (1 << 51) - 1, 1 << 51, (1 << 51) + 1, (1 << 52) - 1, 1 << 52, (1 << 64) - 1, (1 << 64) - (1 << 51),
            (1 << 64) - (1 << 51) - 1, 1 << 63, (4095 << 52) + (1 << 51) - 1]
    rnd = random.Random(5)
    edge += [rnd.getrandbits(64) for _ in range(64)]
    assert [int(v) for v in X.modswitch(np.array(edge, np.uint64), N)] == [lib.fho_modswitch(v) for v in edge]
    assert [int(v) for v in X.modswitch(np.array([0, 1 << 58, (1 << 58) - 1, (1 << 64) - 1], np.uint64), 32)] == [0, 1, 1, 0]
    for t in S.TABLES:
        assert np.array_equal(X.lut_poly(t, N), ok.make_lut(t))
    glwe = np.array([rnd.getrandbits(64) for _ in range(2 * N)], np.uint64)
    out = np.zeros(N + 1, np.uint64)
    lib.fho_sample_extract(_p(glwe), _p(out))
    assert np.array_equal(X.sample_extract(glwe.reshape(2, N)), out)
    sk = np.array([rnd.getrandbits(1) for _ in range(N)], np.uint64)
    assert int(X.glwe_phase(glwe.reshape(2, N), sk)[0]) == int(X.lwe_phase(out, sk))


@pytest.mark.parametrize("grouping", [CLASSIC, MULTIBIT], ids=["cl", "mb"])
def test_noiseless_key_gives_the_rotated_lut(grouping):
    """N = 64, n = 4, a hand-built key whose GGSW masks and noise are zero (row r holds m 2^41 in
    polynomial r): the mask stays zero and the body is X^(-b + sum a_i s_i) LUT up to the gadget
    rounding alone, for all 16 messages.  The LUT carries low bits so that the rounding is there: with
    acc = A + eps, A the digits times 2^41, every update gives X^a A + eps -- the first rounding is
    carried along, not compounded -- so the error against the rotated LUT is eps - X^r eps, r the sum
    of the a_i s_i: at most 2^41 however many steps, and zero only when r is 0 mod 2N"""
    n_poly, n = 64, 4
    rnd = random.Random(40 + grouping)
    secret = [1, 0, 1, 1]
    if grouping == CLASSIC:
        plain = secret
    else:  # group i: the indicators of (s_2i, s_2i+1) = (1, 0), (0, 1), (1, 1)
        plain = [int(secret[2 * i] == (B & 1) and secret[2 * i + 1] == B >> 1) for i in range(n // 2) for B in (1, 2, 3)]
    bsk = np.zeros((len(plain), 2, 2, n_poly), np.uint64)
    for q, m in enumerate(plain):
        bsk[q, 0, 0, 0] = bsk[q, 1, 1, 0] = m << 41
    table = S.TABLES[0]
    lut = X.lut_poly(table, n_poly) + np.array([rnd.getrandbits(41) for _ in range(n_poly)], np.uint64)
    for m in range(16):
        mask = [rnd.getrandbits(7) << 57 for _ in range(n)]  # exact under the modulus switch to 2N = 128
        body = (sum(a * s for a, s in zip(mask, secret)) + (m << 59) + rnd.randint(-(1 << 54), 1 << 54)) % (1 << 64)
        small = np.array(mask + [body], np.uint64)
        acc = X.blind_rotate(bsk, small, lut, grouping)
        assert not acc[0].any()
        err = X.signed(acc[1] - X.ideal_rotation(small, secret, lut))
        r = sum((a >> 57) * s for a, s in zip(mask, secret)) % (2 * n_poly)
        assert int(np.abs(err).max()) <= 1 << 41 and bool(err.any()) == (r != 0)
        assert decode(acc[1][0]) == table[m]


# ---------------------------------------------------------------- b. sharp tier
def _hand_rows(ok):
    """two big LWE rows for n = 1 whose mask exponent after keyswitch and modulus switch is 0 (a zero
    mask: the update runs with X^0 - 1 = 0) and 2N - 1 (one mask word, the first 15-bit pattern whose
    digits times the key's first column land there)"""
    rows = np.zeros((2, N + 1), np.uint64)
    rows[0, N] = np.uint64(5 * DELTA + (1 << 57))
    cand = (np.arange(1 << 15, dtype=np.uint64) << np.uint64(49)).reshape(-1, N)
    d = ks_ref.digits(cand).reshape(-1, ks_ref.LEVELS)  # candidate p: the digits of word p << 49
    col = np.asarray(ok.ksk, np.uint64).reshape(N, ks_ref.LEVELS, 2)[0, :, 0]
    with np.errstate(over="ignore"):
        a = X.modswitch(np.uint64(0) - d.astype(np.uint64) @ col, N)
    rows[1, 0] = np.uint64(int(np.flatnonzero(a == 2 * N - 1)[0]) << 49)
    rows[1, N] = np.uint64(11 * DELTA)
    return rows


@functools.lru_cache(maxsize=None)
def sharp_case(n, grouping, seed=S.SEEDS[0]):
    """(smalls, luts, exact accumulators, oracle accumulators) of the committed sharp set"""
    ok = keys(n, grouping)
    cts, luts = inputs(ok, S.SHARP_COUNT, seed)
    if (n, grouping) == (1, CLASSIC):
        cts = np.concatenate([cts, _hand_rows(ok)])
        luts = np.concatenate([luts, luts[:2]])
    smalls = ks_ref.keyswitch_np(ok.ksk, n, cts)
    assert np.array_equal(smalls, ok.keyswitch_batch(cts))
    exact = X.blind_rotate_batch(ok.bsk, smalls, luts, grouping)
    f64 = np.stack([oracle_glwe(ok, s, l) for s, l in zip(smalls, luts)])
    for a in (smalls, luts, exact, f64):
        a.setflags(write=False)
    return smalls, luts, exact, f64


def sharp_word_figures(n, grouping, seed=S.SEEDS[0]):
    """(largest, rms) |oracle word - exact word| over all 4096 words of every accumulator of the set"""
    _, _, exact, f64 = sharp_case(n, grouping, seed)
    with np.errstate(over="ignore"):
        diff = X.signed(f64 - exact)
    return int(np.abs(diff).max()), S.rms(diff)


def test_sharp_set_reaches_the_rotations():
    """>= 48 distinct exponents, odd and even, in all four quarter turns, per set; the hand-built rows
    reach 0 and 2N - 1"""
    for n, g in S.SHARP_SETS:
        smalls = sharp_case(n, g)[0]
        a = X.modswitch(smalls[:, :n], N).astype(np.int64)
        if g == MULTIBIT:
            a = np.concatenate([a, a.sum(axis=1, keepdims=True) % (2 * N)], axis=1)
        used = {int(x) for x in a.reshape(-1)}
        assert len(used) >= 48, (n, g, len(used))
        assert {x % 2 for x in used} == {0, 1} and {x // (N // 2) for x in used} == {0, 1, 2, 3}
        if g == CLASSIC:
            assert [int(x) for x in a[S.SHARP_COUNT:, 0]] == [0, 2 * N - 1]
            assert not smalls[S.SHARP_COUNT, :n].any()


@pytest.mark.parametrize("s", S.SHARP_SETS, ids=S.set_id)
def test_sharp_words_within_caps(s):
    worst, r = sharp_word_figures(*s)
    print(f"\nsharp {S.set_id(s)}: |oracle - exact| over {sharp_case(*s)[2].size} words: max 2^{S.log2(worst):.2f}, "
          f"rms 2^{S.log2(r):.2f}; cap 2^{S.log2(S.WORD_CAP[s]):.2f}")
    assert worst < S.WORD_CLAIM
    assert worst <= S.WORD_CAP[s]


# ---------------------------------------------------------------- c. multi-step tier
def multi_step_figures(n, grouping, count, seed):
    """(rms exact, rms f64, R, worst |f64 - exact| / exact sigma, decodes right) of one set: output
    phases (coefficient 0) of `count` ciphertexts, or all 2048 phase coefficients of one"""
    ok = keys(n, grouping)
    cts, luts = inputs(ok, count, seed)
    smalls = ks_ref.keyswitch_np(ok.ksk, n, cts)
    if count == 1:
        exact = X.blind_rotate(ok.bsk, smalls[0], luts[0], grouping, threads=4)[None]
    else:
        exact = X.blind_rotate_batch(ok.bsk, smalls, luts, grouping)
    f64 = np.stack([oracle_glwe(ok, s, l) for s, l in zip(smalls, luts)])
    ideal = np.stack([X.ideal_rotation(s, ok.lwe_sk, l) for s, l in zip(smalls, luts)])
    with np.errstate(over="ignore"):
        if count == 1:
            ph = [X.glwe_phase(a[0], ok.glwe_sk) for a in (exact, f64)]
            errs = [X.signed(p - ideal[0]) for p in ph]
            ph = [p[:1] for p in ph]
        else:
            ph = [np.array([X.lwe_phase(X.sample_extract(g), ok.glwe_sk) for g in a]) for a in (exact, f64)]
            errs = [X.signed(p - ideal[:, 0]) for p in ph]
    want = [S.table_of(i)[m] for i, m in enumerate(S.messages(count))]
    right = all([decode(v) for v in p] == want for p in ph) and [decode(v) for v in ideal[:, 0]] == want
    return S.phase_figures(*errs) + (right,)


@pytest.mark.parametrize("s", list(S.MULTI_SETS), ids=S.set_id)
def test_multi_step_phase_within_caps(s):
    t0 = time.perf_counter()
    se, sf, ratio, worst, right = multi_step_figures(*s, S.MULTI_SETS[s], S.SEEDS[0])
    print(f"\nmulti-step {S.set_id(s)}: phase error rms exact 2^{S.log2(se):.2f}, f64 2^{S.log2(sf):.2f}, R = {ratio:.3f} "
          f"(cap {S.RATIO_CAP[s]:.3f}), worst |f64 - exact| = {worst:.3f} sigma (cap {S.DIFF_CAP[s]:.3f}); "
          f"{time.perf_counter() - t0:.1f} s")
    assert right
    assert ratio <= S.RATIO_CAP[s]
    assert worst <= S.DIFF_CAP[s]


if __name__ == "__main__":
    for s in S.SHARP_SETS:
        for seed in S.SEEDS:
            w, r = sharp_word_figures(*s, seed)
            print(f"sharp {S.set_id(s)} seed {seed:#x}: max 2^{S.log2(w):.2f} ({w}), rms 2^{S.log2(r):.2f}", flush=True)
    for s, count in S.MULTI_SETS.items():
        for seed in S.SEEDS:
            se, sf, ratio, worst, right = multi_step_figures(*s, count, seed)
            print(f"multi-step {S.set_id(s)} seed {seed:#x}: exact 2^{S.log2(se):.2f} f64 2^{S.log2(sf):.2f} R {ratio:.4f} "
                  f"worst {worst:.4f} sigma, decodes {'right' if right else 'WRONG'}", flush=True)
