"""The launch order on the GPU, word for word: programs run on a device context with the launch trace on
(fhe_ctx_trace), and every launched node -- its fields read back from the staged host copy of the level descriptors,
the wide term tables and the scatter tables -- is evaluated again by tests/launch_replay.py through the oracle: the
wrapping u64 combination, the oracle's keyswitch, ms_center_ref in centered mode, the oracle's blind rotation under
the polynomial built here from fhe_ctx_lut_table's entries.  Comparison is exact equality of u64 words.

After every program: the structural checks; the result's exported words equal the replay's map at the result's
addresses (the map holds the oracle's output of EVERY launched node: none is sampled or skipped); the decryption is
the expected integer; for every LUT id in the trace the device table (fhe_ctx_export_luts) equals the Python
polynomial.

Keys at n = 16 (tests/lwe_dims.py, the seed of test_br_qz_gpu.py), classic and multi-bit; one chain at the default
n = 834.  Budgets: at most 20,000 replayed bootstraps per test at n = 16 and 512 at n = 834 (asserted on the
trace).  The oracle's rate, measured on 8 CPU threads: 0.11 ms (classic) / 0.13 ms (multi-bit) per bootstrap at
n = 16 in a batched level, 0.5 / 0.65 ms one by one (the centered path), 4.6 / 7.3 ms at n = 834.  Replay seconds of
the programs below on the same 8 threads, measured on a simulated context's trace of the same program with
oracle-encrypted operands (bootstraps: classic / multi-bit seconds):
  ops at 6 bits      161: 0.06 / 0.08      division          1408: 0.24 / 0.30     recycled slots  125: 0.03 / 0.04
  ops at 8 bits      170: 0.04 / 0.07      BigUintFHE, both 14597: 2.06 / 2.74     configurations  ~100: 0.03 each
  ops at 34 bits    1570: 0.27 / 0.36        modes (one mode: half)                 chain            41: 0.01 / 0.02
  pseudo-Mersenne    466: 0.09 / 0.11      chain, centered (one by one) 41: 0.04 / 0.06      chain at n = 834  41: 0.5"""
import contextlib
import random

import numpy as np
import pytest

import launch_replay as LR
import oracle
import ref_semantics as R
from fhe_sign import (COMPAT, FAST, BigUintFHE, Context, FheUint, block_addrs, export_luts, generate_keys, lut_table,
                      set_server_key, tuning)
from lwe_dims import CLASSIC, MULTIBIT, oracle_params, product_params

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
QY, AUTO, QZ = 4, 7, 9
MAX_NODES_16, MAX_NODES_834 = 20000, 512


class Program:
    """a traced program on a device context: operands exported as they are encrypted (before any op is recorded: an
    export flushes), results decrypted, exported and kept alive, so that their slots are theirs until the check"""

    def __init__(self, ctx, ck, ok, centered=False):
        self.ctx, self.ck, self.ok, self.centered = ctx, ck, ok, centered
        self.rec = LR.Recorder(ctx)
        self.results = []

    def enc(self, v, bits):
        X = FheUint.try_encrypt(v, self.ck, bits=bits)
        return self.rec.note_rows(X, X.export())

    def big(self, limbs):
        B = BigUintFHE.new(R.from_limbs(limbs), self.ck)
        return self.rec.note_rows(B, B.to_radix(32 * len(limbs)).export())

    def read(self, X, want, what):
        got = X.decrypt(self.ck)
        self.results.append((X, X.export(), want, got, what))

    def read_big(self, B, want_limbs, same, what):
        got = B.decrypt_limbs(self.ck)
        assert same(got, want_limbs), what
        Xr = B.to_radix(32 * len(got))
        self.results.append((B, Xr.export(), R.from_limbs(got), R.from_limbs(got), what))

    def check(self, max_nodes=MAX_NODES_16):
        try:
            records, tables = self.rec.finish()
        finally:
            self.rec.close()
        nodes = LR.nodes_of(records)
        assert 0 < len(nodes) <= max_nodes, len(nodes)
        delta = self.ok.delta()
        for lut, (kind, entries) in tables.items():
            dev = export_luts(self.ctx, lut, 1)[0]
            assert np.array_equal(dev, LR.lut_poly(kind, entries, self.ok.make_lut, delta)), ("device table", lut, kind, entries)
        val, rewritten = LR.replay_words(records, tables, self.rec.inputs, self.ok, self.centered)
        for X, rows, want, got, what in self.results:
            assert got == want, what
            addrs, triv = block_addrs(self.ctx, X)
            assert len(addrs) == len(rows), what
            for k, (a, t) in enumerate(zip(addrs, triv)):
                if a == 0:
                    ref = np.zeros(LR.BIG_CT, np.uint64)
                    ref[LR.N] = np.uint64(t * delta)
                else:
                    ref = val[a]
                assert ref is not None and np.array_equal(rows[k], ref), (what, "block", k, hex(a))
        return records, val, rewritten, [rows for _, rows, _, _, _ in self.results]


def _env(n, grouping):
    ck, sk = generate_keys(product_params(n, grouping), seed=SEED)
    ok = oracle.OracleKeys(SEED, oracle_params(n, grouping))
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    return ck, ok, ctx


@pytest.fixture(scope="module", params=[CLASSIC, MULTIBIT], ids=["classic", "multibit"])
def env16(request):
    ck, ok, ctx = _env(16, request.param)
    yield ck, ok, ctx, request.param
    set_server_key(None)
    ctx.close()


# ------------------------------------------------------------------------------------------------ the programs
def prog_ops(P, bits):
    rng = random.Random(0x6A0 + bits)
    M = 1 << bits
    x, y = rng.getrandbits(bits) | 1 | M // 2, rng.getrandbits(bits) | 1
    s = rng.getrandbits(bits)
    c = rng.getrandbits(max(2, bits // 2)) | 1
    X, Y, S = P.enc(x, bits), P.enc(y, bits), P.enc(s, bits)
    P.read(X + Y, (x + y) % M, ("add", bits))
    P.read(X - Y, (x - y) % M, ("sub", bits))
    P.read(X * Y, x * y % M, ("mul", bits))
    P.read(X.lt(Y), int(x < y), ("lt", bits))
    P.read(X.min(Y), min(x, y), ("min", bits))
    P.read(X.max(Y), max(x, y), ("max", bits))
    P.read(X & Y, x & y, ("and", bits))
    P.read(X + c, (x + c) % M, ("addc", bits))
    P.read(X * c, x * c % M, ("mulc", bits))
    P.read(X & c, x & c, ("andc", bits))
    P.read(X >> 3, x >> (3 % bits), ("shrc", bits))
    P.read(X >> S, x >> (s % bits), ("shr", bits))
    P.read(X << S, (x << (s % bits)) % M, ("shl", bits))


def prog_division(P):
    rng = random.Random(0xD1)
    x, y, d = 0xE7, 0x0B, 7
    X, Y = P.enc(x, 8), P.enc(y, 8)
    Z = P.enc(0, 8)
    q, r = X.div_rem(Y)
    P.read(q, x // y, "q")
    P.read(r, x % y, "r")
    q0, r0 = X.div_rem(Z)
    P.read(q0, 255, "q by zero")
    P.read(r0, x, "r by zero")
    for residue in (0, 1):
        with tuning(scalar_div_residue=residue):
            P.read(X // d, x // d, ("divc", residue))
            P.read(X % d, x % d, ("remc", residue))
    del rng


def _same(mode):
    return (lambda g, w: g == w) if mode == COMPAT else (lambda g, w: R.from_limbs(g) == R.from_limbs(w))


def _mul_ref(a, b, mode):
    return R.biguint_mul(a, b) if mode == COMPAT else R.to_u32_digits(R.from_limbs(a) * R.from_limbs(b))


def prog_biguint(P, modes=(COMPAT, FAST)):
    rng = random.Random(0xB16)
    al, bl, kl = ([rng.getrandbits(32) | 1 | 1 << 31 for _ in range(2)] for _ in range(3))
    a, b, k = P.big(al), P.big(bl), P.big(kl)
    for mode in modes:
        want = R.biguint_add(kl, _mul_ref(al, bl, mode))
        P.read_big(a.mul_add(b, k, mode), want, _same(mode), ("mul_add", mode))
        # the call site: the product released before the flush, the sum decrypted from its column form
        P.read_big(k.add(a.mul(b, mode)), want, _same(mode), ("call site", mode))


def prog_rem_pm(P):
    c = 0x2F5
    for x in (0xFFFFFFFF, 0x9E3779B9):
        P.read(P.enc(x, 32).rem_pseudo_mersenne(16, c), x % ((1 << 16) - c), ("rem_pm", hex(x)))


def prog_recycle(P):
    """intermediates destroyed while the graph that reads them is pending, then more work: the pool hands their
    slots out again"""
    bits = 8
    M = 1 << bits
    x, y, z = 0xB5, 0x6E, 0x39
    X, Y, Z = P.enc(x, bits), P.enc(y, bits), P.enc(z, bits)
    t = X * Y
    u = t + Z
    del t          # read by u's pending graph
    v = u * X
    del u
    P.read(v, (x * y + z) * x % M, "v")
    w = (v - Y) * Z   # after the flush the released slots are free: these bootstraps write into them
    t2 = w + X
    del w
    P.read(t2, (((x * y + z) * x - y) * z + x) % M, "t2")
    P.read(t2.min(v), min((((x * y + z) * x - y) * z + x) % M, (x * y + z) * x % M), "min")


def prog_hundred(P):
    """about a hundred bootstraps, several levels, one wide enough to split over two emulated ranks"""
    bits = 8
    M = 1 << bits
    x, y = 0xC7, 0x5D
    P.ck.seed_encryption(77)  # the same operand words in every configuration
    X, Y = P.enc(x, bits), P.enc(y, bits)
    p = X * Y
    P.read(((p + X).max(Y) - X) * Y, (max((x * y + x) % M, y) - x) * y % M, "hundred")


def prog_chain(P):
    x, y = 0xA7, 0x3C
    X, Y = P.enc(x, 8), P.enc(y, 8)
    s = X + Y
    p = s * Y
    P.read(p.lt(X), int(((x + y) % 256) * y % 256 < x), "add -> mul -> lt")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("bits", [6, 8, 34])
def test_radix_ops_word_for_word(env16, bits):
    ck, ok, ctx, _ = env16
    P = Program(ctx, ck, ok)
    prog_ops(P, bits)
    P.check()


def test_division_word_for_word(env16):
    """8-bit encrypted divrem (half-step tables and their raw items) and the scalar division by both methods"""
    ck, ok, ctx, _ = env16
    P = Program(ctx, ck, ok)
    prog_division(P)
    records, _, _, _ = P.check()
    kinds = {lut_table(ctx, n.lut)[0] for n in LR.nodes_of(records)}
    assert LR.LUT_HALF_STEP in kinds and LR.LUT_INTEGER in kinds


@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
def test_biguint_word_for_word(env16, mode):
    """2 x 2 limbs: mul_add, and the call site k + (a * b) whose sum is decrypted from its column form"""
    ck, ok, ctx, _ = env16
    P = Program(ctx, ck, ok)
    prog_biguint(P, (mode,))
    P.check()


def test_rem_pseudo_mersenne_word_for_word(env16):
    ck, ok, ctx, _ = env16
    P = Program(ctx, ck, ok)
    prog_rem_pm(P)
    P.check()


def test_recycled_slots_word_for_word(env16):
    ck, ok, ctx, _ = env16
    P = Program(ctx, ck, ok)
    prog_recycle(P)
    _, _, rewritten, _ = P.check()
    assert rewritten > 0, "no address was written twice: the program recycled no slot and tests nothing"


@contextlib.contextmanager
def _config(ctx, name):
    try:
        if name in ("latency-none qy", "latency-none qz"):
            ctx.set_wide_threshold(0)
            ctx.set_br_kernel(QY if name.endswith("qy") else QZ)
        elif name == "latency-all":
            ctx.set_wide_threshold(1 << 30)
        elif name == "ks valu":
            ctx.set_ks_kernel(0)
        elif name == "fanout 2":
            ctx.set_fanout(min_level=4, emulate_ranks=2)
        with (tuning(flush_depth=0) if name == "flush depth 0" else contextlib.nullcontext()):
            yield
    finally:
        ctx.set_wide_threshold(256)
        ctx.set_br_kernel(AUTO)
        ctx.set_ks_kernel(1)
        ctx.set_fanout(min_level=257, emulate_ranks=0)


def test_configurations_agree_word_for_word(env16):
    """one program under the kernels and schedules a context can be moved to: every run passes its own replay, and
    the result words are the same in all of them"""
    ck, ok, ctx, grouping = env16
    names = ["latency-none qy", "latency-all", "ks valu", "flush depth 0", "fanout 2"]
    if grouping == CLASSIC:
        names.insert(1, "latency-none qz")  # the classic throughput kernel
    words, split = {}, False
    for name in names:
        with _config(ctx, name):
            P = Program(ctx, ck, ok)
            prog_hundred(P)
            records, _, _, rows = P.check()
            words[name] = rows
            if name == "fanout 2":
                split = any(r.split for r in records if isinstance(r, LR.Level))
    assert split, "no level was fanned out: the scatter tables were not staged"
    first = words[names[0]]
    for name in names[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(first, words[name])), name


def test_centered_modulus_switch_word_for_word(env16):
    ck, ok, ctx, _ = env16
    ctx.set_modulus_switch("centered")
    try:
        P = Program(ctx, ck, ok, centered=True)
        prog_chain(P)
        P.check()
    finally:
        ctx.set_modulus_switch("standard")


def test_deferred_upload_precedes_what_reads_it(env16):
    """the signer encrypts e and k on a helper thread while it records the FHE block, and the engine uploads them
    right before the block's first launch (Engine::upload_deferred): in the trace that write comes before every
    level that reads its slots -- the structural check -- and the signature is the plaintext signer's.  The words
    of e and k never leave the call, so this program is not replayed word for word."""
    from fhe_sign import Schnorr, compute_nonce
    ck, ok, ctx, _ = env16
    d = 0xB7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFEF
    msg = b"launch order"
    k0 = compute_nonce(d, msg, bytes(32))
    s = Schnorr()
    rec = LR.Recorder(ctx)
    try:
        D = BigUintFHE.new(d, ck)  # an upload of its own, inside the trace
        sig = s.sign_fhe_with_k0(msg, k0, d, D, ck, COMPAT)
        records, _ = rec.finish()
    finally:
        rec.close()
    assert sig == s.sign_with_k0(msg, k0, d)
    deferred = [r for r in records if isinstance(r, LR.Write) and r.kind == LR.WRITE_DEFERRED]
    assert [len(r.addrs) for r in deferred] == [2 * 8 * 16]  # e and k: 8 limbs of 16 blocks each, one upload
    first_level = next(i for i, r in enumerate(records) if isinstance(r, LR.Level))
    assert records.index(deferred[0]) < first_level
    nodes = LR.nodes_of(records)  # 59,020 of them (the compat 256-bit product): held to the structure, none replayed
    assert len(nodes) > 0
    assert {s_ for n in nodes for s_, _ in n.terms} & set(deferred[0].addrs)


def test_trace_only_reads(env16):
    """the same program with the trace off and on: the same result words, level log and bootstrap count"""
    from fhe_sign import level_log, stats, trace_enable, trace_read
    ck, ok, ctx, _ = env16
    seen = []
    for on in (False, True, False):
        level_log(ctx, reset=True)
        pbs0 = stats(ctx)[0]
        trace_read(ctx, reset=True)
        trace_enable(ctx, on)
        try:
            ck.seed_encryption(91)
            X, Y = FheUint.try_encrypt(0xC7, ck, bits=8), FheUint.try_encrypt(0x5D, ck, bits=8)
            q, r = (X * Y + X).div_rem(Y)
            words = np.concatenate([q.export(), r.export()])
        finally:
            trace_enable(ctx, False)
        assert (len(trace_read(ctx, reset=True)) > 0) == on
        seen.append((words, level_log(ctx, reset=True), stats(ctx)[0] - pbs0))
    for words, log, pbs in seen[1:]:
        assert np.array_equal(words, seen[0][0]) and log == seen[0][1] and pbs == seen[0][2]


def test_congruent_coefficient_fails_the_word_replay(env16):
    """the replay itself: a recorded trace with one coefficient changed by +16 on a source that holds 0 -- the
    plaintext of every node is unchanged (tests/test_launch_replay.py states that limit) -- no longer gives the
    device's words, while the trace as recorded does"""
    import copy
    ck, ok, ctx, _ = env16
    P = Program(ctx, ck, ok)
    x, y = 0xA4, 0x3C  # x's low block is 0
    X, Y = P.enc(x, 8), P.enc(y, 8)
    zero = block_addrs(ctx, X)[0][0]
    out = (X + Y) * Y
    assert out.decrypt(ck) == (x + y) * y % 256
    rows = out.export()
    try:
        records, tables = P.rec.finish()
    finally:
        P.rec.close()
    addrs, _ = block_addrs(ctx, out)

    def words(recs):
        val, _ = LR.replay_words(recs, tables, copy.deepcopy(P.rec.inputs), ok)
        return [val[a] for a in addrs]

    assert all(np.array_equal(a, b) for a, b in zip(words(records), rows))
    hit = next((n, t) for n in LR.nodes_of(records) for t, (s, _) in enumerate(n.terms) if s == zero)
    n, t = hit
    n.terms[t] = (n.terms[t][0], n.terms[t][1] + 16)
    assert not all(np.array_equal(a, b) for a, b in zip(words(records), rows))


@pytest.mark.parametrize("grouping", [CLASSIC, MULTIBIT], ids=["classic", "multibit"])
def test_chain_at_the_default_dimension(grouping):
    ck, ok, ctx = _env(834, grouping)
    try:
        P = Program(ctx, ck, ok)
        prog_chain(P)
        P.check(MAX_NODES_834)
    finally:
        set_server_key(None)
        ctx.close()
