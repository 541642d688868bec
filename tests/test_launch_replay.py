"""The launch order on the CPU: programs run on a simulated context (fhe_host_sim_ctx_create) with the launch trace
on (fhe_ctx_trace), and what Engine::flush launched -- after the dead-node sweep and its remap, the level schedule,
flush_for's closure split, the slices of FHE_TUNE_FLUSH_DEPTH levels -- is replayed in plaintext by
tests/launch_replay.py, in the order it was launched.

After every program: the structural checks hold (every source written earlier, no destination twice or read in its
own level, node counts equal to fhe_ctx_level_log and to the fhe_ctx_stats delta), every launched node's input lies
in its table's domain, and the replayed value of the result's blocks (sum block 4^k mod 2^bits) equals both the Python
integer and the simulated context's own decryption.  The op and width lists are those of test_radix_sim.py,
test_radix_widths.py and test_sim_context.py.  Two tests mutate a recorded trace and require the replay to fail."""
import contextlib
import random

import pytest

import launch_replay as LR
import ref_semantics as R
import test_sim_context as TS
from fhe_sign import (COMPAT, FAST, SECP256K1_N_C, BigUintFHE, FheUint, SimContext, SimKey, set_server_key, tuning)
from test_radix_sim import operands
from test_radix_widths import _clear_divisors, _shift_cases
from test_radix_sim import SHL, SHR

WIDTHS = [2, 6, 8, 34, 66, 256, 258]
BINARY = {k: v for k, v in TS.BINARY.items() if k not in ("div", "rem")}
OPS = sorted(BINARY) + sorted(TS.CLEAR)


@pytest.fixture(scope="module")
def sim():
    ctx = SimContext()
    set_server_key(ctx)
    yield ctx, SimKey()
    set_server_key(None)
    ctx.close()


@pytest.fixture
def rec(sim):
    r = LR.Recorder(sim[0])
    yield r
    r.close()


class Program:
    """operands noted as they are encrypted, results read (decrypted: the flush a program makes) and kept by address"""

    def __init__(self, rec, ck):
        self.rec, self.ck, self.results = rec, ck, []

    def enc(self, v, bits):
        return self.rec.note(FheUint.try_encrypt(v, self.ck, bits=bits), v)

    def big(self, limbs):
        v = R.from_limbs(limbs)
        return self.rec.note(BigUintFHE.new(v, self.ck), v)

    def read(self, X, want, what):
        got = X.decrypt(self.ck)
        self.results.append((self.rec.addrs(X), X.bits, want, got, what))

    def read_limbs(self, B, want, mode, what):
        """a BigUintFHE: its decryption (a sum's reads its column form and leaves its digits pending), then its
        digits launched and read limb by limb"""
        got = B.decrypt_limbs(self.ck)
        assert TS.same_limbs(got, want, mode), what
        B.to_radix(32 * max(1, len(got))).decrypt(self.ck)  # a full flush: the digits' own normalization
        addrs, triv = self.rec.addrs(B)
        assert len(addrs) == 16 * len(got), what
        for i, limb in enumerate(got):
            self.results.append(((addrs[16 * i:16 * i + 16], triv[16 * i:16 * i + 16]), 32, limb, limb, what + (i,)))

    def check(self, min_nodes=1):
        records, tables = self.rec.finish()
        assert len(LR.nodes_of(records)) >= min_nodes
        val, _ = LR.replay_plain(records, tables, self.rec.inputs)
        for (addrs, triv), bits, want, got, what in self.results:
            assert got == want, what
            assert LR.value_of(val, addrs, triv, bits) == want, what
        return records, tables, val


def _pairs(bits, rng, count):
    return operands(bits, rng, count)[-(count + 3):]  # three edge pairs and the random ones


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("op", OPS)
def test_radix_ops_replayed(sim, rec, op, bits):
    ctx, ck = sim
    rng = random.Random(0x1A7C * bits + OPS.index(op))
    P = Program(rec, ck)
    for x, y in _pairs(bits, rng, 2 if bits >= 256 else 4):
        X = P.enc(x, bits)
        if op in BINARY:
            y = y % (1 << bits)
            P.read(BINARY[op][1](X, P.enc(y, bits)), BINARY[op][0](x, y, bits), (op, bits, hex(x), hex(y)))
        else:
            c = rng.getrandbits(max(2, bits // 2)) | 1
            P.read(TS.CLEAR[op][1](X, c), TS.CLEAR[op][0](x, c, bits), (op, bits, hex(x), hex(c)))
    P.check()


@pytest.mark.parametrize("bits", [6, 34, 66, 258])
@pytest.mark.parametrize("op", [SHR, SHL])
def test_encrypted_shifts_replayed(sim, rec, op, bits):
    """the non-power-of-two widths, where the amount is first reduced mod the width under encryption"""
    ctx, ck = sim
    P = Program(rec, ck)
    name = "shr" if op == SHR else "shl"
    cases = _shift_cases(bits, op)
    for a, s in cases[:: max(1, len(cases) // 12)]:
        P.read(BINARY[name][1](P.enc(a, bits), P.enc(s, bits)), BINARY[name][0](a, s, bits), (name, bits, hex(a), hex(s)))
    P.check()


@pytest.mark.parametrize("lead", [0, 2, 16])
@pytest.mark.parametrize("bits", [6, 8, 34, 64])
def test_encrypted_divrem_replayed(sim, rec, bits, lead):
    """the radix-16 leads: half-step tables and the 16-term wide combinations"""
    ctx, ck = sim
    rng = random.Random(0xD17 * bits + lead)
    M = 1 << bits
    P = Program(rec, ck)
    with tuning(div_r16_lead=lead):
        for x, y in _pairs(bits, rng, 3) + [(rng.getrandbits(bits), 0), (M - 1, 1), (rng.getrandbits(bits), rng.getrandbits(bits // 2) | 1)]:
            q, r = P.enc(x, bits).div_rem(P.enc(y, bits))
            P.read(q, x // y if y else M - 1, ("q", bits, lead, hex(x), hex(y)))
            P.read(r, x % y if y else x, ("r", bits, lead, hex(x), hex(y)))
    records, tables, _ = P.check()
    if lead and bits >= 8:
        assert any(k == LR.LUT_HALF_STEP for k, _ in tables.values())
    if lead == 16 and bits >= 34:
        assert max(len(n.terms) for n in LR.nodes_of(records)) > 6  # a wide combination was launched


@pytest.mark.parametrize("residue", [0, 1])
@pytest.mark.parametrize("bits", [34, 66, 258])
def test_scalar_divrem_replayed(sim, rec, bits, residue):
    """both methods of the division by a public divisor: the multiplier (0) and the residue split (1)"""
    ctx, ck = sim
    rng = random.Random(0x5CA1 * bits + residue)
    M = 1 << bits
    P = Program(rec, ck)
    with tuning(scalar_div_residue=residue):
        for d in _clear_divisors(bits, rng)[2::3]:
            for a in (M - 1, rng.getrandbits(bits)):
                X = P.enc(a, bits)
                P.read(X // d, a // d, ("div", bits, residue, hex(a), hex(d)))
                P.read(X % d, a % d, ("rem", bits, residue, hex(a), hex(d)))
    P.check()


def test_rem_pseudo_mersenne_replayed(sim, rec):
    ctx, ck = sim
    rng = random.Random(0x9E5)
    n = (1 << 256) - SECP256K1_N_C
    P = Program(rec, ck)
    for x in ((1 << 512) - 1, rng.getrandbits(512), n * n - 1):
        P.read(P.enc(x, 512).rem_pseudo_mersenne(256, SECP256K1_N_C), x % n, ("rem_pm", hex(x)))
    P.check()


# ---------------------------------------------------------------------------------------------- BigUintFHE
def _limbs(rng, n):
    return [rng.getrandbits(32) | 1 for _ in range(n)]


@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
@pytest.mark.parametrize("n", [2, 3])
def test_biguint_products_replayed(sim, rec, n, mode):
    """mul, mul_add, the call site k + (a * b) with the product released before the flush, and the column form"""
    ctx, ck = sim
    rng = random.Random(0xB16 * n + mode)
    P = Program(rec, ck)
    for al in TS.limb_values(n, rng):
        bl, kl = _limbs(rng, n), _limbs(rng, n)
        a, b, k = P.big(al), P.big(bl), P.big(kl)
        pl = TS.mul_ref(al, bl, mode)
        P.read_limbs(a.mul(b, mode), pl, mode, ("mul", n, mode))
        P.read_limbs(a.mul_add(b, k, mode), R.biguint_add(kl, pl), mode, ("mul_add", n, mode))
        P.read_limbs(k.add(a.mul(b, mode)), R.biguint_add(kl, pl), mode, ("call site", n, mode))
        assert a.mul_add_value(b, k, ck, mode) == R.from_limbs(R.biguint_add(kl, pl)), ("columns", n, mode)
    P.check()


@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
@pytest.mark.parametrize("decrypt_first", [True, False], ids=["decrypt-reuse", "reuse-decrypt"])
@pytest.mark.parametrize("scenario", TS.SCENARIOS)
def test_biguint_states_replayed(sim, rec, scenario, decrypt_first, mode):
    """test_sim_context.py's scenarios at two limbs: a source decrypted first (its column form read by flush_for,
    its digits left pending) and then reused, or reused first; with the source handle released mid-graph (the sweep)"""
    ctx, ck = sim
    n = 2
    rng = random.Random(0xB16 * n + mode)
    P = Program(rec, ck)
    al, bl, kl = TS.limb_values(n, rng)[1], _limbs(rng, n), _limbs(rng, n)
    made = []

    def big(limbs, _ck):
        made.append(P.big(limbs))
        return made[-1]

    old, TS.big = TS.big, big
    try:
        for release in (False, True):
            (src, src_limbs), use, want = dict(TS._scenarios(al, bl, kl, ck, mode))[scenario]()
            what = (scenario, decrypt_first, release, mode)
            if decrypt_first:
                assert TS.same_limbs(src.decrypt_limbs(ck), src_limbs, mode), what
            out = use(src)
            if release:
                del src
                made.clear()
            P.read_limbs(out, want, mode, what)
            if not release:
                P.read_limbs(src, src_limbs, mode, what + ("source",))
    finally:
        TS.big = old
    P.check()


def test_handle_dropped_mid_graph_is_swept(sim, rec):
    """values recorded and released before any flush: their bootstraps are dropped, the remap holds"""
    ctx, ck = sim
    rng = random.Random(0x5EE9)
    bits = 34
    x, y, z = (rng.getrandbits(bits) for _ in range(3))
    M = 1 << bits
    P = Program(rec, ck)
    X, Y, Z = P.enc(x, bits), P.enc(y, bits), P.enc(z, bits)
    dead1 = X * Y          # never read
    keep = (X + Y) * Z
    dead2 = keep - X       # reads a live value, dies itself
    keep2 = keep & Y
    del dead1, dead2
    import fhe_sign
    before = fhe_sign.stats(ctx)[0]
    P.read(keep2, ((x + y) * z % M) & y, "keep2")
    P.read(keep, (x + y) * z % M, "keep")
    launched = fhe_sign.stats(ctx)[0] - before
    records, _, _ = P.check()
    recorded_alone = len(LR.nodes_of(records))
    assert recorded_alone == launched
    # the same program with every handle kept launches more: the two dead values were not launched above
    rec2 = LR.Recorder(ctx)
    P2 = Program(rec2, ck)
    X, Y, Z = P2.enc(x, bits), P2.enc(y, bits), P2.enc(z, bits)
    d1 = X * Y
    keep = (X + Y) * Z
    d2 = keep - X
    P2.read(keep & Y, ((x + y) * z % M) & y, "keep2")
    P2.read(d1, x * y % M, "d1")
    P2.read(d2, ((x + y) * z - x) % M, "d2")
    records2, _, _ = P2.check()
    assert len(LR.nodes_of(records2)) > recorded_alone


# ------------------------------------------------------------------------- slices and Karatsuba thresholds
def _mixed_program(P, rng):
    bits = 34
    M = 1 << bits
    x, y = rng.getrandbits(bits), rng.getrandbits(bits // 2) | 1
    X, Y = P.enc(x, bits), P.enc(y, bits)
    q, r = X.div_rem(Y)
    P.read((X * Y) + q, (x * y + x // y) % M, "mul + q")
    P.read(r >> Y, (x % y) >> (y % bits), "r >> y")
    al, bl, kl = _limbs(rng, 3), _limbs(rng, 3), _limbs(rng, 3)
    for mode in (COMPAT, FAST):
        P.read_limbs(P.big(al).mul_add(P.big(bl), P.big(kl), mode), R.biguint_add(kl, TS.mul_ref(al, bl, mode)), mode,
                     ("mul_add", mode))


@pytest.mark.parametrize("depth", [0, 7, 64])
def test_sliced_flushes_replayed(sim, rec, depth):
    ctx, ck = sim
    P = Program(rec, ck)
    with tuning(flush_depth=depth):
        _mixed_program(P, random.Random(0xF1 + depth))
    P.check()


@pytest.mark.parametrize("kara", [0, 6, None])
def test_karatsuba_thresholds_replayed(sim, rec, kara):
    ctx, ck = sim
    P = Program(rec, ck)
    with (tuning(kara_min=kara, kara_compat_min=kara) if kara is not None else contextlib.nullcontext()):
        _mixed_program(P, random.Random(0xCA7 + (kara or 99)))
        x, y = (1 << 66) - 1, random.Random(kara or 99).getrandbits(66)
        P.read(P.enc(x, 66) * P.enc(y, 66), x * y % (1 << 66), "mul 66")
    P.check()


# ---------------------------------------------------------------------------------------------- op chains
@pytest.mark.parametrize("bits", [6, 8, 18, 34])
def test_chains_replayed(sim, rec, bits, monkeypatch):
    """test_sim_context.py::test_chains_through_the_abi itself, with its encryptions noted and its decryptions
    kept by address: several ops share one pending graph, handles leave while it is pending"""
    ctx, ck = sim
    P = Program(rec, ck)
    monkeypatch.setattr(TS, "enc", lambda v, _ck, b: P.enc(v, b))
    decrypt = FheUint.decrypt

    def noting(self, key):
        got = decrypt(self, key)
        P.results.append((rec.addrs(self), self.bits, got, got, ("chain", bits, len(P.results))))
        return got

    monkeypatch.setattr(FheUint, "decrypt", noting)
    TS.test_chains_through_the_abi(sim, bits)
    monkeypatch.undo()
    assert len(P.results) >= TS.CHAIN_STEPS[bits]
    P.check(min_nodes=TS.CHAIN_STEPS[bits])


# ---------------------------------------------------------------------------------------------- the replay itself
@pytest.mark.parametrize("grouping", [1, 2], ids=["classic", "multibit"])
def test_word_replay_of_a_simulated_trace_decrypts(sim, rec, grouping):
    """tests/launch_replay.py's word replay and its table polynomials (the half-step one is restated there), without
    a GPU: the trace of an 8-bit encrypted division on the simulated context, its operands encrypted by the oracle
    at n = 16, every node bootstrapped by the oracle -- the result's words decrypt to the quotient and remainder"""
    import oracle
    from lwe_dims import oracle_params
    ctx, ck = sim
    ok = oracle.OracleKeys(0xC0FFEE, oracle_params(16, grouping))
    rng = ok.rng(5)
    x, y = 0xE7, 0x0B

    def enc(v):
        X = FheUint.try_encrypt(v, ck, bits=8)
        return rec.note_rows(X, [ok.encrypt(rng, d) for d in LR.digits(v, 4)])

    q, r = enc(x).div_rem(enc(y))
    assert (q.decrypt(ck), r.decrypt(ck)) == (x // y, x % y)
    records, tables = rec.finish()
    assert LR.LUT_HALF_STEP in {k for k, _ in tables.values()}
    val, _ = LR.replay_words(records, tables, rec.inputs, ok)
    for X, want in ((q, x // y), (r, x % y)):
        addrs, triv = rec.addrs(X)
        assert sum((t if a == 0 else ok.decrypt(val[a])) << (2 * k) for k, (a, t) in enumerate(zip(addrs, triv))) % 256 == want


def test_trace_is_off_by_default_and_refuses_an_overflow(sim):
    """off: nothing is recorded; on: at most 2^23 words, and a trace that would have passed them is refused, not
    handed out short (reset clears it and the next trace is whole again)"""
    from fhe_sign import FheError, trace_enable, trace_read
    ctx, ck = sim
    trace_enable(ctx, False)
    trace_read(ctx, reset=True)
    x = FheUint.try_encrypt(5, ck, bits=8)
    assert (x + x).decrypt(ck) == 10
    assert len(trace_read(ctx)) == 0
    trace_enable(ctx, True)
    try:
        big = (1 << 4096) - 1
        for _ in range((1 << 23) // (4 * 2048) + 1):  # one 4-word write record per encrypted block
            FheUint.try_encrypt(big, ck, bits=4096)
        with pytest.raises(FheError, match="overflowed"):
            trace_read(ctx, reset=False)
        with pytest.raises(FheError, match="overflowed"):
            trace_read(ctx, reset=True)
        assert (x + x).decrypt(ck) == 10
        records = LR.parse(trace_read(ctx))
        assert len(LR.nodes_of(records)) > 0
    finally:
        trace_enable(ctx, False)


def test_trace_only_reads(sim):
    """the same program with the trace off and on: the same level log, bootstrap count and result"""
    from fhe_sign import level_log, stats, trace_enable, trace_read
    ctx, ck = sim
    seen = []
    for on in (False, True):
        level_log(ctx, reset=True)
        pbs0 = stats(ctx)[0]
        trace_enable(ctx, on)
        try:
            X, Y = FheUint.try_encrypt(0x2B7C9D3A5, ck, bits=34), FheUint.try_encrypt(0x19E3B, ck, bits=34)
            q, r = (X * Y + X).div_rem(Y)
            got = (q.decrypt(ck), r.decrypt(ck))
        finally:
            trace_enable(ctx, False)
        assert (len(trace_read(ctx, reset=True)) > 0) == on
        seen.append((got, level_log(ctx, reset=True), stats(ctx)[0] - pbs0))
    assert seen[0] == seen[1]


def test_swapped_levels_fail_the_structural_check(sim, rec):
    ctx, ck = sim
    P = Program(rec, ck)
    x, y = 0x2B7C9D3A5, 0x19E3B
    P.read(P.enc(x, 34) * P.enc(y, 34), x * y % (1 << 34), "mul")
    records, tables = rec.finish()
    LR.check_structure(records)
    levels = [i for i, r in enumerate(records) if isinstance(r, LR.Level)]
    # two consecutive levels of which the second reads what the first writes
    pair = next((i, j) for i, j in zip(levels, levels[1:])
                if {n.dst for n in records[i].nodes} & {s for n in records[j].nodes for s, _ in n.terms})
    i, j = pair
    swapped = list(records)
    swapped[i], swapped[j] = LR.Level(records[i].number, records[j].split, records[j].nodes), \
        LR.Level(records[j].number, records[i].split, records[i].nodes)
    swapped = LR.parse(LR.unparse(swapped))  # through the wire format, as a recorded trace would come
    with pytest.raises(LR.ReplayError, match="reads .* which no write, lincomb or earlier level has written"):
        LR.check_structure(swapped)


def test_coefficient_off_by_16_fails_the_plaintext_replay(sim, rec):
    ctx, ck = sim
    P = Program(rec, ck)
    x, y = 0x2B7C9D3A5, 0x19E3B
    X, Y = P.enc(x, 34), P.enc(y, 34)
    noted = {a: list(q) for a, q in rec.inputs.q.items()}
    P.read(X * Y, x * y % (1 << 34), "mul")
    records, tables = rec.finish()

    def inputs():
        fresh = LR.Inputs()
        for a, vs in noted.items():
            fresh.note([a] * len(vs), vs)
        return fresh

    val, _ = LR.replay_plain(records, tables, inputs())
    (addrs, triv), bits, want, got, _ = P.results[0]
    assert LR.value_of(val, addrs, triv, bits) == want == got

    def mutated(pick):
        """the trace with +16 on the first coefficient `pick` accepts: (level index, node index, term index) or None"""
        words = LR.parse(LR.unparse(records))
        for r in words:
            if not isinstance(r, LR.Level):
                continue
            for n in r.nodes:
                for t, (s, coef) in enumerate(n.terms):
                    if tables[n.lut][0] == LR.LUT_INTEGER and pick(val[s]):
                        n.terms[t] = (s, coef + 16)
                        return words
        return None

    # a source holding 1 or 3: the input moves by 16 or 48 steps, on a torus of 32 into the padding bit's half
    out = mutated(lambda h2: h2 in (2, 6))
    assert out is not None
    with pytest.raises(LR.ReplayError, match="outside the message space"):
        LR.replay_plain(out, tables, inputs())
    # the limit, stated: on a source that holds 0 or 2 the input moves by a whole turn of the torus or not at all, and
    # the change is invisible in plaintext (wrong but congruent is the word replay's to find,
    # tests/test_launch_replay_gpu.py)
    blind = mutated(lambda h2: h2 in (0, 4))
    if blind is not None:
        val2, _ = LR.replay_plain(blind, tables, inputs())
        assert LR.value_of(val2, addrs, triv, bits) == want
