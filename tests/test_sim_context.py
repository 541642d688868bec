"""The C ABI's radix layer on the CPU, through a simulated context (fhe_host_sim_ctx_create: no device, the engine
shadows every block's plaintext): FheUint and BigUintFHE run as they are, through capi_radix.cpp's glue -- widths,
casts, clones, word forms, amounts of another width, the column-form decryption and its partial flush.

What is pinned here: chains of ops whose results feed later ops, with handles released while their graph is
pending; every op on operands that SHARE blocks (a value with itself, its clone, a cast round trip); BigUintFHE
sums and products reused before and after their decryption; the glue's refusals; and the noise budget as the
engine enforces it -- on the merged coefficients of what is launched (fhe_ctx_noise_audit).

Every comparison is exact equality with Python integers: tfhe's semantics for the radix ops (wrapping + - *,
shift amounts mod the width, x / 0 = all ones, x % 0 = x: tests/test_radix_sim.py::expect), oracle/ref_semantics.py
for the BigUintFHE limbs (the compat mode's lost carries included).  The shadow evaluates a bootstrap when it is
recorded, so these tests see every recorded graph and every value, not the launch order."""
import ctypes as C
import random

import pytest

import ref_semantics as R
from fhe_sign import (COMPAT, FAST, BigUintFHE, FheError, FheUint, FheUint8, FheUint32, SimContext, SimKey, _lib,
                      noise_audit, set_server_key, stats, tuning)

K_MAX_NOISE = 25  # csrc/engine.h kMaxNoise
FHE_ERR_INVALID = -1


@pytest.fixture(scope="module")
def sim():
    ctx = SimContext()
    set_server_key(ctx)
    yield ctx, SimKey()
    set_server_key(None)
    ctx.close()


@pytest.fixture(autouse=True)
def audit(sim):
    """every test of this file: no recorded bootstrap above the budget, counted on what is launched"""
    ctx, _ = sim
    noise_audit(ctx, reset=True)
    yield
    assert noise_audit(ctx)[1] <= K_MAX_NOISE


def enc(v, ck, bits):
    return FheUint.try_encrypt(v, ck, bits=bits)


def cast(x, bits):
    h = C.c_void_p()
    _lib.check(_lib.load().fhe_radix_cast(None, x.handle, bits, C.byref(h)))
    return FheUint._wrap(h, bits)


def round_trip(x):
    """the same blocks through a wider width and back: no bootstrap"""
    return cast(cast(x, x.bits + 6), x.bits)


# op -> (python semantics on (x, y, bits), the encrypted form); `lt` gives one bit, div_rem a pair
BINARY = {
    "add": (lambda x, y, b: (x + y) % (1 << b), lambda X, Y: X + Y),
    "sub": (lambda x, y, b: (x - y) % (1 << b), lambda X, Y: X - Y),
    "mul": (lambda x, y, b: (x * y) % (1 << b), lambda X, Y: X * Y),
    "and": (lambda x, y, b: x & y, lambda X, Y: X & Y),
    "min": (lambda x, y, b: min(x, y), lambda X, Y: X.min(Y)),
    "max": (lambda x, y, b: max(x, y), lambda X, Y: X.max(Y)),
    "lt": (lambda x, y, b: int(x < y), lambda X, Y: X.lt(Y)),
    "shr": (lambda x, y, b: x >> (y % b), lambda X, Y: X >> Y),
    "shl": (lambda x, y, b: (x << (y % b)) % (1 << b), lambda X, Y: X << Y),
    "div": (lambda x, y, b: x // y if y else (1 << b) - 1, lambda X, Y: X // Y),
    "rem": (lambda x, y, b: x % y if y else x, lambda X, Y: X % Y),
}
CLEAR = {  # second operand public
    "andc": (lambda x, c, b: x & c, lambda X, c: X & c),
    "addc": (lambda x, c, b: (x + c) % (1 << b), lambda X, c: X + c),
    "mulc": (lambda x, c, b: (x * c) % (1 << b), lambda X, c: X * c),
    "divc": (lambda x, c, b: x // c, lambda X, c: X // c),
    "remc": (lambda x, c, b: x % c, lambda X, c: X % c),
}
KINDS = ("independent", "self", "clone", "derived")
# steps per width: several hundred where an encrypted division is a few hundred bootstraps, fewer where it is
# thousands (66) or where the width itself is the cost (130, 256)
CHAIN_STEPS = {6: 400, 8: 400, 18: 300, 32: 220, 34: 220, 64: 130, 66: 130, 130: 90, 256: 60}


@pytest.mark.parametrize("bits", sorted(CHAIN_STEPS))
def test_chains_through_the_abi(sim, bits):
    """test_radix_gpu.py::test_random_op_chains' generator on the CPU: results feed later steps; operands are
    encrypted, trivial (encrypt_trivial) and clear; the second operand is an independent value, the first operand
    itself, its clone, or a value derived from it without a bootstrap (a cast round trip, + 0), about a quarter
    each; reads are batched so that several ops share one pending graph, and in a quarter of the steps a random
    handle of the pool is dropped before the next read.  Every recorded step is compared."""
    ctx, ck = sim
    rng = random.Random(0xA11A5 + bits)
    M = (1 << bits) - 1
    names = sorted(BINARY) if bits <= 66 else [n for n in sorted(BINARY) if n not in ("div", "rem")]
    vals = [rng.getrandbits(bits) for _ in range(3)] + [0, M, rng.getrandbits(bits), 1]
    pool = [enc(v, ck, bits) for v in vals[:5]] + [FheUint.encrypt_trivial(v, bits=bits) for v in vals[5:]]
    met = {n: set() for n in names}
    deck = []  # (op, kind) pairs: every pair once per shuffle, so each kind is a quarter of every op's draws
    unread = []  # (handle, expected, what): decrypted together at the next read
    dropped = 0

    def read():
        for got, want, what in unread:
            assert got.decrypt(ck) == want, what
        unread.clear()

    for step in range(CHAIN_STEPS[bits]):
        i = rng.randrange(len(vals))
        x, X = vals[i], pool[i]
        if rng.random() < 0.2:
            op = rng.choice(sorted(CLEAR))
            c = rng.getrandbits(max(2, bits // 2)) | 1
            want, got = CLEAR[op][0](x, c, bits), CLEAR[op][1](X, c)
            kind = "clear"
        else:
            if not deck:
                deck = [(n, k) for n in names for k in KINDS]
                rng.shuffle(deck)
            op, kind = deck.pop()
            if kind == "independent":
                j = rng.randrange(len(vals))
                y, Y = vals[j], pool[j]
            else:
                y = x
                Y = {"self": lambda: X, "clone": X.clone,
                     "derived": (lambda: round_trip(X)) if step % 2 else (lambda: X + 0)}[kind]()
            met[op].add(kind)
            want, got = BINARY[op][0](x, y, bits), BINARY[op][1](X, Y)
            del Y
        unread.append((got, want, (bits, step, op, kind, hex(x))))
        if op != "lt":  # feed the result into later steps
            vals.append(want)
            pool.append(got)
        del X, got
        if step % 4 == 3:  # a handle leaves while the graph that reads it is pending
            k = rng.randrange(len(vals))
            vals.pop(k)
            pool.pop(k)
            dropped += 1
        while len(vals) > 12:
            k = rng.randrange(len(vals))
            vals.pop(k)
            pool.pop(k)
        if rng.random() < 0.4:
            read()
    read()
    assert dropped == CHAIN_STEPS[bits] // 4
    assert all(kinds == set(KINDS) for kinds in met.values()), {n: sorted(set(KINDS) - k) for n, k in met.items()}


def matrix_values(bits, rng):
    M = (1 << bits) - 1
    return [0, 1, M, 1 << (bits - 1), rng.getrandbits(bits) | 1 | 1 << (bits - 1)]


def alias_kinds(X):
    return (("self", X), ("clone", X.clone()), ("cast", round_trip(X)))


@pytest.mark.parametrize("bits", [6, 8, 34, 66])
def test_aliasing_matrix(sim, bits):
    """op(x, x), op(x, x.clone()), op(x, cast round trip of x) for every binary op and div_rem: the operands are
    the same blocks.  All ops of one value are recorded before the first read."""
    ctx, ck = sim
    rng = random.Random(0xA71A5 + bits)
    for x in matrix_values(bits, rng):
        X = enc(x, ck, bits)
        unread = []
        for kind, Y in alias_kinds(X):
            for op in sorted(BINARY):
                unread.append((BINARY[op][1](X, Y), BINARY[op][0](x, x, bits), (bits, hex(x), op, kind)))
            q, r = X.div_rem(Y)
            unread.append((q, 1 if x else (1 << bits) - 1, (bits, hex(x), "div_rem q", kind)))
            unread.append((r, 0, (bits, hex(x), "div_rem r", kind)))
        del Y
        for got, want, what in unread:
            assert got.decrypt(ck) == want, what


@pytest.mark.parametrize("bits", [128, 258])
@pytest.mark.parametrize("kara_min", [8, None])
def test_aliasing_wide_products_and_sums(sim, bits, kara_min):
    """x * x and x + x where the product takes the Karatsuba split (kara_min=8: every level of it; the default:
    the product's own rule): its memo of halves and half sums, keyed by operand address, sees one address twice,
    and a value and its clone at two addresses."""
    ctx, ck = sim
    rng = random.Random(0xCA7A + bits)
    M = 1 << bits
    import contextlib
    with (tuning(kara_min=kara_min) if kara_min else contextlib.nullcontext()):
        for x in matrix_values(bits, rng):
            X = enc(x, ck, bits)
            unread = [(f(X, Y), want, (bits, hex(x), name, kind)) for kind, Y in alias_kinds(X)
                      for name, f, want in (("mul", lambda a, b: a * b, x * x % M), ("add", lambda a, b: a + b, 2 * x % M))]
            for got, want, what in unread:
                assert got.decrypt(ck) == want, what


# ---------------------------------------------------------------------------------------------- BigUintFHE
def big(limbs, ck):
    return BigUintFHE.new(R.from_limbs(limbs), ck)


def limb_values(n, rng):
    """all-ones limbs (the compat product drops carries there) and random limbs with a set top limb"""
    rnd = [rng.getrandbits(32) for _ in range(n)]
    rnd[-1] |= 1 << 31
    return [[0xFFFFFFFF] * n, rnd]


def mul_ref(a, b, mode):
    return R.biguint_mul(a, b) if mode == COMPAT else R.to_u32_digits(R.from_limbs(a) * R.from_limbs(b))


def same_limbs(got, want, mode):
    """compat: the reference's limbs, one for one; fast: the true value (its limb count is the op's own)"""
    return got == want if mode == COMPAT else R.from_limbs(got) == R.from_limbs(want)


# scenario -> (sources, result): sources are the handles the result reuses; each gives (handle, reference limbs)
def _scenarios(al, bl, kl, ck, mode):
    a, b, k = big(al, ck), big(bl, ck), big(kl, ck)
    pl = mul_ref(al, bl, mode)
    sl = R.biguint_add(al, bl)
    kp = R.biguint_add(kl, pl)

    def product():
        return a.mul(b, mode)

    yield "a.add(a)", lambda: ((a, al), lambda s: s.add(s), R.biguint_add(al, al))
    yield "a.mul(a)", lambda: ((a, al), lambda s: s.mul(s, mode), mul_ref(al, al, mode))
    yield "a.mul_add(a, a)", lambda: ((a, al), lambda s: s.mul_add(s, s, mode), R.biguint_add(al, mul_ref(al, al, mode)))
    yield "P + P", lambda: ((product(), pl), lambda s: s.add(s), R.biguint_add(pl, pl))
    yield "P + P.clone()", lambda: ((product(), pl), lambda s: s.add(s.clone()), R.biguint_add(pl, pl))
    yield "(k + P) + (k + P)", lambda: ((k.add(product()), kp), lambda s: s.add(s), R.biguint_add(kp, kp))
    yield "P * P", lambda: ((product(), pl), lambda s: s.mul(s, mode), mul_ref(pl, pl, mode))
    yield "s + s", lambda: ((a.add(b), sl), lambda s: s.add(s), R.biguint_add(sl, sl))


SCENARIOS = ("a.add(a)", "a.mul(a)", "a.mul_add(a, a)", "P + P", "P + P.clone()", "(k + P) + (k + P)", "P * P", "s + s")


@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
@pytest.mark.parametrize("decrypt_first", [True, False], ids=["decrypt-reuse", "reuse-decrypt"])
@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9])
def test_biguint_states_and_aliasing(sim, n, scenario, decrypt_first, mode):
    """A BigUintFHE value in each of its states -- fresh limbs, a product (compat: lazy last waves), a sum (its
    column form kept, its carry propagation pending after a decryption: test_sum_decrypted_from_its_columns) --
    used on both sides of the next op.  Each scenario four ways: the source decrypted first and then reused, or
    reused first and then decrypted, and each of those again with the source handle released before the result
    is read.  Values: all-ones limbs, and at the small shapes random limbs too."""
    ctx, ck = sim
    rng = random.Random(0xB16 * n + mode)
    for al in limb_values(n, rng)[: 2 if n <= 3 else 1]:
        bl = [rng.getrandbits(32) | 1 for _ in range(n)]
        kl = [rng.getrandbits(32) | 1 for _ in range(n)]
        make = dict(_scenarios(al, bl, kl, ck, mode))[scenario]
        for release in (False, True):
            (src, src_limbs), use, want = make()
            what = (n, mode, scenario, decrypt_first, release, hex(al[0]))
            if decrypt_first:
                assert same_limbs(src.decrypt_limbs(ck), src_limbs, mode), what
            out = use(src)
            if release:
                del src
            assert same_limbs(out.decrypt_limbs(ck), want, mode), what
            if not release and not decrypt_first:
                assert same_limbs(src.decrypt_limbs(ck), src_limbs, mode), what


@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9])
def test_biguint_mul_add_value_aliased(sim, n, mode):
    """the column form of a + a * a, and of a + a * a.clone(), decrypted with its carries resolved on the host"""
    ctx, ck = sim
    rng = random.Random(0xB17 * n + mode)
    for al in limb_values(n, rng)[: 2 if n <= 3 else 1]:
        a = big(al, ck)
        want = R.from_limbs(R.biguint_add(al, mul_ref(al, al, mode)))
        assert a.mul_add_value(a, a, ck, mode) == want, (n, mode)
        assert a.mul_add_value(a.clone(), a, ck, mode) == want, (n, mode, "clone")


# ------------------------------------------------------------------------------- what only the glue decides
@pytest.mark.parametrize("bits", [6, 8, 18, 32, 34, 64, 66])
def test_scalar_words_longer_than_the_value(sim, bits):
    """the _words forms with more words than the operand has: the clear value is taken mod 2^bits by the
    wrapping ops, at its full value by / and % (a divisor above every value: quotient 0, remainder x)"""
    ctx, ck = sim
    rng = random.Random(0x3075 + bits)
    M = 1 << bits
    lib = _lib.load()
    x = rng.getrandbits(bits) | 1
    X = enc(x, ck, bits)

    def words_op(fn, c, nwords):
        w = (C.c_uint64 * nwords)(*[(c >> (64 * i)) & (2**64 - 1) for i in range(nwords)])
        h = C.c_void_p()
        _lib.check(getattr(lib, fn)(ctx.handle, X.handle, w, nwords, C.byref(h)))
        return FheUint._wrap(h, bits)

    nwords = (bits + 63) // 64 + 2
    big_c = rng.getrandbits(64 * nwords) | 1 << (64 * nwords - 1) | 1
    small_c = rng.getrandbits(max(2, bits // 2)) | 1
    for c in (big_c, small_c):
        assert words_op("fhe_radix_scalar_and_words", c, nwords).decrypt(ck) == x & c & (M - 1), (bits, hex(c))
        assert words_op("fhe_radix_scalar_add_words", c, nwords).decrypt(ck) == (x + c) % M, (bits, hex(c))
        assert words_op("fhe_radix_scalar_mul_words", c, nwords).decrypt(ck) == (x * c) % M, (bits, hex(c))
        assert words_op("fhe_radix_scalar_div_words", c, nwords).decrypt(ck) == x // c, (bits, hex(c))
        assert words_op("fhe_radix_scalar_rem_words", c, nwords).decrypt(ck) == x % c, (bits, hex(c))
    assert X.scalar_mul_add(big_c, small_c).decrypt(ck) == (x * big_c + small_c) % M


@pytest.mark.parametrize("bits", [6, 8, 18, 32, 34, 64, 66])
def test_shift_amount_of_another_width(sim, bits):
    """a narrower amount counts as zero-extended, a wider one is read at its full width before the reduction
    mod the width (test_radix_widths_gpu.py::test_amount_of_another_width on the GPU)"""
    ctx, ck = sim
    rng = random.Random(0x5417 + bits)
    M = 1 << bits
    x = rng.getrandbits(bits) | 1 | 1 << (bits - 1)
    X = enc(x, ck, bits)
    for abits in (2, 4, bits - 2, bits + 2, bits + 32, 2 * bits + 2):
        for amount in (rng.getrandbits(abits), (1 << abits) - 1, 1 << (abits - 1)):
            A = enc(amount, ck, abits)
            s = amount % bits
            assert (X >> A).decrypt(ck) == x >> s, (bits, abits, amount)
            assert (X << A).decrypt(ck) == (x << s) % M, (bits, abits, amount)


def test_glue_refusals(sim):
    ctx, ck = sim
    a, b = enc(5, ck, 8), enc(3, ck, 10)
    for f in (lambda: a + b, lambda: a * b, lambda: a.lt(b), lambda: a // b, lambda: a.div_rem(b), lambda: a.min(b)):
        with pytest.raises(FheError, match="same bit width"):
            f()
    for f in (lambda: a // 0, lambda: a % 0):
        with pytest.raises(FheError, match="division by zero"):
            f()
    h = C.c_void_p()
    zero = (C.c_uint64 * 3)(0, 0, 0)
    lib = _lib.load()
    assert lib.fhe_radix_scalar_div_words(ctx.handle, a.handle, zero, 3, C.byref(h)) != 0
    assert lib.fhe_radix_scalar_rem_words(ctx.handle, a.handle, zero, 3, C.byref(h)) != 0
    assert (a + a).decrypt(ck) == 10  # the context is usable after each refusal


def test_simulated_context_refuses_what_needs_a_device_or_a_key(sim):
    """export and serialize, digest and re-randomize, both compress forms and every expand, random, broadcast,
    the raw pbs / keyswitch / pbs_lincomb, every key install and the signer: FHE_ERR_INVALID, a message that names
    the simulated context, and the context still works"""
    import numpy as np
    from fhe_sign import Schnorr
    ctx, ck = sim
    x = FheUint8.try_encrypt(0xA5, ck)
    B = BigUintFHE.new(0x1234567890ABCDEF, ck)
    cts = np.zeros((2, 2049), np.uint64)
    lib = _lib.load()
    null = C.c_void_p()

    def raw(name, *args):
        def call():
            _lib.check(getattr(lib, name)(ctx.handle, *args))
        return call

    refused = {
        "export": x.export, "serialize": x.serialize, "biguint serialize": B.serialize,
        "deserialize": lambda: FheUint8.deserialize(b"\0" * 64),
        "digest": x.digest, "biguint digest": B.digest,
        "re_randomize": lambda: x.re_randomize(b"\1" * 32), "biguint re_randomize": lambda: B.re_randomize(b"\1" * 32),
        "compress": x.compress, "biguint compress": B.compress,
        "compress_switched": x.compress_switched, "biguint compress_switched": B.compress_switched,
        "compress_switched rekeyed": lambda: x.compress_switched(rekey=True),
        "random": lambda: FheUint8.random(b"\2" * 32), "random_below": lambda: FheUint8.random_below(200, b"\2" * 32),
        "biguint random": lambda: BigUintFHE.random(64, b"\2" * 32),
        "broadcast": lambda: FheUint.broadcast(x, 0, ctx), "biguint broadcast": lambda: BigUintFHE.broadcast(B, 0, ctx),
        "pbs": lambda: ctx.pbs(cts, 0), "keyswitch": lambda: ctx.keyswitch(cts),
        "pbs_lincomb": lambda: ctx.pbs_lincomb(cts, [([(0, 1)], 0)], [0]),
        "set_server_key": raw("fhe_set_server_key", null), "set_server_key_seeded": raw("fhe_set_server_key_seeded", null),
        "set_compression_key": raw("fhe_set_compression_key", null),
        "set_compression_key_seeded": raw("fhe_set_compression_key_seeded", null),
        "set_public_key": raw("fhe_set_public_key", null), "set_rekey_key": raw("fhe_set_rekey_key", null),
        "seeded expand": raw("fhe_seeded_expand_radix", null, C.byref(null)),
        "seeded expand biguint": raw("fhe_seeded_expand_biguint", null, C.byref(null)),
        "compressed expand": raw("fhe_compressed_expand_radix", null, C.byref(null)),
        "compressed expand biguint": raw("fhe_compressed_expand_biguint", null, C.byref(null)),
        "switched expand": raw("fhe_switched_expand_radix", null, C.byref(null)),
        "switched expand biguint": raw("fhe_switched_expand_biguint", null, C.byref(null)),
        "compact expand": raw("fhe_compact_list_expand_radix", null, 0, C.byref(null)),
        "compact expand biguint": raw("fhe_compact_list_expand_biguint", null, 0, C.byref(null)),
        "signer": lambda: Schnorr().sign_fhe_with_k0(b"m", 7, 11, B, ck, COMPAT),
    }
    for name, call in refused.items():
        with pytest.raises(FheError, match="simulated context") as e:
            call()
        assert e.value.code == FHE_ERR_INVALID, name
        assert (x + x).decrypt(ck) == (2 * 0xA5) % 256, name


# --------------------------------------------------------------------------------------------- the audit
def test_audit_sees_what_the_label_misses(sim):
    """x * x: every diagonal block product is a lookup of 4 x_i + x_i; x & x: every block.  One slot with
    coefficient 5 is 25 units, where the label (4^2 + 1^2) says 17."""
    ctx, ck = sim
    x = 0x9C3B5A17
    for name, f, want in (("mul", lambda X: X * X, x * x % 2**32), ("and", lambda X: X & X, x)):
        X = FheUint32.try_encrypt(x, ck)
        noise_audit(ctx, reset=True)
        assert f(X).decrypt(ck) == want
        max_label, max_merged, n_above = noise_audit(ctx)
        assert max_merged == K_MAX_NOISE and n_above > 0 and max_label < K_MAX_NOISE, (name, max_label, max_merged, n_above)


def test_audit_independent_operands(sim):
    """with no slot named twice the merged noise is the label: every op on independent operands -- all but the
    encrypted division, which forms 2 d and 3 d as d + d and d + d + d itself (merged 4 and 9 where the labels say
    2 and 3: small, and counted), so it is held to the budget and to its own largest label instead"""
    ctx, ck = sim
    rng = random.Random(0xA0D17)
    noise_audit(ctx, reset=True)
    pairs = {}
    for bits in (8, 34):
        x, y = rng.getrandbits(bits) | 1, rng.getrandbits(bits) | 1
        pairs[bits] = (x, y, enc(x, ck, bits), enc(y, ck, bits))
        x, y, X, Y = pairs[bits]
        for op in sorted(set(BINARY) - {"div", "rem"}):
            assert BINARY[op][1](X, Y).decrypt(ck) == BINARY[op][0](x, y, bits), (bits, op)
    al, bl, kl = ([rng.getrandbits(32) | 1 for _ in range(3)] for _ in range(3))
    for mode in (COMPAT, FAST):
        got = big(al, ck).mul_add(big(bl, ck), big(kl, ck), mode).decrypt_limbs(ck)
        assert same_limbs(got, R.biguint_add(kl, mul_ref(al, bl, mode)), mode)
        got = big(al, ck).add(big(bl, ck), mode).decrypt_limbs(ck)
        assert got == R.biguint_add(al, bl)
    max_label, max_merged, n_above = noise_audit(ctx, reset=True)
    assert n_above == 0 and max_merged == max_label <= K_MAX_NOISE, (max_label, max_merged, n_above)
    assert stats(ctx)[0] > 0
    for bits, (x, y, X, Y) in pairs.items():
        q, r = X.div_rem(Y)
        assert (q.decrypt(ck), r.decrypt(ck)) == (x // y, x % y)
    max_label, max_merged, n_above = noise_audit(ctx)
    assert n_above > 0 and max_merged <= max_label <= K_MAX_NOISE, (max_label, max_merged, n_above)
