"""The radix ops on the GPU at widths that are not a power of two (odd block counts, 17 and 33 blocks, 258
bits), on classic and multi-bit keys: decrypted results against exact Python integers with tfhe's
conventions (wrapping arithmetic, shift amounts mod the value's width whatever the amount's own width,
x / 0 = all ones, x % 0 = x).  Every test issues all its ops before the first decryption, so the engine
runs them as one graph.  tests/test_radix_widths.py runs the same algorithms simulated on the CPU."""
import random

import pytest

from fhe_sign import FheUint, stats
from test_radix_gpu import keys  # noqa: F401  (the fixture: one classic and one multi-bit key per module)
from test_radix_widths import nbits_of

pytestmark = pytest.mark.gpu

WIDTHS = (6, 10, 34, 66)


def _uint(bits):
    """an FheUint class of this width (cast_into takes a class)"""
    return type(f"FheUint{bits}", (FheUint,), {"BITS": bits})


def _enc(v, ck, bits):
    return FheUint.try_encrypt(v, ck, bits=bits)


def _check(ck, pending):
    """pending: (what, expected value, ciphertext) -- decrypted only here, after every op was issued"""
    got = [(what, want, ct.decrypt(ck)) for what, want, ct in pending]
    bad = [(what, hex(want), hex(g)) for what, want, g in got if g != want]
    assert not bad, (len(bad), len(pending), bad[:6])


def test_shifts_by_encrypted_amount(keys):
    """value >> Enc(amount) and <<: amounts at and around the width and 2^nbits, and all ones -- the shift
    is by amount mod the width, where the barrel shifter alone would take amount mod 2^nbits"""
    ck, ctx = keys
    rng = random.Random(0x5A1F)
    p0, l0 = stats(ctx)
    pending = []
    for bits in WIDTHS:
        M = 1 << bits
        x = rng.getrandbits(bits) | 1 | M // 2
        X = _enc(x, ck, bits)
        for amt in (0, 1, bits - 1, bits, bits + 1, (1 << nbits_of(bits)) - 1, 2 * bits + 3, M - 1):
            A = _enc(amt, ck, bits)
            pending.append((("shr", bits, amt), x >> (amt % bits), X >> A))
            pending.append((("shl", bits, amt), (x << (amt % bits)) % M, X << A))
    _check(ck, pending)
    p1, l1 = stats(ctx)
    assert p1 > p0 and l1 > l0


OPS = ["add", "sub", "mul", "and", "andc", "shr", "shl", "min", "max", "lt", "divc", "remc", "div", "rem"]


def test_op_chains(keys):
    """Seeded chains of ops whose ciphertext outputs feed later ops, 10 steps at each width, every
    intermediate decrypted; encrypted divisors up to 34 bits; one cast down and back up between two of the
    widths."""
    ck, _ = keys
    rng = random.Random(0xC4A2)
    pending, used, last = [], set(), {}
    turn = 0  # the ops taken in turn across the widths (each one reached about three times), shuffled per width
    for bits in WIDTHS:
        M = (1 << bits) - 1
        vals = [rng.getrandbits(bits) for _ in range(3)] + [0, M]
        enc = [_enc(v, ck, bits) for v in vals]
        ops = []
        while len(ops) < 10:
            op = OPS[turn % len(OPS)]
            turn += 1
            if bits <= 34 or op not in ("div", "rem"):
                ops.append(op)
        rng.shuffle(ops)
        for step, op in enumerate(ops):
            i, j = rng.randrange(len(vals)), rng.randrange(len(vals))
            x, y, X, Y = vals[i], vals[j], enc[i], enc[j]
            c = rng.getrandbits(max(2, bits // 2)) | 1
            s = y % bits
            want, got = {
                "add": (lambda: ((x + y) & M, X + Y)), "sub": (lambda: ((x - y) & M, X - Y)),
                "mul": (lambda: ((x * y) & M, X * Y)), "and": (lambda: (x & y, X & Y)),
                "andc": (lambda: (x & c, X & c)),
                "shr": (lambda: (x >> s, X >> Y)), "shl": (lambda: ((x << s) & M, X << Y)),
                "min": (lambda: (min(x, y), X.min(Y))), "max": (lambda: (max(x, y), X.max(Y))),
                "lt": (lambda: (int(x < y), X.lt(Y))), "divc": (lambda: (x // c, X / c)),
                "remc": (lambda: (x % c, X % c)),
                "div": (lambda: (x // y if y else M, X // Y)), "rem": (lambda: (x % y if y else x, X % Y)),
            }[op]()
            pending.append(((bits, step, op, hex(x), hex(y), hex(c)), want, got))
            used.add(op)
            if op != "lt":  # feed the result into later steps
                vals.append(want)
                enc.append(got)
        k = max(range(5, len(vals)), key=lambda t: vals[t])  # the chain's largest result
        last[bits] = (vals[k], enc[k])
    assert used == set(OPS)
    v, V = last[34]
    down = V.cast_into(_uint(10))
    pending.append((("cast", 34, 10), v % (1 << 10), down))
    pending.append((("cast", 10, 34), v % (1 << 10), down.cast_into(_uint(34))))
    pending.append((("cast", 34, 66), v, V.cast_into(_uint(66))))
    _check(ck, pending)


def test_258_bits(keys):
    """258 bits (129 blocks): the ops of the 256-bit suite one block above it, a clear 40-bit divisor, and
    shifts whose amounts lie above the width -- and, for <<, above 2^nbits too: Enc(2^200 + 3) shifts by
    (2^200 + 3) mod 258, not by 3"""
    ck, _ = keys
    bits = 258
    rng = random.Random(258)
    M = 1 << bits
    x, y = rng.getrandbits(bits) | 1 | M // 2, rng.getrandbits(bits)
    d = rng.getrandbits(40) | 1 | 1 << 39
    X, Y = _enc(x, ck, bits), _enc(y, ck, bits)
    s1, s2 = bits + 5, (1 << 200) + 3
    assert s2 % bits != 3
    pending = [
        ("add", (x + y) % M, X + Y), ("sub", (x - y) % M, X - Y), ("lt", int(x < y), X.lt(Y)), ("gt", int(y < x), Y.lt(X)),
        ("min", min(x, y), X.min(Y)), ("max", max(x, y), X.max(Y)), ("and", x & y, X & Y),
        ("divc", x // d, X / d), ("remc", x % d, X % d),
        ("shr", x >> (s1 % bits), X >> _enc(s1, ck, bits)),
        ("shl", (x << (s2 % bits)) % M, X << _enc(s2, ck, bits)),
    ]
    _check(ck, pending)


def test_amount_of_another_width(keys):
    """fhe_radix_shr / _shl take an amount of any width: a narrower one is zero-extended (8-bit Enc(37) on a
    34-bit value shifts by 37 mod 34), a wider one is reduced from its own width (66-bit Enc(2^65 + 1)).
    Beside these: a 4-bit amount (it cannot reach 34: read as it is), an amount whose blocks are all public
    (encrypt_trivial) and one whose high blocks are (a 6-bit Enc(59) cast up to 34 bits)."""
    ck, _ = keys
    bits = 34
    rng = random.Random(34)
    M = 1 << bits
    x = rng.getrandbits(bits) | 1 | M // 2
    X = _enc(x, ck, bits)
    amounts = [(("enc", abits), amt, _enc(amt, ck, abits)) for abits, amt in ((8, 37), (66, (1 << 65) + 1))]
    for _, amt, _ in amounts:
        assert amt % bits != amt % 64  # the shifter's own 6 amount bits would shift by something else
    amounts += [(("enc", 4), 13, _enc(13, ck, 4)),
                (("trivial", bits), M - 3, FheUint.encrypt_trivial(M - 3, bits=bits)),
                (("cast", 6), 59, _enc(59, ck, 6).cast_into(_uint(bits)))]
    pending = []
    for what, amt, A in amounts:
        s = amt % bits
        pending.append((("shr",) + what, x >> s, X >> A))
        pending.append((("shl",) + what, (x << s) % M, X << A))
    _check(ck, pending)
