"""The radix ops at widths that are not a power of two, on the CPU through the simulating engine
(test_radix_sim.py's sim_radix): odd block counts, block counts between two powers of two, values that
straddle a 64-bit word, the first widths past narrow_cap's 16 live blocks and past residue_split's
64-block threshold, and the widest such width (4094).  Every comparison is exact equality against Python
integers (tfhe's semantics: wrapping arithmetic, shift amounts mod the width, x / 0 = all ones, x % 0 = x).

The encrypted shifts are the ops where the width itself enters the arithmetic: the barrel shifter reads
nbits = ceil(log2(width)) amount bits, and amount mod width differs from amount mod 2^nbits whenever the
width is not 2^nbits -- so the amount lists below are built to make the bits above nbits matter, and each
list is checked for that before it is used.

The simulator hook gives both operands the same width; an amount of another width than the value's is
pinned on the GPU (test_radix_widths_gpu.py)."""
import random

import pytest

from fhe_sign import tuning
from test_radix_sim import (ADD, AND, DIV_SCALAR, DIVREM, DIVREM_CLEAR, DIVREM_CLEAR_MIXED, LT, MIN, MUL, MUL_FULL,
                            SHL, SHR, SUB, expect, operands, sim_radix)

# bits: what the width reaches (blocks = bits / 2)
WIDTHS = {
    6: "3 blocks, odd; nbits 3: one 4-way stage and the odd top-bit stage; amounts 6, 7 alias",
    10: "5 blocks; nbits 4: two 4-way stages, no odd stage; amounts 10..15 alias",
    12: "6 blocks: even, not a power of two",
    14: "7 blocks, just below 16: only 14 and 15 alias",
    18: "9 blocks, just above 16: 14 of 32 amounts alias",
    34: "17 blocks: past narrow_cap's 16 live blocks, a carry prefix over more than 16 positions",
    62: "31 blocks: the widest value within one 64-bit word",
    66: "33 blocks: two words (word_bits / words_of); nbits 7",
    130: "65 blocks: past residue_split's 64-block threshold",
    258: "129 blocks: just above 256",
}
MAX_ODD = 4094  # 2047 blocks: the widest width that is not a power of two
NARROW = 18     # up to here the shifts take every amount below 2^nbits


def nbits_of(bits):
    """the barrel shifter's amount bits: ceil(log2(bits))"""
    return (bits - 1).bit_length()


def _check(op, bits, cases):
    bad = []
    for a, b in cases:
        got = sim_radix(op, bits, a, b)
        want = expect(op, bits, a, b)
        if (got if op == DIVREM else got[0]) != want:
            bad.append((hex(a), hex(b), got, want))
    assert not bad, (op, bits, len(bad), len(cases), bad[:4])


@pytest.mark.parametrize("bits", list(WIDTHS))
@pytest.mark.parametrize("op", [ADD, SUB, MUL, MUL_FULL, LT, AND, MIN, DIV_SCALAR])
def test_ops_at_width(bits, op):
    _check(op, bits, operands(bits, random.Random(1000 * op + bits), 12))


@pytest.mark.parametrize("bits", [b for b in WIDTHS if b <= 66])
def test_encrypted_divrem_at_width(bits):
    rng = random.Random(bits)
    M = 1 << bits
    _check(DIVREM, bits, operands(bits, rng, 12) + [(rng.getrandbits(bits), 0), (0, 0), (M - 1, 1)])


def _clear_divisors(bits, rng):
    M = 1 << bits
    ds = [1, 2, 3, 5, 7, M - 1, M // 2, M // 2 + 1, (1 << (bits // 2)) + 1, rng.getrandbits(bits) | 1 | M // 2,
          rng.getrandbits(bits // 3) | 1 | 1 << (bits // 3 - 1)]
    assert all(0 < d < M for d in ds)
    return ds


@pytest.mark.parametrize("residue", [0, 1, -1])
@pytest.mark.parametrize("bits", list(WIDTHS))
def test_clear_divrem_at_width(residue, bits):
    """a / d and a % d by a public d: the multiplier method (tuning scalar_div_residue 0), the residue
    split wherever it is valid (1), the size rule (-1: the default); plain dividends and ones whose odd
    blocks are public constants (DIVREM_CLEAR_MIXED)."""
    rng = random.Random(7 * bits + residue + 1)
    M = 1 << bits
    bad = []
    with tuning(scalar_div_residue=residue):
        for d in _clear_divisors(bits, rng):
            for a in (M - 1, 0, d - 1, d, rng.getrandbits(bits)):
                for op in (DIVREM_CLEAR, DIVREM_CLEAR_MIXED):
                    got = sim_radix(op, bits, a, d)
                    if got != (a // d, a % d):
                        bad.append((op, hex(a), hex(d), got))
    assert not bad, (residue, bits, len(bad), bad[:4])


def shift_amounts(bits, rng):
    """Amounts below 2^bits for a `bits`-wide shift.  Narrow widths: every s below 2^nbits, and for each
    an s + k * bits (k random, drawn until the amount's low nbits bits alone give another shift than the
    amount mod the width: the high amount bits matter).  Wider: the edges around the width and around
    2^nbits, the all-ones amount and random full-width ones."""
    M, nb = 1 << bits, nbits_of(bits)
    if bits <= NARROW:
        out = []
        for s in range(1 << nb):
            out.append(s)
            while True:
                amt = s + bits * rng.randrange(1, (M - 1 - s) // bits + 1)
                if amt % (1 << nb) != amt % bits:
                    break
            out.append(amt)
        return out
    return [0, 1, 2, 3, bits // 2, bits - 1, bits, bits + 1, (1 << nb) - 1, 1 << nb, 2 * bits + 3, M - 1] + \
        [rng.getrandbits(bits) | M // 2 for _ in range(3)]


def _shift_cases(bits, op):
    rng = random.Random(bits + 7 * op)
    M, nb = 1 << bits, nbits_of(bits)
    amounts = shift_amounts(bits, rng)
    assert all(0 <= s < M for s in amounts)
    assert len(amounts) == (2 << nb if bits <= NARROW else 15)
    # the list itself: at least half of it tells "mod the width" from "mod 2^nbits"
    telling = sum(s % (1 << nb) != s % bits for s in amounts)
    assert 2 * telling >= len(amounts), (bits, telling, len(amounts))
    values = [rng.getrandbits(bits) | 1 | M // 2] + ([M - 1] if bits <= NARROW else [])
    return [(a, s) for s in amounts for a in values]


@pytest.mark.parametrize("bits", list(WIDTHS) + [MAX_ODD])
@pytest.mark.parametrize("op", [SHR, SHL])
def test_encrypted_shifts_at_width(bits, op):
    """value >> Enc(amount) and << at every width: the shift is by the amount's value mod the width, the
    amount read at its full width (the values have their top and bottom bits set, so a shift off by any
    number of bits shows)."""
    _check(op, bits, _shift_cases(bits, op))


@pytest.mark.parametrize("op", [ADD, SUB, LT, AND, MIN])
def test_ops_at_max_odd_width(op):
    """4094 bits, as test_radix_ops_max_width_simulated at 4096"""
    rng = random.Random(MAX_ODD + op)
    M = 1 << MAX_ODD
    _check(op, MAX_ODD, [(M - 1, M - 1), (rng.getrandbits(MAX_ODD), rng.getrandbits(MAX_ODD)), (0, M - 1)])
