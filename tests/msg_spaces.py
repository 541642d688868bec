"""Test-only table of the message spaces the suite pins besides the default 4 x 4, and the parameter structs of
the product and of the oracle at each.  The C ABI accepts any message_modulus in {2 .. 64} and carry_modulus in
{1 .. 64}, both powers of two, with product mc <= 64 (Params::from_c); keys, block encryption, lookup tables, the
raw bootstrap and the oblivious pseudo-random blocks take mc at run time, while the radix layer needs 4 x 4 exactly
(Params::radix_space).  Each space here is one at which something true at 4 x 4 (mc 16, delta 2^59, a box of 128
coefficients per value) is not.  Never used by the product."""
import oracle
from fhe_sign import default_params

CLASSIC, MULTIBIT = 1, 2
N = 2048

# (message_modulus, carry_modulus): why it is here
SPACES = {
    (2, 1): "mc 2: a box of 1024 coefficients, half-box 512; one message bit; oprf_max_bits = 1",
    (2, 2): "mc 4: tfhe-rs' 1_1",
    (4, 2): "mc 8: message and carry of different widths, mc below 16",
    (2, 8): "mc 16, delta as 4 x 4: LUT ids survive a re-key from 4 x 4 (context.cpp compares mc and delta); oprf_max_bits = 1",
    (8, 2): "mc 16, delta as 4 x 4, another split; oprf_max_bits = 3",
    (16, 1): "mc 16, no carry at all; oprf_max_bits = 4",
    (4, 8): "mc 32: the first space above the radix layer's 16-entry tables",
    (8, 8): "mc 64: box 32, half-box 16; Engine::beyond()'s special case; 64-entry tables",
    (64, 1): "mc 64 in one message: 6 OPRF bits",
}
DEFAULT = (4, 4)


def space_id(s):
    return f"{s[0]}x{s[1]}"


def mc_of(s):
    return s[0] * s[1]


def delta_of(s):
    return (1 << 63) // mc_of(s)


def box_of(s):
    """coefficients of the accumulator polynomial per message value"""
    return N // mc_of(s)


def oprf_max_bits(s):
    return s[0].bit_length() - 1


def product_params(space, n=16, grouping=CLASSIC):
    p = default_params()
    p.lwe_dimension = n
    p.grouping = grouping
    p.message_modulus, p.carry_modulus = space
    return p


def oracle_params(space, n=16, grouping=CLASSIC):
    p = oracle.default_params()
    p.n = n
    p.grouping = grouping
    p.message_modulus, p.carry_modulus = space
    return p


def tables(mc):
    """identity, an affine map with every output distinct, the constant mc - 1, reversal"""
    return [list(range(mc)), [(3 * m + 1) % mc for m in range(mc)], [mc - 1] * mc, [mc - 1 - m for m in range(mc)]]
