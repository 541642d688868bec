"""Operands that share blocks, on the GPU: every radix op on a value with itself, its clone and a cast round trip
of it; BigUintFHE sums and products with one operand on both sides -- all ops of a test recorded before the first
decryption, so they run as one schedule -- and the measurement behind the engine's merged noise budget: a block
that enters a lookup twice carries (sum of its coefficients)^2 of its variance, not the sum of their squares.
Expected values as tests/test_sim_context.py (the same cases on the CPU): exact Python integers."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import ref_semantics as R
from fhe_sign import (COMPAT, FAST, BigUintFHE, Context, FheUint, _lib, generate_keys, multi_bit_params, noise_audit,
                      set_server_key, tuning)

pytestmark = pytest.mark.gpu
K_MAX_NOISE = 25  # csrc/engine.h kMaxNoise
DELTA = 1 << 59


@pytest.fixture(scope="module", params=["classic", "multibit"])
def keys(request):
    ck, sk = generate_keys(multi_bit_params() if request.param == "multibit" else None, seed=0xA11A5)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    yield ck, ctx
    set_server_key(None)
    ctx.close()


@pytest.fixture(autouse=True)
def audit(keys):
    """no bootstrap of the test was recorded above the budget, counted on what is launched"""
    _, ctx = keys
    noise_audit(ctx, reset=True)
    yield
    assert noise_audit(ctx)[1] <= K_MAX_NOISE


def cast(x, bits):
    h = C.c_void_p()
    _lib.check(_lib.load().fhe_radix_cast(None, x.handle, bits, C.byref(h)))
    return FheUint._wrap(h, bits)


def alias_kinds(X):
    return (("self", X), ("clone", X.clone()), ("cast", cast(cast(X, X.bits + 6), X.bits)))


OPS = {
    "add": (lambda x, b: 2 * x % (1 << b), lambda X, Y: X + Y),
    "sub": (lambda x, b: 0, lambda X, Y: X - Y),
    "mul": (lambda x, b: x * x % (1 << b), lambda X, Y: X * Y),
    "and": (lambda x, b: x, lambda X, Y: X & Y),
    "min": (lambda x, b: x, lambda X, Y: X.min(Y)),
    "max": (lambda x, b: x, lambda X, Y: X.max(Y)),
    "lt": (lambda x, b: 0, lambda X, Y: X.lt(Y)),
    "shr": (lambda x, b: x >> (x % b), lambda X, Y: X >> Y),
    "shl": (lambda x, b: (x << (x % b)) % (1 << b), lambda X, Y: X << Y),
    "div": (lambda x, b: 1 if x else (1 << b) - 1, lambda X, Y: X // Y),
    "rem": (lambda x, b: 0, lambda X, Y: X % Y),
}


def matrix(ck, bits, ops, div_rem, seed):
    rng = random.Random(seed + bits)
    M = (1 << bits) - 1
    unread = []
    for x in (0, 1, M, 1 << (bits - 1), rng.getrandbits(bits) | 1 | 1 << (bits - 1)):
        X = FheUint.try_encrypt(x, ck, bits=bits)
        for kind, Y in alias_kinds(X):
            for op in ops:
                unread.append((OPS[op][1](X, Y), OPS[op][0](x, bits), (bits, hex(x), op, kind)))
            if div_rem:
                q, r = X.div_rem(Y)
                unread.append((q, 1 if x else M, (bits, hex(x), "div_rem q", kind)))
                unread.append((r, 0, (bits, hex(x), "div_rem r", kind)))
    for got, want, what in unread:  # the first host read: everything above is one schedule
        assert got.decrypt(ck) == want, what


@pytest.mark.parametrize("bits", [6, 8])
def test_aliasing_matrix_narrow(keys, bits):
    ck, _ = keys
    matrix(ck, bits, sorted(OPS), True, 0xA71A5)


def test_aliasing_matrix_34_bits(keys):
    ck, _ = keys
    matrix(ck, 34, ["add", "sub", "mul", "and", "min", "lt", "shr", "shl"], False, 0xA71A5)


def test_aliasing_karatsuba_64_bits(keys):
    """x * x and x + x where the product splits: the memo of halves and half sums sees one address twice"""
    ck, _ = keys
    with tuning(kara_min=8):
        matrix(ck, 64, ["mul", "add"], False, 0xCA7A)


def mul_ref(a, b, mode):
    return R.biguint_mul(a, b) if mode == COMPAT else R.to_u32_digits(R.from_limbs(a) * R.from_limbs(b))


def same_limbs(got, want, mode):
    return got == want if mode == COMPAT else R.from_limbs(got) == R.from_limbs(want)


@pytest.mark.parametrize("n", [2, 3])
def test_biguint_aliasing(keys, n):
    ck, _ = keys
    rng = random.Random(0xB16 * n)
    unread = []
    for al in ([0xFFFFFFFF] * n, [rng.getrandbits(32) | 1 << 31 for _ in range(n)]):
        bl = [rng.getrandbits(32) | 1 for _ in range(n)]
        a, b = BigUintFHE.new(R.from_limbs(al), ck), BigUintFHE.new(R.from_limbs(bl), ck)
        unread.append((a.add(a), R.biguint_add(al, al), COMPAT, (n, "a.add(a)")))
        for mode in (COMPAT, FAST):
            sq, pl = mul_ref(al, al, mode), mul_ref(al, bl, mode)
            unread.append((a.mul(a, mode), sq, mode, (n, mode, "a.mul(a)")))
            unread.append((a.mul_add(a, a, mode), R.biguint_add(al, sq), mode, (n, mode, "a.mul_add(a, a)")))
            P = a.mul(b, mode)
            unread.append((P.add(P), R.biguint_add(pl, pl), mode, (n, mode, "P + P")))
            unread.append((P.add(P.clone()), R.biguint_add(pl, pl), mode, (n, mode, "P + P.clone()")))
            del P
    for got, want, mode, what in unread:
        assert same_limbs(got.decrypt_limbs(ck), want, mode), what


def test_merged_variance_model(keys):
    """The one measurement behind the merged budget.  4,096 unit-noise blocks b (fresh encryptions through one
    identity bootstrap); 4 b + b of the SAME block against 4 b + b' of two blocks: the phase-error standard
    deviations are 5 sigma and sqrt(17) sigma, ratio sqrt(25 / 17) = 1.213.  With 4,096 samples each the estimated
    deviation has about 1.1 % relative error and the ratio about 1.6 %: 5 % is three standard errors.  Then the
    aliased inputs -- 25 units, where the label says 17 -- go through the diagonal block product's lookup,
    (x * x) & 3, without a decode failure."""
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    ck, ctx = keys
    dev = torch.device("cuda:0")
    count = 4096
    _, glwe = ck.export()
    S = torch.from_numpy(glwe.astype(np.int64)).to(dev)

    def phase(ct):
        return ct[:, 2048] - (ct[:, :2048] * S).sum(dim=1)

    def pbs(cts, table):
        lut = torch.full((count,), ctx.lut(table), dtype=torch.int32, device=dev)
        out = torch.empty((count, 2049), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        ctx.pbs_device(cts.data_ptr(), count, lut.data_ptr(), out.data_ptr())
        ctx.sync()
        return out

    m = np.random.default_rng(0xA11A5).integers(0, 4, count)
    ck.seed_encryption(0xA11, 100)
    fresh = torch.from_numpy(ck.encrypt_blocks(m).view(np.int64)).to(dev)
    b = pbs(fresh, list(range(16)))
    mt = torch.from_numpy(m).to(dev)
    assert bool((torch.remainder(torch.div(phase(b) + DELTA // 2, DELTA, rounding_mode="floor"), 16) == mt).all())
    other = torch.roll(torch.arange(count, device=dev), 1)  # b' = another block of the pool, never b itself
    aliased, independent = 4 * b + b, 4 * b + b[other]
    s_alias = float((phase(aliased) - 5 * mt * DELTA).to(torch.float64).std())
    s_indep = float((phase(independent) - (4 * mt + mt[other]) * DELTA).to(torch.float64).std())
    ratio = s_alias / s_indep
    print(f"\nmerged variance: 4b + b sigma 2^{math.log2(s_alias):.3f}, 4b + b' sigma 2^{math.log2(s_indep):.3f}, "
          f"ratio {ratio:.4f} (sqrt(25/17) = {math.sqrt(25 / 17):.4f})")
    assert abs(ratio / math.sqrt(25 / 17) - 1) < 0.05
    out = pbs(aliased.contiguous(), [((v >> 2) * (v & 3)) & 3 for v in range(16)])
    got = torch.remainder(torch.div(phase(out) + DELTA // 2, DELTA, rounding_mode="floor"), 16)
    assert int((got != (mt * mt) % 4).sum()) == 0
