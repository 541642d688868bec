"""Handle ownership on the CPU: a radix, BigUintFHE or column-form handle is a value of the context that made it,
and every entry point that takes a context refuses a handle made under another one with FHE_ERR_INVALID and a
message that says "another context" -- before anything is recorded, staged, launched or read.

Two or three simulated contexts (fhe_host_sim_ctx_create) are live at once.  Every host-mode pool hands out the
same placeholder addresses, so without the check context B finds its OWN plaintext shadow under a block of A
(a wrong value, no error), and a block that is pending in A carries an index into A's graph that B's engine
would follow into its own list (an out-of-bounds host read).  The simulated contexts go through the engine check
that the device contexts go through; the device-only entry points are tests/test_handle_owner_gpu.py's.

What is compared: statuses and messages of the refusals; fhe_ctx_stats and fhe_ctx_noise_audit of both contexts
around each refusal (equal); and exact equality with Python integers of what both contexts compute before and
after (wrapping radix semantics, oracle/ref_semantics.py for the BigUintFHE limbs)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import ref_semantics as R
from seeded_key_ref import refnv
from fhe_sign import (COMPAT, FAST, BigUintFHE, ClientKey, CompressedFheUint, FheError, FheUint, SimContext,
                      SimKey, _lib, default_params, generate_keys, noise_audit, set_server_key, stats)

FHE_ERR_INVALID = -1
FHE_ERR_UNSUPPORTED = -5
BITS = 16
M = (1 << BITS) - 1
CK = SimKey()
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fhe_rocm.h")


def lib():
    return _lib.load()


def last_error():
    return lib().fhe_last_error().decode()


class Under:
    """`with Under(ctx):` -- the operators' context for the block, as set_server_key selects it"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        set_server_key(self.ctx)
        return self.ctx

    def __exit__(self, *exc):
        set_server_key(None)


@pytest.fixture(scope="module")
def two():
    a, b = SimContext(), SimContext()
    yield a, b
    set_server_key(None)
    a.close()
    b.close()


def words(v, n=1):
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(n)], dtype=np.uint64)


def wp(w):
    return w.ctypes.data_as(C.POINTER(C.c_uint64))


# ----------------------------------------------------------------------------------- the table
# entry point -> (operands, call).  operands: (name in the C prototype, kind) in order, kind "R" a 16-bit radix,
# "B" a 2-limb BigUintFHE, "C" a column form; call(ctx handle, the operands' handles, out) -> status.
# `out` makes a fresh NULL output handle and remembers it: a refusal must leave it NULL.
W1, W3 = words(0x1234), words(3)
LIMBS = (C.c_uint32 * 8)()
NLIMBS = C.c_size_t()
WBUF = words(0, 4)
ABUF = words(0, 256)


def _bin(fn):
    return ((("a", "R"), ("b", "R")), lambda c, h, out: getattr(lib(), fn)(c, h[0], h[1], out()))


def _scalar(fn, s):
    return ((("a", "R"),), lambda c, h, out: getattr(lib(), fn)(c, h[0], s, out()))


def _wordsop(fn, w):
    return ((("a", "R"),), lambda c, h, out: getattr(lib(), fn)(c, h[0], wp(w), w.size, out()))


def _big(fn, names, mode):
    return (tuple((n, "B") for n in names), lambda c, h, out: getattr(lib(), fn)(c, *h, mode, out()))


SIMULATED = {
    **{f"fhe_radix_{n}": _bin(f"fhe_radix_{n}")
       for n in ("add", "sub", "mul", "min", "max", "lt", "bitand", "div", "rem")},
    "fhe_radix_divrem": ((("a", "R"), ("b", "R")),
                         lambda c, h, out: lib().fhe_radix_divrem(c, h[0], h[1], out(), out())),
    "fhe_radix_shr": ((("a", "R"), ("amount", "R")), lambda c, h, out: lib().fhe_radix_shr(c, h[0], h[1], out())),
    "fhe_radix_shl": ((("a", "R"), ("amount", "R")), lambda c, h, out: lib().fhe_radix_shl(c, h[0], h[1], out())),
    "fhe_radix_scalar_and": _scalar("fhe_radix_scalar_and", 0xF0F),
    "fhe_radix_scalar_shr": _scalar("fhe_radix_scalar_shr", 3),
    "fhe_radix_scalar_shl": _scalar("fhe_radix_scalar_shl", 3),
    "fhe_radix_scalar_add": _scalar("fhe_radix_scalar_add", 77),
    "fhe_radix_scalar_mul": _scalar("fhe_radix_scalar_mul", 5),
    "fhe_radix_scalar_div": _scalar("fhe_radix_scalar_div", 7),
    "fhe_radix_scalar_rem": _scalar("fhe_radix_scalar_rem", 7),
    "fhe_radix_scalar_and_words": _wordsop("fhe_radix_scalar_and_words", W1),
    "fhe_radix_scalar_add_words": _wordsop("fhe_radix_scalar_add_words", W1),
    "fhe_radix_scalar_mul_words": _wordsop("fhe_radix_scalar_mul_words", W3),
    "fhe_radix_scalar_div_words": _wordsop("fhe_radix_scalar_div_words", W3),
    "fhe_radix_scalar_rem_words": _wordsop("fhe_radix_scalar_rem_words", W3),
    "fhe_radix_scalar_mul_add_words": ((("a", "R"),), lambda c, h, out: lib().fhe_radix_scalar_mul_add_words(
        c, h[0], wp(W3), 1, wp(W1), 1, out())),
    "fhe_radix_cast": _scalar("fhe_radix_cast", 34),
    "fhe_radix_decrypt": ((("x", "R"),), lambda c, h, out: lib().fhe_radix_decrypt(c, None, h[0], wp(WBUF), 4)),
    "fhe_radix_rem_pseudo_mersenne": ((("a", "R"),), lambda c, h, out: lib().fhe_radix_rem_pseudo_mersenne(
        c, h[0], 8, wp(W3), 1, out())),
    "fhe_radix_scalar_mul_add_rem_pseudo_mersenne": (
        (("a", "R"),), lambda c, h, out: lib().fhe_radix_scalar_mul_add_rem_pseudo_mersenne(
            c, h[0], wp(W3), 1, wp(W3), 1, 8, wp(W3), 1, out())),
    "fhe_radix_scalar_mul_add_columns": ((("a", "R"),), lambda c, h, out: lib().fhe_radix_scalar_mul_add_columns(
        c, h[0], wp(W3), 1, wp(W1), 1, out())),
    "fhe_columns_decrypt": ((("x", "C"),), lambda c, h, out: lib().fhe_columns_decrypt(c, None, h[0], wp(WBUF), 4)),
    "fhe_columns_rem_pseudo_mersenne": ((("x", "C"),), lambda c, h, out: lib().fhe_columns_rem_pseudo_mersenne(
        c, h[0], 32, wp(W3), 1, out())),
    "fhe_biguint_decrypt": ((("x", "B"),), lambda c, h, out: lib().fhe_biguint_decrypt(
        c, None, h[0], LIMBS, 8, C.byref(NLIMBS))),
    # the launch trace's read-only hooks: an address means something under its own context only
    "fhe_radix_block_addrs": ((("x", "R"),), lambda c, h, out: lib().fhe_radix_block_addrs(
        c, h[0], wp(ABUF), None, ABUF.size, C.byref(NLIMBS))),
    "fhe_biguint_block_addrs": ((("x", "B"),), lambda c, h, out: lib().fhe_biguint_block_addrs(
        c, h[0], wp(ABUF), None, ABUF.size, C.byref(NLIMBS))),
}
for _mode, _tag in ((COMPAT, "compat"), (FAST, "fast")):
    SIMULATED[f"fhe_biguint_add/{_tag}"] = _big("fhe_biguint_add", "ab", _mode)
    SIMULATED[f"fhe_biguint_mul/{_tag}"] = _big("fhe_biguint_mul", "ab", _mode)
    SIMULATED[f"fhe_biguint_mul_add/{_tag}"] = _big("fhe_biguint_mul_add", "abk", _mode)
    SIMULATED[f"fhe_biguint_mul_add_columns/{_tag}"] = _big("fhe_biguint_mul_add_columns", "abk", _mode)

# refuse a simulated context before they look at the handle: tests/test_handle_owner_gpu.py, on device contexts
DEVICE_ONLY = {
    "fhe_radix_export", "fhe_radix_serialize", "fhe_biguint_serialize", "fhe_radix_compress", "fhe_biguint_compress",
    "fhe_radix_compress_switched", "fhe_biguint_compress_switched", "fhe_radix_compress_switched_rekeyed",
    "fhe_biguint_compress_switched_rekeyed", "fhe_radix_rerandomize", "fhe_biguint_rerandomize", "fhe_radix_digest",
    "fhe_biguint_digest", "fhe_rerand_context_add_radix", "fhe_rerand_context_add_biguint", "fhe_ctx_broadcast_radix",
    "fhe_ctx_broadcast_biguint", "fhe_schnorr_sign_fhe_with_k0", "fhe_schnorr_sign_fhe_with_k0_rerand",
    "fhe_schnorr_sign_fhe_with_k0_batch", "fhe_schnorr_sign_fhe_with_k0_reduced",
    "fhe_schnorr_sign_fhe_with_k0_rerand_reduced", "fhe_schnorr_sign_fhe_with_k0_batch_reduced", "fhe_schnorr_eval_s",
    "fhe_schnorr_eval_s_public",
}
# entry points with a context and a handle that provably touch no slot and hand nothing of the handle on: none
NO_SLOT_READ = set()


def header_entry_points():
    """every function of the header with an fhe_ctx* parameter and a radix / BigUintFHE / column-form INPUT"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    found = {}
    for m in re.finditer(r"\b(?:int|void)\s+(fhe_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        name, params = m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]
        if not any(re.match(r"(const )?fhe_ctx\s*\*", p) for p in params):
            continue
        # an input: a const handle (or an array of them), or the in-out handle of a broadcast (fhe_radix** x)
        ins = [p for p in params if re.match(r"const fhe_(radix|biguint|columns)\s*\*", p) or
               re.match(r"fhe_(radix|biguint|columns)\s*\*\*\s*x$", p)]
        if ins:
            found[name] = ins
    return found


def test_every_handle_taking_entry_point_is_classified():
    found = header_entry_points()
    assert len(found) >= 60 and {"fhe_radix_add", "fhe_ctx_broadcast_radix"} <= set(found), "the parser lost the header"
    table = {n.split("/")[0] for n in SIMULATED}
    classes = (table, DEVICE_ONLY, NO_SLOT_READ)
    for name in sorted(found):
        assert sum(name in c for c in classes) == 1, f"{name}{found[name]} is not classified (exactly one class)"
    for name in sorted(table | DEVICE_ONLY | NO_SLOT_READ):
        assert name in found, f"{name} is classified but the header has no such handle-taking entry point"
    # the table's operand names are the prototypes'
    for key, (operands, _) in SIMULATED.items():
        protos = [re.sub(r".*\*\s*", "", p) for p in found[key.split("/")[0]]]
        assert [n for n, _ in operands] == protos, (key, protos)


# ----------------------------------------------------------------------------------- values
RA1, RA2, RB1, RB2 = 0x1234, 0x0101, 0xBEEF, 0x0F0F
BL = {"a": [0x89ABCDEF, 0x01234567], "b": [0x0BADF00D, 0xFEEDFACE], "k": [0x13572468, 0x24681357]}
BV = {n: R.from_limbs(l) for n, l in BL.items()}
DESTROY = {"R": "fhe_radix_destroy", "B": "fhe_biguint_destroy", "C": "fhe_columns_destroy"}


def big(limbs):
    return BigUintFHE.new(R.from_limbs(limbs), CK)


def columns_of(ctx, a, b, k, mode=FAST):
    h = C.c_void_p()
    _lib.check(lib().fhe_biguint_mul_add_columns(ctx.handle, a.handle, b.handle, k.handle, mode, C.byref(h)))
    return h


def columns_value(ctx, h):
    bits = C.c_uint32()
    _lib.check(lib().fhe_columns_bits(h, C.byref(bits)))
    w = words(0, (bits.value + 63) // 64)
    _lib.check(lib().fhe_columns_decrypt(ctx.handle, None, h, wp(w), w.size))
    return sum(int(x) << (64 * i) for i, x in enumerate(w)), bits.value


class Made:
    """a value and what it must decrypt to under its maker (an integer; column forms: modulo their width)"""

    def __init__(self, kind, obj, want):
        self.kind, self.obj, self.want = kind, obj, want

    @property
    def handle(self):
        return self.obj if self.kind == "C" else self.obj.handle

    def check(self, ctx):
        with Under(ctx):
            if self.kind == "R":
                assert self.obj.decrypt(CK) == self.want
            elif self.kind == "B":
                assert self.obj.to_biguint(CK) == self.want
            else:
                got, bits = columns_value(ctx, self.obj)
                assert got == self.want % (1 << bits)

    def free(self):
        if self.kind == "C" and self.obj:
            lib().fhe_columns_destroy(self.obj)
            self.obj = None


def make(ctx, kind, form="computed", v1=RA1, v2=RA2):
    """a value under ctx whose producers are pending: nothing of it has been read"""
    with Under(ctx):
        if kind == "R":
            x1, x2 = FheUint.try_encrypt(v1, CK, bits=BITS), FheUint.try_encrypt(v2, CK, bits=BITS)
            return Made("R", (x1 * x2) * x2 + x1, (v1 * v2 * v2 + v1) & M)
        a, b, k = big(BL["a"]), big(BL["b"]), big(BL["k"])
        if kind == "C":
            return Made("C", columns_of(ctx, a, b, k), BV["k"] + BV["a"] * BV["b"])
        if form == "sum":  # carries a sum's column form: lazy entries over both operands' blocks
            return Made("B", a.add(b, FAST), BV["a"] + BV["b"])
        if form == "product":  # carries an exact product's block-product columns
            return Made("B", a.mul(b, FAST), BV["a"] * BV["b"])
        compat = R.biguint_add(R.biguint_mul(BL["a"], BL["b"]), BL["k"])
        return Made("B", a.mul(b, COMPAT).add(k, COMPAT), R.from_limbs(compat))


def snapshot(*ctxs):
    return [(stats(c), noise_audit(c)) for c in ctxs]


def refused(rc, operand=None):
    assert rc == FHE_ERR_INVALID, (rc, last_error())
    msg = last_error()
    assert "another context" in msg, msg
    if operand:
        assert f"operand {operand} " in msg, msg


def chain_ref(v1, v2):
    t = ((v1 + v2) * v1 - v2) & M
    return (min(t, (v1 << 3) & M) + (v2 >> 1)) & M


def short_chain(ctx, v1, v2):
    """a short chain of the kind in test_sim_context.py, left pending: (value, expected)"""
    with Under(ctx):
        x, y = FheUint.try_encrypt(v1, CK, bits=BITS), FheUint.try_encrypt(v2, CK, bits=BITS)
        return ((x + y) * x - y).min(x << 3) + (y >> 1), chain_ref(v1, v2)


class Outs:
    """fresh NULL output handles of one call; destroyed by kind when the call made them"""

    def __init__(self):
        self.h = []

    def __call__(self):
        self.h.append(C.c_void_p())
        return C.byref(self.h[-1])

    def all_null(self):
        return all(o.value is None for o in self.h)

    def destroy(self, name):
        kind = "C" if "_columns" in name and "decrypt" not in name and "rem_pseudo" not in name else (
            "B" if name.startswith("fhe_biguint") else "R")
        for o in self.h:
            if o.value:
                getattr(lib(), DESTROY[kind])(o)


# ----------------------------------------------------------------------------------- the matrix
def forms_of(kind):
    return ("computed", "sum", "product") if kind == "B" else ("computed",)


@pytest.mark.parametrize("name", sorted(SIMULATED))
def test_foreign_operand_is_refused(two, name):
    """each operand position in turn foreign, pending in its maker and already flushed there (BigUintFHE: also a
    sum and a product, whose column forms are lazy blocks over foreign slots): FHE_ERR_INVALID naming the operand,
    no output, statistics of both contexts unchanged, and both pending graphs exact afterwards"""
    A, B = two
    operands, call = SIMULATED[name]
    chain_a, want_a = short_chain(A, 0x0123, 0x4567)
    chain_b, want_b = short_chain(B, 0x89AB, 0x00CD)  # B has a pending graph of its own
    native = [make(B, kind, v1=RB1, v2=RB2) for _, kind in operands]
    for pos, (opname, kind) in enumerate(operands):
        for form in forms_of(kind):
            for state in ("pending", "flushed"):
                foreign = make(A, kind, form)
                if state == "flushed":
                    foreign.check(A)
                    with Under(A):
                        assert chain_a.decrypt(CK) == want_a
                    chain_a, want_a = short_chain(A, 0x0123, 0x4567)  # A's graph pending again
                handles = [foreign.handle if i == pos else native[i].handle for i in range(len(operands))]
                outs = Outs()
                before = snapshot(A, B)
                refused(call(B.handle, handles, outs), opname)
                assert outs.all_null(), (name, opname, form, state)
                assert snapshot(A, B) == before, (name, opname, form, state)
                foreign.check(A)  # what was pending in A computes the right value
                foreign.free()
    # the same call with every operand B's own goes through, and both contexts' earlier graphs are exact
    outs = Outs()
    assert call(B.handle, [m.handle for m in native], outs) == 0, last_error()
    outs.destroy(name)
    for m in native:
        m.check(B)
        m.free()
    with Under(A):
        assert chain_a.decrypt(CK) == want_a
    with Under(B):
        assert chain_b.decrypt(CK) == want_b


def test_contextless_views_of_a_foreign_value_stay_foreign(two):
    """fhe_biguint_to_radix, fhe_biguint_digit, fhe_radix_clone and fhe_radix_cast(NULL, ..) take no context and
    stay as they are; what they give shares the maker's slots, so B refuses it as it refuses the original"""
    A, B = two
    foreign = make(A, "B", "sum")
    views = {"to_radix": foreign.obj.to_radix(64), "digit": foreign.obj.digits[1],
             "clone": foreign.obj.to_radix(64).clone()}
    h = C.c_void_p()
    _lib.check(lib().fhe_radix_cast(None, views["digit"].handle, 34, C.byref(h)))
    views["cast"] = FheUint._wrap(h, 34)
    for what, v in views.items():
        before = snapshot(A, B)
        refused(lib().fhe_radix_decrypt(B.handle, None, v.handle, wp(WBUF), 4), "x")
        out = C.c_void_p()
        refused(lib().fhe_radix_scalar_add(B.handle, v.handle, 1, C.byref(out)), "a")
        assert out.value is None and snapshot(A, B) == before, what
    with Under(A):
        assert views["to_radix"].decrypt(CK) == foreign.want % (1 << 64)
        assert views["digit"].decrypt(CK) == (foreign.want >> 32) & 0xFFFFFFFF
    foreign.check(A)


def test_trivial_values_cross_freely(two):
    A, B = two
    with Under(A):
        t = FheUint.encrypt_trivial(0x0F0F, bits=BITS)
        ta = FheUint.try_encrypt(1, CK, bits=BITS) + t
    with Under(B):
        b1 = FheUint.try_encrypt(RB1, CK, bits=BITS)
        assert t.decrypt(CK) == 0x0F0F
        assert (b1 + t).decrypt(CK) == (RB1 + 0x0F0F) & M
        assert (t * b1).decrypt(CK) == (RB1 * 0x0F0F) & M
        assert (b1 & t).decrypt(CK) == RB1 & 0x0F0F
        assert (t + t).decrypt(CK) == 0x1E1E  # no slot anywhere: folds on the host, under any context
    with Under(A):
        assert ta.decrypt(CK) == 0x0F10


# ----------------------------------------------------------------------------------- the parent's two failures
def test_decrypt_under_another_context_is_refused_not_that_contexts_value():
    """before the check: both pools hand out the same placeholder addresses, so B's shadow answered for A's
    block -- a1.decrypt under B gave 0xbeef, and a1 + a2 under B gave B's own b1 + b2"""
    A, B = SimContext(), SimContext()
    try:
        with Under(A):
            a1, a2 = FheUint.try_encrypt(0x1234, CK, bits=BITS), FheUint.try_encrypt(0x0101, CK, bits=BITS)
        with Under(B):
            b1, b2 = FheUint.try_encrypt(0xBEEF, CK, bits=BITS), FheUint.try_encrypt(0x0F0F, CK, bits=BITS)
            with pytest.raises(FheError, match="another context") as e:
                a1.decrypt(CK)
            assert e.value.code == FHE_ERR_INVALID
            with pytest.raises(FheError, match="operand a was made under another context"):
                a1 + a2
            with pytest.raises(FheError, match="operand b was made under another context"):
                b1 + a2
            assert (b1 + b2).decrypt(CK) == 0xCDFE
        with Under(A):
            assert a1.decrypt(CK) == 0x1234 and (a1 + a2).decrypt(CK) == 0x1335
    finally:
        set_server_key(None)
        A.close()
        B.close()


def test_pending_foreign_value_is_refused_without_reading_its_node():
    """B holds forty 256-bit values and nothing pending; A leaves p = (a1 * a2) * a2 + a1 pending.  p + b1 under B
    followed p's node index into B's empty list (a host crash: tools/engine_host_check.c shows it on the parent)"""
    A, B = SimContext(), SimContext()
    try:
        with Under(B):
            held = [FheUint.try_encrypt(i, CK, bits=256) for i in range(40)]
            b1 = FheUint.try_encrypt(0xBEEF, CK, bits=BITS)
        with Under(A):
            a1, a2 = FheUint.try_encrypt(0x1234, CK, bits=BITS), FheUint.try_encrypt(0x0101, CK, bits=BITS)
            p = (a1 * a2) * a2 + a1
        before = snapshot(A, B)
        with Under(B):
            with pytest.raises(FheError, match="operand a was made under another context"):
                p + b1
            with pytest.raises(FheError, match="operand b was made under another context"):
                b1 + p
        assert snapshot(A, B) == before
        with Under(A):
            assert p.decrypt(CK) == (0x1234 * 0x0101 * 0x0101 + 0x1234) & M
        with Under(B):
            assert held[39].decrypt(CK) == 39 and (b1 + b1).decrypt(CK) == (2 * 0xBEEF) & M
    finally:
        set_server_key(None)
        A.close()
        B.close()


# ----------------------------------------------------------------------------------- lifetimes
def test_handles_outlive_their_context():
    A, B = SimContext(), SimContext()
    try:
        with Under(A):
            a1 = FheUint.try_encrypt(0x1234, CK, bits=BITS)
            pend = a1 * a1 + a1  # pending when A goes
            big_a = big(BL["a"]).add(big(BL["b"]), FAST)
        with Under(B):
            b1 = FheUint.try_encrypt(RB1, CK, bits=BITS)
            chain_b, want_b = short_chain(B, 0x0777, 0x1001)
        A.close()
        before = snapshot(B)
        with Under(B):
            for x in (a1, pend):
                with pytest.raises(FheError, match="another context"):
                    x.decrypt(CK)
                with pytest.raises(FheError, match="operand b was made under another context"):
                    b1 + x
            with pytest.raises(FheError, match="another context"):
                big_a.decrypt_limbs(CK)
        assert snapshot(B) == before
        del a1, pend, big_a, x  # dropped after their context: no error
        Cx = SimContext()
        try:
            with Under(Cx):
                c1 = FheUint.try_encrypt(0x4321, CK, bits=BITS)
                assert (c1 * c1 + c1).decrypt(CK) == (0x4321 * 0x4321 + 0x4321) & M
            with Under(B):
                with pytest.raises(FheError, match="another context"):
                    c1.decrypt(CK)
                assert chain_b.decrypt(CK) == want_b
        finally:
            set_server_key(None)
            Cx.close()
    finally:
        set_server_key(None)
        B.close()


# ----------------------------------------------------------------------------------- parameters
BAD_MODULI = [(0x40000001, 4, "message_modulus"), (4, 0x40000001, "carry_modulus"), (0x80000000, 2, "message_modulus"),
              (2, 0, "carry_modulus"), (0, 4, "message_modulus"), (1, 16, "message_modulus"), (3, 4, "message_modulus"),
              (128, 1, "message_modulus")]
MSG_OFF, CARRY_OFF = 32 + 24, 32 + 28  # in a frame whose payload starts with the parameters (csrc/serial.cpp)


def with_moduli(msg, carry):
    p = default_params()
    p.message_modulus, p.carry_modulus = msg, carry
    return p


@pytest.mark.parametrize("msg,carry,named", BAD_MODULI)
def test_wrapped_and_degenerate_moduli_are_refused_at_key_generation(msg, carry, named):
    """0x40000001 * 4 is 4 in 32 bits, 0x80000000 * 2 is 0, a zero carry modulus reaches a division: each modulus
    is checked on its own and the product is formed in 64 bits"""
    ck, sk = C.c_void_p(), C.c_void_p()
    rc = lib().fhe_generate_keys(C.byref(with_moduli(msg, carry)), 7, C.byref(ck), C.byref(sk))
    assert rc == FHE_ERR_UNSUPPORTED, (rc, last_error())
    assert named in last_error(), last_error()
    assert ck.value is None and sk.value is None


@pytest.fixture(scope="module")
def default_key():
    ck, _ = generate_keys(seed=0x0A11)
    return ck


@pytest.mark.parametrize("msg,carry", [(4, 4), (2, 2), (8, 8), (2, 1)])
def test_message_spaces_stay_accepted(msg, carry):
    ck, sk = generate_keys(with_moduli(msg, carry), seed=7)
    assert (ck.params.message_modulus, ck.params.carry_modulus) == (msg, carry)


@pytest.mark.parametrize("msg,carry,named", BAD_MODULI)
def test_wrapped_moduli_are_refused_at_deserialize(default_key, msg, carry, named):
    """the same fields in a serialized client key and in a seeded ciphertext, re-checksummed"""
    blobs = {"client key": (default_key.serialize(), ClientKey.deserialize),
             "seeded ciphertext": (CompressedFheUint.try_encrypt(5, default_key, bits=4, seed=b"\x01" * 32).serialize(),
                                   CompressedFheUint.deserialize)}
    for what, (blob, load) in blobs.items():
        assert struct.unpack_from("<II", blob, MSG_OFF) == (4, 4), what
        load(refnv(blob))  # the helper's checksum is the library's
        bad = bytearray(blob)
        struct.pack_into("<II", bad, MSG_OFF, msg, carry)
        with pytest.raises(FheError, match=named) as e:
            load(refnv(bytes(bad)))
        assert e.value.code == FHE_ERR_INVALID, what
