"""FheUint{8,32,64} and BigUintFHE: the reference's encrypted-integer surface over the C ABI.

Mirrors the operator set coset-io/fhe-sign uses on tfhe's high-level types
(src/biguint.rs:108-117,135-143,221-248; src/perf_test.rs:19-56) and the BigUintFHE struct
(src/biguint.rs:8-265).  Operators do not consume their inputs (Rust consumed them; callers
cloned, src/schnorr.rs:274).  The server side is an explicit Context (tfhe's thread-local
set_server_key, src/schnorr.rs:443, is `set_server_key(ctx)` here).
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np

from ._lib import CompressionParams, FheError, FheParams, check, load, ptr, serialize_with
from .core import RekeyKey, modulus_switch_mode

COMPAT = 0  # exact replay of src/biguint.rs:214-254 incl. the wrapping add at :247-249
FAST = 1    # true product/sum, single wide carry propagation
PUBLIC = 2  # signer only: e and k stay clear, s = e * Enc(d') + k as a wide scalar multiply-add

# secp256k1's moduli as 2^256 - c (FheUint.rem_pseudo_mersenne(256, c))
SECP256K1_N_C = 0x14551231950B75FC4402DA1732FC9BEBF  # the curve order n
SECP256K1_P_C = 2**32 + 977                          # the field prime p

_tls = threading.local()


def set_server_key(ctx) -> None:
    """tfhe::set_server_key (src/schnorr.rs:443): the context used by operators on this thread."""
    _tls.ctx = ctx


def _ctx():
    ctx = getattr(_tls, "ctx", None)
    if ctx is None:
        raise RuntimeError("no server key set on this thread (call set_server_key(ctx))")
    return ctx


def _hval(h):
    """the address of a handle (c_void_p or int)"""
    return h.value if isinstance(h, C.c_void_p) else h


def _words(value: int, bits: int) -> np.ndarray:
    n = (bits + 63) // 64
    v = value % (1 << bits)
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(n)], dtype=np.uint64)


class FheUint:
    BITS = 0

    def __init__(self, handle, bits=None):
        self._h = handle
        self.bits = bits or self.BITS

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_radix_destroy(self._h)
            self._h = None

    @classmethod
    def _wrap(cls, h, bits):
        kind = {8: FheUint8, 32: FheUint32, 64: FheUint64, 128: FheUint128, 256: FheUint256, 2: FheBool}.get(bits, FheUint)
        obj = kind.__new__(kind)
        FheUint.__init__(obj, h, bits)
        return obj

    @classmethod
    def try_encrypt(cls, value: int, client_key, bits=None):
        bits = bits or cls.BITS
        ctx = _ctx()
        w = _words(value, bits)
        h = C.c_void_p()
        check(load().fhe_radix_encrypt(ctx.handle, client_key.handle, ptr(w), bits, C.byref(h)))
        return cls._wrap(h, bits)

    encrypt = try_encrypt

    @classmethod
    def encrypt_trivial(cls, value: int, bits=None):
        bits = bits or cls.BITS
        w = _words(value, bits)
        h = C.c_void_p()
        check(load().fhe_radix_trivial(_ctx().handle, ptr(w), bits, C.byref(h)))
        return cls._wrap(h, bits)

    @classmethod
    def random(cls, seed=None, random_bits=None, bits=None):
        """tfhe-rs' generate_oblivious_pseudo_random(seed, random_bits) (fhe_radix_random): an encrypted value
        uniform in [0, 2^random_bits) (default: the whole width) that the server makes by itself on the GPU and
        only the client-key holder can read.  seed: 32 PUBLIC bytes; the same seed and key give the same words, so
        a seed serves one call.  None draws OS entropy -- refused under a communicator of more than one rank,
        where callers derive the seed (rerandomization_seed, ReRandomizationContext.seed)."""
        bits = bits or cls.BITS
        h = C.c_void_p()
        check(load().fhe_radix_random(_ctx().handle, _rerand_seed(seed), bits, bits if random_bits is None else int(random_bits),
                                      C.byref(h)))
        return cls._wrap(h, bits)

    @classmethod
    def random_below(cls, bound: int, seed=None, extra_bits: int = 64, bits=None):
        """tfhe-rs' generate_oblivious_pseudo_random_bounded (fhe_radix_random_below): an encrypted value in
        [0, bound), at most 2^-extra_bits from uniform: (m random bits * bound) >> m, m = bit_length(bound - 1) +
        extra_bits.  Seed rules as random's."""
        bits = bits or cls.BITS
        bound = int(bound)
        if bound < 0:
            raise ValueError("the bound is a positive integer")
        w = _words(bound, max(64, (bound.bit_length() + 63) // 64 * 64))
        h = C.c_void_p()
        check(load().fhe_radix_random_below(_ctx().handle, _rerand_seed(seed), bits, ptr(w), w.size, int(extra_bits),
                                            C.byref(h)))
        return cls._wrap(h, bits)

    def decrypt(self, client_key) -> int:
        n = (self.bits + 63) // 64
        w = np.zeros(n, np.uint64)
        check(load().fhe_radix_decrypt(_ctx().handle, client_key.handle, self._h, ptr(w), n))
        return sum(int(w[i]) << (64 * i) for i in range(n))

    def clone(self):
        h = C.c_void_p()
        check(load().fhe_radix_clone(self._h, C.byref(h)))
        return self._wrap(h, self.bits)

    @classmethod
    def broadcast(cls, x, root: int = 0, ctx=None):
        """Collective (fhe_ctx_broadcast_radix): rank `root` passes its FheUint, every other rank
        passes None and receives a copy with byte-identical block ciphertexts (RCCL over xGMI)."""
        ctx = ctx or _ctx()
        h = C.c_void_p(_hval(x.handle) if x is not None else None)
        check(load().fhe_ctx_broadcast_radix(ctx.handle, C.byref(h), root))
        if x is not None and h.value == _hval(x.handle):
            return x
        bits = C.c_uint32()
        check(load().fhe_radix_num_bits(h, C.byref(bits)))
        return cls._wrap(h, int(bits.value))

    def export(self) -> np.ndarray:
        nb = self.bits // 2
        out = np.zeros(nb * 2049, np.uint64)
        check(load().fhe_radix_export(_ctx().handle, self._h, ptr(out), out.size))
        return out.reshape(nb, 2049)

    def re_randomize(self, seed=None):
        """tfhe-rs' re_randomize under the CompactPublicKey (Context.set_public_key): a new FheUint, every
        block this one's plus a fresh public-key encryption of zero (fhe_radix_rerandomize); self is untouched.
        seed: 32 bytes used for this call only (rerandomization_seed), or None for OS entropy -- refused under a
        communicator of more than one rank, where every rank passes the same seed."""
        h = C.c_void_p()
        check(load().fhe_radix_rerandomize(_ctx().handle, self._h, _rerand_seed(seed), C.byref(h)))
        return self._wrap(h, self.bits)

    def digest(self) -> bytes:
        """the 32-byte value digest D(self) (fhe_radix_digest): the blocks are hashed on the GPU, 32 bytes each
        come back; self is untouched"""
        out = (C.c_uint8 * 32)()
        check(load().fhe_radix_digest(_ctx().handle, self._h, out))
        return bytes(out)

    # ---- helpers
    def _bin(self, fn, other):
        h = C.c_void_p()
        check(getattr(load(), fn)(_ctx().handle, self._h, other._h, C.byref(h)))
        return self._wrap(h, self.bits)

    def _scalar(self, fn, s):
        h = C.c_void_p()
        check(getattr(load(), fn)(_ctx().handle, self._h, s, C.byref(h)))
        return self._wrap(h, self.bits)

    def _scalar_any(self, fn, s: int, wrap: bool = True):
        """u64 entry point when the clear operand fits, the _words one otherwise (wide FheUint)."""
        s = int(s)
        if wrap:
            s %= 1 << self.bits
        if s < 0:
            raise ValueError("clear operand must be non-negative")
        if s < 2**64:
            return self._scalar(fn, s)
        w = _words(s, max(64, s.bit_length()))
        h = C.c_void_p()
        check(getattr(load(), fn + "_words")(_ctx().handle, self._h, ptr(w), w.size, C.byref(h)))
        return self._wrap(h, self.bits)

    # ---- operators (tfhe HL API)
    def __add__(self, o):
        return self._bin("fhe_radix_add", o) if isinstance(o, FheUint) else self._scalar_any("fhe_radix_scalar_add", o)

    def __sub__(self, o):
        return self._bin("fhe_radix_sub", o)

    def __mul__(self, o):
        return self._bin("fhe_radix_mul", o) if isinstance(o, FheUint) else self._scalar_any("fhe_radix_scalar_mul", o)

    def scalar_mul_add(self, m: int, k: int):
        """self * m + k for clear m, k (wrapping), one carry propagation"""
        wm, wk = _words(m, self.bits), _words(k, self.bits)
        h = C.c_void_p()
        P = C.POINTER(C.c_uint64)
        check(load().fhe_radix_scalar_mul_add_words(_ctx().handle, self._h, wm.ctypes.data_as(P), len(wm),
                                                     wk.ctypes.data_as(P), len(wk), C.byref(h)))
        return self._wrap(h, self.bits)

    def __and__(self, o):
        return self._bin("fhe_radix_bitand", o) if isinstance(o, FheUint) else self._scalar_any("fhe_radix_scalar_and", o)

    def __rshift__(self, o):
        if isinstance(o, FheUint):
            return self._bin("fhe_radix_shr", o)
        return self._scalar("fhe_radix_scalar_shr", int(o) % 2**32)

    def __lshift__(self, o):
        if isinstance(o, FheUint):
            return self._bin("fhe_radix_shl", o)
        return self._scalar("fhe_radix_scalar_shl", int(o) % 2**32)

    def __floordiv__(self, d):
        if isinstance(d, FheUint):
            return self._bin("fhe_radix_div", d)
        return self._scalar_any("fhe_radix_scalar_div", d, wrap=False)

    __truediv__ = __floordiv__  # tfhe's `&a / 5` on FheUint is integer division (src/perf_test.rs:54)

    def __mod__(self, d):
        if isinstance(d, FheUint):
            return self._bin("fhe_radix_rem", d)
        return self._scalar_any("fhe_radix_scalar_rem", d, wrap=False)

    def rem_pseudo_mersenne(self, k_bits: int, c: int):
        """self mod (2^k_bits - c) for a public pseudo-Mersenne modulus, as an FheUint of k_bits
        (fhe_radix_rem_pseudo_mersenne): a few folds x <- (x mod 2^k) + (x >> k) c and one conditional subtraction
        instead of `%`'s general division.  k_bits even, 0 < c < 2^(k_bits - 2); self of any width.  secp256k1:
        (256, SECP256K1_N_C) and (256, SECP256K1_P_C)."""
        k_bits, c = int(k_bits), int(c)
        if c < 0:
            raise ValueError("c must be positive")
        w = _words(c, max(64, (c.bit_length() + 63) // 64 * 64))
        h = C.c_void_p()
        check(load().fhe_radix_rem_pseudo_mersenne(_ctx().handle, self._h, k_bits, ptr(w), w.size, C.byref(h)))
        return self._wrap(h, k_bits)

    def serialize(self) -> bytes:
        """ciphertext bytes (own format, include/fhe_rocm.h); restore with FheUint.deserialize"""
        return serialize_with(load().fhe_radix_serialize, _ctx().handle, self._h)

    @classmethod
    def deserialize(cls, data: bytes):
        h = C.c_void_p()
        check(load().fhe_radix_deserialize(_ctx().handle, data, len(data), C.byref(h)))
        bits = C.c_uint32(0)
        check(load().fhe_radix_num_bits(h, C.byref(bits)))
        return FheUint._wrap(h, bits.value)

    def div_rem(self, d):
        """(self // d, self % d) for an encrypted divisor, one pass"""
        q, r = C.c_void_p(), C.c_void_p()
        check(load().fhe_radix_divrem(_ctx().handle, self._h, d._h, C.byref(q), C.byref(r)))
        return self._wrap(q, self.bits), self._wrap(r, self.bits)

    def min(self, o):
        return self._bin("fhe_radix_min", o)

    def max(self, o):
        return self._bin("fhe_radix_max", o)

    def lt(self, o):
        h = C.c_void_p()
        check(load().fhe_radix_lt(_ctx().handle, self._h, o._h, C.byref(h)))
        return self._wrap(h, 2)

    def cast_into(self, cls):
        bits = cls.BITS
        h = C.c_void_p()
        check(load().fhe_radix_cast(_ctx().handle, self._h, bits, C.byref(h)))
        return cls._wrap(h, bits)

    @classmethod
    def cast_from(cls, other):
        return other.cast_into(cls)


class FheBool(FheUint):
    BITS = 2


class FheUint8(FheUint):
    BITS = 8


class FheUint32(FheUint):
    BITS = 32


class FheUint64(FheUint):
    BITS = 64


class FheUint128(FheUint):
    BITS = 128


class FheUint256(FheUint):
    BITS = 256


def to_u32_digits(value: int) -> list[int]:
    """num_bigint::BigUint::to_u32_digits: LSB first, no leading zeros, [] for 0."""
    out = []
    while value:
        out.append(value & 0xFFFFFFFF)
        value >>= 32
    return out


class BigUintFHE:
    """src/biguint.rs:8-13 -- Vec<FheUint32> digits, least significant first."""

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_biguint_destroy(self._h)
            self._h = None

    @classmethod
    def new(cls, value: int, client_key):  # src/biguint.rs:17-31
        limbs = np.array(to_u32_digits(value), dtype=np.uint32)
        h = C.c_void_p()
        check(load().fhe_biguint_encrypt(_ctx().handle, client_key.handle, ptr(limbs, C.c_uint32), limbs.size, C.byref(h)))
        return cls(h)

    @classmethod
    def random(cls, bits: int, seed=None):
        """FheUint.random over bits / 32 digits (fhe_biguint_random; bits a multiple of 32): block i of the whole
        on row i of the seed"""
        h = C.c_void_p()
        check(load().fhe_biguint_random(_ctx().handle, _rerand_seed(seed), int(bits), C.byref(h)))
        return cls(h)

    def serialize(self) -> bytes:
        return serialize_with(load().fhe_biguint_serialize, _ctx().handle, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "BigUintFHE":
        h = C.c_void_p()
        check(load().fhe_biguint_deserialize(_ctx().handle, data, len(data), C.byref(h)))
        return cls(h)

    @classmethod
    def from_u32(cls, value: int, client_key):  # src/biguint.rs:34-36
        return cls.new(value, client_key)

    @classmethod
    def zero(cls, client_key):  # src/biguint.rs:51-53
        return cls.new(0, client_key)

    @classmethod
    def one(cls, client_key):  # src/biguint.rs:56-58
        return cls.new(1, client_key)

    @classmethod
    def from_encrypted_digits(cls, digits):  # src/biguint.rs:46-48
        arr = (C.c_void_p * len(digits))(*[d.handle for d in digits])
        h = C.c_void_p()
        check(load().fhe_biguint_from_digits(arr, len(digits), C.byref(h)))
        return cls(h)

    def __len__(self):
        n = C.c_size_t()
        check(load().fhe_biguint_len(self._h, C.byref(n)))
        return int(n.value)

    @property
    def digits(self):
        out = []
        for i in range(len(self)):
            h = C.c_void_p()
            check(load().fhe_biguint_digit(self._h, i, C.byref(h)))
            out.append(FheUint._wrap(h, 32))
        return out

    @classmethod
    def broadcast(cls, x, root: int = 0, ctx=None):
        """Collective (fhe_ctx_broadcast_biguint): the root's BigUintFHE (e.g. sign_fhe_with_k0's
        encrypted private key, src/schnorr.rs:235) replicated to every rank; other ranks pass None."""
        ctx = ctx or _ctx()
        h = C.c_void_p(_hval(x.handle) if x is not None else None)
        check(load().fhe_ctx_broadcast_biguint(ctx.handle, C.byref(h), root))
        if x is not None and h.value == _hval(x.handle):
            return x
        return cls(h)

    def decrypt_limbs(self, client_key) -> list[int]:
        n = len(self)
        buf = np.zeros(max(n, 1), np.uint32)
        got = C.c_size_t()
        check(load().fhe_biguint_decrypt(_ctx().handle, client_key.handle, self._h, ptr(buf, C.c_uint32), buf.size, C.byref(got)))
        return [int(x) for x in buf[: got.value]]

    def to_biguint(self, client_key) -> int:  # src/biguint.rs:61-76
        return sum(d << (32 * i) for i, d in enumerate(self.decrypt_limbs(client_key)))

    def decrypt_to_u32(self, client_key):  # src/biguint.rs:79-88
        limbs = self.decrypt_limbs(client_key)
        return {0: 0, 1: limbs[0] if limbs else 0}.get(len(limbs))

    def decrypt_to_u64(self, client_key):  # src/biguint.rs:91-105
        limbs = self.decrypt_limbs(client_key)
        if len(limbs) > 2:
            return None
        return sum(d << (32 * i) for i, d in enumerate(limbs))

    def to_radix(self, bits: int):
        """the limbs' blocks as one FheUint of `bits` (concatenation, no bootstrap)"""
        h = C.c_void_p()
        check(load().fhe_biguint_to_radix(self._h, bits, C.byref(h)))
        return FheUint._wrap(h, bits)

    def rem_pseudo_mersenne(self, k_bits: int, c: int):
        """the limbs' value mod (2^k_bits - c) as an FheUint of k_bits (FheUint.rem_pseudo_mersenne on to_radix)"""
        return self.to_radix(32 * max(1, len(self))).rem_pseudo_mersenne(k_bits, c)

    def clone(self):
        h = C.c_void_p()
        check(load().fhe_biguint_clone(self._h, C.byref(h)))
        return BigUintFHE(h)

    def add(self, other, mode: int = COMPAT):
        h = C.c_void_p()
        check(load().fhe_biguint_add(_ctx().handle, self._h, other._h, mode, C.byref(h)))
        return BigUintFHE(h)

    def mul(self, other, mode: int = COMPAT):
        h = C.c_void_p()
        check(load().fhe_biguint_mul(_ctx().handle, self._h, other._h, mode, C.byref(h)))
        return BigUintFHE(h)

    def mul_add(self, other, addend, mode: int = COMPAT):
        """addend + self * other, limbs identical to addend.add(self.mul(other)) (one schedule)"""
        h = C.c_void_p()
        check(load().fhe_biguint_mul_add(_ctx().handle, self._h, other._h, addend._h, mode, C.byref(h)))
        return BigUintFHE(h)

    def mul_add_value(self, other, addend, client_key, mode: int = COMPAT) -> int:
        """the value of mul_add's limbs, computed in column form (fhe_biguint_mul_add_columns: no final
        carry propagation) and decrypted with its carries resolved on the host -- what the signer does"""
        lib = load()
        h = C.c_void_p()
        check(lib.fhe_biguint_mul_add_columns(_ctx().handle, self._h, other._h, addend._h, mode, C.byref(h)))
        try:
            bits = C.c_uint32()
            check(lib.fhe_columns_bits(h, C.byref(bits)))
            n = (bits.value + 63) // 64
            w = np.zeros(n, np.uint64)
            check(lib.fhe_columns_decrypt(_ctx().handle, client_key.handle, h, ptr(w), n))
        finally:
            lib.fhe_columns_destroy(h)
        return sum(int(x) << (64 * i) for i, x in enumerate(w))

    def re_randomize(self, seed=None):
        """FheUint.re_randomize over the digits in order, 16 blocks each (fhe_biguint_rerandomize); the empty
        vector gives the empty vector"""
        h = C.c_void_p()
        check(load().fhe_biguint_rerandomize(_ctx().handle, self._h, _rerand_seed(seed), C.byref(h)))
        return BigUintFHE(h)

    def digest(self) -> bytes:
        """the 32-byte value digest of the digits in order, 16 blocks each (fhe_biguint_digest)"""
        out = (C.c_uint8 * 32)()
        check(load().fhe_biguint_digest(_ctx().handle, self._h, out))
        return bytes(out)

    __add__ = add
    __mul__ = mul


def _rerand_seed(seed):
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a re-randomization seed is 32 bytes")
    return seed


def rerandomize_host(public_key, seed, rows) -> np.ndarray:
    """the host definition of re_randomize (fhe_rerandomize_host): a re-randomized copy of `rows` (n x 2049
    words, e.g. FheUint.export()) under the CompactPublicKey and the 32-byte seed; no context, no GPU"""
    out = np.array(rows, dtype=np.uint64, order="C").reshape(-1, 2049)
    check(load().fhe_rerandomize_host(public_key.handle, _rerand_seed(seed), ptr(out), out.shape[0]))
    return out


def rerandomize_zero_host(public_key, seed, nblocks):
    """test hook (fhe_rerandomize_zero_host): (Z_A (nchunks, 2048), Z_B (nblocks,)) of the zero encryptions"""
    chunks = (nblocks + 2047) // 2048
    za, zb = np.zeros((chunks, 2048), np.uint64), np.zeros(nblocks, np.uint64)
    check(load().fhe_rerandomize_zero_host(public_key.handle, _rerand_seed(seed), nblocks, ptr(za), za.size, ptr(zb), zb.size))
    return za, zb


def rerandomize_rows(seed, rows, ctx=None) -> np.ndarray:
    """test hook (fhe_rerandomize_rows): the GPU path over n x 2049 host words, any n up to 2^24"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2049)
    out = np.zeros_like(rows)
    check(load().fhe_rerandomize_rows((ctx or _ctx()).handle, _rerand_seed(seed), ptr(rows), rows.shape[0], ptr(out)))
    return out


def rerandomization_seed(domain: bytes, data: bytes) -> bytes:
    """fhe_rerandomize_seed: the tagged SHA-256 replicas and ranks derive one call's seed from (a request id, a
    message hash).  A seed an adversary can predict before choosing the ciphertext protects nothing."""
    domain, data = bytes(domain), bytes(data)
    out = (C.c_uint8 * 32)()
    check(load().fhe_rerandomize_seed(domain, len(domain), data, len(data), out))
    return bytes(out)


def ct_digest_host(rows) -> np.ndarray:
    """the host definition of the row digest (fhe_ct_digest_host): (n, 32) bytes for n rows of 2049 words; no
    context, no GPU"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2049)
    out = np.zeros((rows.shape[0], 32), np.uint8)
    check(load().fhe_ct_digest_host(ptr(rows), rows.shape[0], ptr(out, C.c_uint8)))
    return out


def ct_digest_rows(rows, ctx=None) -> np.ndarray:
    """test hook (fhe_ct_digest_rows): the GPU path over n x 2049 host words, any n up to 2^24"""
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2049)
    out = np.zeros((rows.shape[0], 32), np.uint8)
    check(load().fhe_ct_digest_rows((ctx or _ctx()).handle, ptr(rows), rows.shape[0], ptr(out, C.c_uint8)))
    return out


def ct_value_digest_host(kind: int, bits: int, tags, degrees, noises, rowdigests) -> bytes:
    """fhe_ct_value_digest_host: D(x) from the per-block fields and row digests; kind 0 radix, 1 BigUintFHE"""
    tags = np.ascontiguousarray(tags, dtype=np.uint8)
    degrees, noises = np.ascontiguousarray(degrees, dtype=np.uint32), np.ascontiguousarray(noises, dtype=np.uint32)
    rowdigests = np.ascontiguousarray(rowdigests, dtype=np.uint8).reshape(-1, 32)
    n = tags.size
    if not (degrees.size == noises.size == rowdigests.shape[0] == n):
        raise ValueError("one tag, degree, noise and row digest per block")
    out = (C.c_uint8 * 32)()
    check(load().fhe_ct_value_digest_host(kind, bits, ptr(tags, C.c_uint8), ptr(degrees, C.c_uint32), ptr(noises, C.c_uint32),
                                          ptr(rowdigests, C.c_uint8), n, out))
    return bytes(out)


class ReRandomizationContext:
    """tfhe-rs' ReRandomizationContext (fhe_rerand_context_*): a running hash over a domain separator and, in call
    order, caller bytes and the digests of ciphertexts; seed(i) is the 32-byte seed of the i-th re_randomize call.
    The first seed() finalizes the context: a later add raises FheError (a seed depends on everything added)."""

    def __init__(self, domain: bytes):
        domain = bytes(domain)
        self._h = C.c_void_p()
        check(load().fhe_rerand_context_new(domain, len(domain), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_rerand_context_destroy(self._h)
            self._h = None

    def add_bytes(self, data: bytes):
        data = bytes(data)
        check(load().fhe_rerand_context_add_bytes(self._h, data, len(data)))
        return self

    def add_digest(self, digest: bytes):
        digest = bytes(digest)
        if len(digest) != 32:
            raise ValueError("a value digest is 32 bytes")
        check(load().fhe_rerand_context_add_digest(self._h, digest))
        return self

    def add(self, x):
        """the value digest of an FheUint or a BigUintFHE, computed on the GPU"""
        fn = load().fhe_rerand_context_add_biguint if isinstance(x, BigUintFHE) else load().fhe_rerand_context_add_radix
        check(fn(_ctx().handle, self._h, x.handle))
        return self

    def seed(self, index: int) -> bytes:
        out = (C.c_uint8 * 32)()
        check(load().fhe_rerand_context_seed(self._h, index, out))
        return bytes(out)


def re_randomize_bound(domain: bytes, values, data: bytes = b"") -> list:
    """re-randomizes every value under a seed bound to all of them: one ReRandomizationContext over `domain`, the
    bytes `data` (if any), then every value's digest in order; value i is re-randomized with seed(i).  No seed is
    passed in or out, so replicas and the ranks of a communicator compute the same ciphertexts."""
    values = list(values)
    rc = ReRandomizationContext(domain)
    if data:
        rc.add_bytes(data)
    for x in values:
        rc.add(x)
    return [x.re_randomize(rc.seed(i)) for i, x in enumerate(values)]


SEEDED_RADIX, SEEDED_BIGUINT = 0, 1  # FHE_SEEDED_*


def _mask_seed(seed):
    """the C ABI's mask_seed argument: None (32 bytes of OS entropy, drawn by the engine) or 32 bytes"""
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a mask seed is 32 bytes")
    return seed


class _Seeded:
    """fhe_seeded: a public mask seed and one body word per block, on the host (no context).  A seed is
    PUBLIC and must never serve two objects under one client key; leave `seed` None outside tests."""
    FORM = None

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_seeded_destroy(self._h)
            self._h = None

    def _info(self):
        form, count, nb = C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(load().fhe_seeded_info(self._h, C.byref(form), C.byref(count), C.byref(nb)))
        return int(form.value), int(count.value), int(nb.value)

    @property
    def nblocks(self) -> int:
        return self._info()[2]

    def serialize(self) -> bytes:
        """about 108 + 8 bytes per block (own format, include/fhe_rocm.h)"""
        return serialize_with(load().fhe_seeded_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes):
        h = C.c_void_p()
        check(load().fhe_seeded_deserialize(data, len(data), C.byref(h)))
        obj = _Seeded(h)
        form = obj._info()[0]
        if cls.FORM is not None and form != cls.FORM:
            raise FheError(f"{cls.__name__}.deserialize: the bytes hold the other seeded form", -1)
        obj.__class__ = CompressedBigUintFHE if form == SEEDED_BIGUINT else CompressedFheUint._kind(obj._info()[1])
        return obj

    def expand_host(self) -> np.ndarray:
        """the full ciphertexts, (nblocks, 2049): masks regenerated on the host, body appended -- the
        definition of what decompress() puts on the GPU"""
        nb = self.nblocks
        out = np.zeros((nb, 2049), np.uint64)
        check(load().fhe_seeded_expand_host(self._h, ptr(out), out.size))
        return out


class CompressedFheUint(_Seeded):
    """tfhe-rs' CompressedFheUint: try_encrypt on the client (no context), decompress on the server"""
    FORM = SEEDED_RADIX
    BITS = 0

    @staticmethod
    def _kind(bits):
        return {32: CompressedFheUint32, 64: CompressedFheUint64, 128: CompressedFheUint128,
                256: CompressedFheUint256, 8: CompressedFheUint8}.get(bits, CompressedFheUint)

    @property
    def bits(self) -> int:
        return self._info()[1]

    @classmethod
    def try_encrypt(cls, value: int, client_key, bits=None, seed=None):
        bits = bits or cls.BITS
        w = _words(value, bits)
        h = C.c_void_p()
        check(load().fhe_radix_encrypt_seeded(client_key.handle, ptr(w), bits, _mask_seed(seed), C.byref(h)))
        obj = cls._kind(bits).__new__(cls._kind(bits))
        _Seeded.__init__(obj, h)
        return obj

    encrypt = try_encrypt

    def decompress(self):
        """the matching FheUint on this thread's context (masks regenerated on the GPU)"""
        h = C.c_void_p()
        check(load().fhe_seeded_expand_radix(_ctx().handle, self._h, C.byref(h)))
        return FheUint._wrap(h, self.bits)


class CompressedFheUint8(CompressedFheUint):
    BITS = 8


class CompressedFheUint32(CompressedFheUint):
    BITS = 32


class CompressedFheUint64(CompressedFheUint):
    BITS = 64


class CompressedFheUint128(CompressedFheUint):
    BITS = 128


class CompressedFheUint256(CompressedFheUint):
    BITS = 256


class CompressedBigUintFHE(_Seeded):
    """BigUintFHE::new (src/biguint.rs:17-31) in the seeded form: 16 blocks per u32 limb"""
    FORM = SEEDED_BIGUINT

    @classmethod
    def new(cls, value: int, client_key, seed=None):
        limbs = np.array(to_u32_digits(value), dtype=np.uint32)
        h = C.c_void_p()
        check(load().fhe_biguint_encrypt_seeded(client_key.handle, ptr(limbs, C.c_uint32), limbs.size, _mask_seed(seed),
                                                C.byref(h)))
        return cls(h)

    def __len__(self):
        return self._info()[1]

    def decompress(self) -> BigUintFHE:
        h = C.c_void_p()
        check(load().fhe_seeded_expand_biguint(_ctx().handle, self._h, C.byref(h)))
        return BigUintFHE(h)


class CompressedCiphertextList:
    """tfhe-rs' CompressedCiphertextList holding one computed value: blocks packed into GLWEs under the
    compression key, 12 bits per coefficient (include/fhe_rocm.h).  A host object: serialize / deserialize /
    decrypt(private) need no context; decompress() brings it back onto this thread's GPU context."""

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_compressed_destroy(self._h)
            self._h = None

    def _info(self):
        form, count, nb = C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(load().fhe_compressed_info(self._h, C.byref(form), C.byref(count), C.byref(nb)))
        return int(form.value), int(count.value), int(nb.value)

    @property
    def nblocks(self) -> int:
        return self._info()[2]

    @property
    def params(self) -> CompressionParams:
        cp = CompressionParams()
        check(load().fhe_compressed_params(self._h, None, C.byref(cp)))
        return cp

    @property
    def bits(self) -> int:
        form, count, _ = self._info()
        return count if form == SEEDED_RADIX else 32 * count

    @classmethod
    def compress_host(cls, key, cts, degrees, form: int, count: int):
        """the packing keyswitch on the host (fhe_compress_host): the definition of the GPU path"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2049)
        deg = np.ascontiguousarray(np.broadcast_to(np.asarray(degrees, np.uint8), (cts.shape[0],)))
        h = C.c_void_p()
        check(load().fhe_compress_host(key.handle, ptr(cts), cts.shape[0], ptr(deg, C.c_uint8), form, count, C.byref(h)))
        return cls(h)

    def serialize(self) -> bytes:
        """108 + nblocks + sum_g ceil(12 (k' N' + b_g) / 8) bytes"""
        return serialize_with(load().fhe_compressed_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes):
        h = C.c_void_p()
        check(load().fhe_compressed_deserialize(data, len(data), C.byref(h)))
        return cls(h)

    def decrypt(self, private) -> int:
        """the value, from the 12-bit GLWEs directly (BigUintFHE form: limb i at bits 32 i)"""
        n = max(1, (self.bits + 63) // 64)
        w = np.zeros(n, np.uint64)
        check(load().fhe_compressed_decrypt(private.handle, self._h, ptr(w), n))
        return sum(int(w[i]) << (64 * i) for i in range(n))

    def decompress(self, ctx=None):
        """FheUint or BigUintFHE on ctx (default: this thread's context), fresh noise"""
        ctx = ctx or _ctx()
        form, count, _ = self._info()
        h = C.c_void_p()
        if form == SEEDED_BIGUINT:
            check(load().fhe_compressed_expand_biguint(ctx.handle, self._h, C.byref(h)))
            return BigUintFHE(h)
        check(load().fhe_compressed_expand_radix(ctx.handle, self._h, C.byref(h)))
        return FheUint._wrap(h, count)

    def extract_rows(self, ctx=None) -> np.ndarray:
        """test hook: the unpack + sample-extract kernel's rows, (nblocks, k' N' + 1)"""
        ctx = ctx or _ctx()
        n = self.nblocks
        out = np.zeros((n, self.params.lwe_dim() + 1), np.uint64)
        check(load().fhe_compressed_extract_rows(ctx.handle, self._h, ptr(out), out.size))
        return out


def _compress_radix(self) -> CompressedCiphertextList:
    """CompressedCiphertextListBuilder::push(self).build() on this thread's context"""
    h = C.c_void_p()
    check(load().fhe_radix_compress(_ctx().handle, self._h, C.byref(h)))
    return CompressedCiphertextList(h)


def _compress_biguint(self) -> CompressedCiphertextList:
    h = C.c_void_p()
    check(load().fhe_biguint_compress(_ctx().handle, self._h, C.byref(h)))
    return CompressedCiphertextList(h)


FheUint.compress = _compress_radix
BigUintFHE.compress = _compress_biguint


class SwitchedCiphertextList:
    """tfhe-rs' CompressedModulusSwitchedCiphertext holding one computed value: per block the keyswitched,
    modulus-switched row, n + 1 values of 12 bits (include/fhe_rocm.h "modulus-switched stored ciphertexts").  No
    key beyond the server key.  A host object: serialize / deserialize / decrypt(client_key) need no context;
    decompress() brings it back onto this thread's GPU context with one blind rotation per block."""

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_switched_list_destroy(self._h)
            self._h = None

    def _info(self):
        form, count, nb = C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(load().fhe_switched_list_info(self._h, C.byref(form), C.byref(count), C.byref(nb)))
        return int(form.value), int(count.value), int(nb.value)

    @property
    def nblocks(self) -> int:
        return self._info()[2]

    @property
    def params(self) -> FheParams:
        p = FheParams()
        check(load().fhe_switched_list_params(self._h, C.byref(p)))
        return p

    @property
    def bits(self) -> int:
        form, count, _ = self._info()
        return count if form == SEEDED_RADIX else 32 * count

    @classmethod
    def compress_host(cls, server_key, cts, degrees, form: int, count: int, ms_mode: str = "standard"):
        """the stored form on the host (fhe_switched_compress_host): the definition of the GPU path in the given
        modulus-switch mode ("standard" / "centered")"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, 2049)
        deg = np.ascontiguousarray(np.broadcast_to(np.asarray(degrees, np.uint8), (cts.shape[0],)))
        h = C.c_void_p()
        # a RekeyKey in the server key's place: its expanded KSK, the list under its destination
        fn = load().fhe_switched_compress_host_rekeyed if isinstance(server_key, RekeyKey) else load().fhe_switched_compress_host
        check(fn(server_key.handle, modulus_switch_mode(ms_mode), ptr(cts), cts.shape[0], ptr(deg, C.c_uint8), form, count,
                 C.byref(h)))
        return cls(h)

    def serialize(self) -> bytes:
        """80 + nblocks (1 + ceil(12 (n + 1) / 8)) bytes"""
        return serialize_with(load().fhe_switched_list_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes):
        h = C.c_void_p()
        check(load().fhe_switched_list_deserialize(data, len(data), C.byref(h)))
        return cls(h)

    def decrypt(self, client_key) -> int:
        """the value, from the 12-bit rows and the small key alone (BigUintFHE form: limb i at bits 32 i)"""
        n = max(1, (self.bits + 63) // 64)
        w = np.zeros(n, np.uint64)
        check(load().fhe_switched_decrypt(client_key.handle, self._h, ptr(w), n))
        return sum(int(w[i]) << (64 * i) for i in range(n))

    def decompress(self, ctx=None):
        """FheUint or BigUintFHE on ctx (default: this thread's context), fresh noise"""
        ctx = ctx or _ctx()
        form, count, _ = self._info()
        h = C.c_void_p()
        if form == SEEDED_BIGUINT:
            check(load().fhe_switched_expand_biguint(ctx.handle, self._h, C.byref(h)))
            return BigUintFHE(h)
        check(load().fhe_switched_expand_radix(ctx.handle, self._h, C.byref(h)))
        return FheUint._wrap(h, count)


def _compress_switched_radix(self, rekey: bool = False) -> SwitchedCiphertextList:
    """FheUint::compress() on this thread's context: the modulus-switched stored form; rekey=True: under the
    destination of the context's re-keying key (Context.set_rekey_key)"""
    h = C.c_void_p()
    fn = load().fhe_radix_compress_switched_rekeyed if rekey else load().fhe_radix_compress_switched
    check(fn(_ctx().handle, self._h, C.byref(h)))
    return SwitchedCiphertextList(h)


def _compress_switched_biguint(self, rekey: bool = False) -> SwitchedCiphertextList:
    h = C.c_void_p()
    fn = load().fhe_biguint_compress_switched_rekeyed if rekey else load().fhe_biguint_compress_switched
    check(fn(_ctx().handle, self._h, C.byref(h)))
    return SwitchedCiphertextList(h)


FheUint.compress_switched = _compress_switched_radix
BigUintFHE.compress_switched = _compress_switched_biguint


class CompactCiphertextListBuilder:
    """CompactCiphertextList::builder(&pk): push values, then build() or build_packed().  Needs the public
    key only -- no client key, no context."""

    def __init__(self, public_key):
        self._h = C.c_void_p()
        check(load().fhe_compact_builder_new(public_key.handle, C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_compact_builder_destroy(self._h)
            self._h = None

    def push(self, value: int, bits: int):
        """a radix integer of `bits` bits (FheUint)"""
        w = _words(value, bits) if bits > 0 else np.zeros(1, np.uint64)
        check(load().fhe_compact_builder_push_radix(self._h, ptr(w), bits))
        return self

    def push_biguint(self, value: int):
        """a BigUintFHE: 16 blocks per u32 limb, no leading zero limb (0 is the empty vector)"""
        limbs = np.array(to_u32_digits(value), dtype=np.uint32)
        check(load().fhe_compact_builder_push_biguint(self._h, ptr(limbs, C.c_uint32), limbs.size))
        return self

    def _build(self, packed, seed):
        h = C.c_void_p()
        check(load().fhe_compact_builder_build(self._h, packed, _mask_seed(seed), C.byref(h)))
        return CompactCiphertextList(h)

    def build(self, seed=None):
        """one block per coefficient.  `seed` is the SECRET encryption seed: tests only; None draws it from
        the OS, and it is kept nowhere"""
        return self._build(0, seed)

    def build_packed(self, seed=None):
        """two blocks per coefficient; expand() splits them with one bootstrap level.  `seed` as in build()"""
        return self._build(1, seed)


class CompactCiphertextList:
    """tfhe-rs' CompactCiphertextList: values encrypted under a CompactPublicKey, one GLWE (C_A, C_B) per
    2048 coefficients (include/fhe_rocm.h "public-key encryption").  A host object: serialize / deserialize /
    expand_host / decrypt(client_key) need no context; expand() brings the values onto this thread's GPU."""

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_compact_list_destroy(self._h)
            self._h = None

    @staticmethod
    def builder(public_key) -> CompactCiphertextListBuilder:
        return CompactCiphertextListBuilder(public_key)

    def _info(self):
        packed, nv, nc, nch = C.c_int(), C.c_uint32(), C.c_size_t(), C.c_size_t()
        check(load().fhe_compact_list_info(self._h, C.byref(packed), C.byref(nv), C.byref(nc), C.byref(nch)))
        return bool(packed.value), int(nv.value), int(nc.value), int(nch.value)

    @property
    def packed(self) -> bool:
        return self._info()[0]

    def __len__(self):
        return self._info()[1]

    @property
    def ncoef(self) -> int:
        return self._info()[2]

    @property
    def nchunks(self) -> int:
        return self._info()[3]

    def value_info(self, i: int):
        """(form, count, nblocks, first coefficient, coefficients) of value i"""
        form, count, nb, first, nc = C.c_uint32(), C.c_uint32(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        check(load().fhe_compact_list_value_info(self._h, i, C.byref(form), C.byref(count), C.byref(nb), C.byref(first),
                                                 C.byref(nc)))
        return int(form.value), int(count.value), int(nb.value), int(first.value), int(nc.value)

    def export(self):
        """(C_A as (nchunks, 2048), C_B as (ncoef,))"""
        _, _, nc, nch = self._info()
        ca, cb = np.zeros((nch, 2048), np.uint64), np.zeros(nc, np.uint64)
        check(load().fhe_compact_list_export(self._h, ptr(ca), ca.size, ptr(cb), cb.size))
        return ca, cb

    def serialize(self) -> bytes:
        """76 + 8 nvalues + 8 (2048 nchunks + ncoef) bytes"""
        return serialize_with(load().fhe_compact_list_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes):
        h = C.c_void_p()
        check(load().fhe_compact_list_deserialize(data, len(data), C.byref(h)))
        return cls(h)

    def expand_host(self) -> np.ndarray:
        """the sample-extracted big LWEs, (ncoef, 2049): the definition of what expand() puts on the GPU"""
        out = np.zeros((self.ncoef, 2049), np.uint64)
        check(load().fhe_compact_list_expand_host(self._h, ptr(out), out.size))
        return out

    def decrypt_value(self, client_key, i: int) -> int:
        form, count, _, _, _ = self.value_info(i)
        bits = count if form == SEEDED_RADIX else 32 * count
        n = max(1, (bits + 63) // 64)
        w = np.zeros(n, np.uint64)
        check(load().fhe_compact_list_decrypt(client_key.handle, self._h, i, ptr(w), n))
        return sum(int(w[k]) << (64 * k) for k in range(n))

    def decrypt(self, client_key) -> list:
        """every value, on the client (no GPU): phase, round, unpack"""
        return [self.decrypt_value(client_key, i) for i in range(len(self))]

    def expand_value(self, i: int, ctx=None):
        """value i as FheUint or BigUintFHE on ctx (default: this thread's context)"""
        ctx = ctx or _ctx()
        form, count = self.value_info(i)[:2]
        h = C.c_void_p()
        if form == SEEDED_BIGUINT:
            check(load().fhe_compact_list_expand_biguint(ctx.handle, self._h, i, C.byref(h)))
            return BigUintFHE(h)
        check(load().fhe_compact_list_expand_radix(ctx.handle, self._h, i, C.byref(h)))
        return FheUint._wrap(h, count)

    def expand(self, ctx=None) -> list:
        """CompactCiphertextList::expand: the values in push order.  A packed list records its unpacking
        bootstraps (one level) in the context's deferred graph"""
        return [self.expand_value(i, ctx) for i in range(len(self))]

    def extract_rows(self, ctx=None) -> np.ndarray:
        """test hook: the extraction kernel's rows, (ncoef, 2049)"""
        ctx = ctx or _ctx()
        out = np.zeros((self.ncoef, 2049), np.uint64)
        check(load().fhe_compact_list_extract_rows(ctx.handle, self._h, ptr(out), out.size))
        return out


LEVEL_SPLIT = 1 << 31  # FHE_LEVEL_SPLIT: the level was fanned out over the ranks


def rank_pbs(ctx) -> int:
    """bootstraps this rank ran itself (fhe_ctx_rank_pbs; emulated ranks: rank 0's share)"""
    v = C.c_uint64()
    check(load().fhe_ctx_rank_pbs(ctx.handle, C.byref(v)))
    return int(v.value)


def level_log(ctx, reset: bool = True) -> list[int]:
    """bootstraps per launched level since the last reset (fhe_ctx_level_log); under fan-out an
    entry carries LEVEL_SPLIT when the level was split over the ranks"""
    n = C.c_size_t()
    check(load().fhe_ctx_level_log(ctx.handle, None, 0, C.byref(n), 0))
    buf = np.zeros(max(1, n.value), np.uint32)
    check(load().fhe_ctx_level_log(ctx.handle, ptr(buf, C.c_uint32), buf.size, C.byref(n), 1 if reset else 0))
    return [int(x) for x in buf[: n.value]]


def stats(ctx):
    p, lv = C.c_uint64(), C.c_uint64()
    check(load().fhe_ctx_stats(ctx.handle, C.byref(p), C.byref(lv)))
    return int(p.value), int(lv.value)


# ---- test hooks: the launch trace (fhe_ctx_trace) and the read-only hooks its replay needs
def trace_enable(ctx, on: bool = True) -> None:
    check(load().fhe_ctx_trace(ctx.handle, 1 if on else 0))


def pending_info(ctx) -> tuple[int, int, int]:
    """(pending bootstraps, a deferred upload armed, helper jobs in flight) of a context (fhe_ctx_pending_info)"""
    out = (C.c_uint64 * 3)()
    check(load().fhe_ctx_pending_info(ctx.handle, out))
    return int(out[0]), int(out[1]), int(out[2])


def trace_read(ctx, reset: bool = True) -> np.ndarray:
    """the launch trace's u64 words since the last reset (fhe_ctx_trace_read; an overflowed trace raises)"""
    n = C.c_size_t()
    try:
        check(load().fhe_ctx_trace_read(ctx.handle, None, 0, C.byref(n), 0))
    except FheError:
        if reset:  # the refusal of an overflowed trace still clears it
            load().fhe_ctx_trace_read(ctx.handle, None, 0, C.byref(n), 1)
        raise
    buf = np.zeros(max(1, n.value), np.uint64)
    check(load().fhe_ctx_trace_read(ctx.handle, ptr(buf), buf.size, C.byref(n), 1 if reset else 0))
    return buf[: n.value].copy()


def block_addrs(ctx, x) -> tuple[list[int], list[int]]:
    """(addresses, trivial values) of the blocks of an FheUint or a BigUintFHE: address 0 marks a trivial block"""
    fn = load().fhe_biguint_block_addrs if isinstance(x, BigUintFHE) else load().fhe_radix_block_addrs
    n = C.c_size_t()
    check(fn(ctx.handle, x.handle, None, None, 0, C.byref(n)))
    a, v = np.zeros(max(1, n.value), np.uint64), np.zeros(max(1, n.value), np.uint32)
    check(fn(ctx.handle, x.handle, ptr(a), ptr(v, C.c_uint32), n.value, C.byref(n)))
    return [int(t) for t in a[: n.value]], [int(t) for t in v[: n.value]]


LUT_INTEGER, LUT_HALF_STEP, LUT_OPRF = 0, 1, 2


def lut_table(ctx, lut_id: int) -> tuple[int, list[int]]:
    """(kind, the 16 entries) of a registered table (fhe_ctx_lut_table)"""
    kind, e = C.c_int(), (C.c_int32 * 16)()
    check(load().fhe_ctx_lut_table(ctx.handle, lut_id, C.byref(kind), e))
    return int(kind.value), [int(t) for t in e]


def export_luts(ctx, first: int, count: int) -> np.ndarray:
    """tables [first, first + count) of the device table as it stands, (count, 2048) u64"""
    out = np.zeros((count, 2048), np.uint64)
    check(load().fhe_ctx_export_luts(ctx.handle, first, count, ptr(out)))
    return out
