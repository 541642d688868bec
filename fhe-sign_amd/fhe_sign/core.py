"""Keys, device context and the raw PBS boundary (thin wrappers over the C ABI)."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

from ._lib import CompressionParams, FheError, FheParams, check, load, ptr, serialize_with

BIG_CT = 2049  # big LWE ciphertext words


def default_params() -> FheParams:
    p = FheParams()
    check(load().fhe_params_default(C.byref(p)))
    return p


def multi_bit_params() -> FheParams:
    """default parameters with the multi-bit blind rotation (grouping 2; fhe_params.grouping)"""
    p = FheParams()
    check(load().fhe_params_multi_bit(C.byref(p)))
    return p


class ClientKey:
    def __init__(self, handle, params: FheParams):
        self._h = handle
        self.params = params

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_client_key_destroy(self._h)
            self._h = None

    def export(self):
        n = self.params.lwe_dimension
        lwe = np.zeros(n, np.uint64)
        glwe = np.zeros(self.params.polynomial_size, np.uint64)
        check(load().fhe_client_key_export(self._h, ptr(lwe), n, ptr(glwe), glwe.size))
        return lwe, glwe

    def serialize(self) -> bytes:
        """own versioned format (include/fhe_rocm.h, serial.h), encryption-stream state included"""
        return serialize_with(load().fhe_client_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "ClientKey":
        h = C.c_void_p()
        check(load().fhe_client_key_deserialize(data, len(data), C.byref(h)))
        p = FheParams()
        check(load().fhe_client_key_params(h, C.byref(p)))
        return cls(h, p)

    def seed_encryption(self, seed: int, stream: int = 100) -> None:
        check(load().fhe_client_key_seed_encryption(self._h, seed, stream))

    def encrypt_block(self, value: int) -> np.ndarray:
        ct = np.zeros(BIG_CT, np.uint64)
        check(load().fhe_encrypt_block(self._h, value, ptr(ct)))
        return ct

    def encrypt_blocks(self, values) -> np.ndarray:
        """many blocks at once: identical to encrypt_block in a loop (multi-threaded on the host)"""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
        out = np.zeros((v.size, BIG_CT), np.uint64)
        check(load().fhe_encrypt_blocks(self._h, ptr(v), v.size, ptr(out)))
        return out

    def decrypt_block(self, ct: np.ndarray) -> int:
        ct = np.ascontiguousarray(ct, dtype=np.uint64)
        out = C.c_uint64(0)
        check(load().fhe_decrypt_block(self._h, ptr(ct), C.byref(out)))
        return int(out.value)

    def encrypt_rows_indexed_host(self, values) -> np.ndarray:
        """host definition (fhe_client_encrypt_rows_indexed_host): encrypt_blocks restated from counter-indexed
        ChaCha blocks through the device kernel's index arithmetic; same words, same stream state afterwards"""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
        out = np.zeros((v.size, BIG_CT), np.uint64)
        check(load().fhe_client_encrypt_rows_indexed_host(self._h, ptr(v), v.size, ptr(out)))
        return out

    def decrypt_phase_host(self, cts) -> np.ndarray:
        """host definition (fhe_decrypt_phase_host): body - <mask, key> of every row, the word decrypt_block decodes"""
        cts = np.ascontiguousarray(np.asarray(cts, dtype=np.uint64).reshape(-1, BIG_CT))
        out = np.zeros(cts.shape[0], np.uint64)
        check(load().fhe_decrypt_phase_host(self._h, ptr(cts), cts.shape[0], ptr(out)))
        return out


class ServerKey:
    def __init__(self, handle, params: FheParams):
        self._h = handle
        self.params = params

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_server_key_destroy(self._h)
            self._h = None

    def serialize(self) -> bytes:
        return serialize_with(load().fhe_server_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "ServerKey":
        h = C.c_void_p()
        check(load().fhe_server_key_deserialize(data, len(data), C.byref(h)))
        p = FheParams()
        check(load().fhe_server_key_params(h, C.byref(p)))
        return cls(h, p)

    def export(self):
        p = self.params
        n, N, L = p.lwe_dimension, p.polynomial_size, p.ks_level
        ksk = np.zeros(N * L * (n + 1), np.uint64)
        bsk = np.zeros(p.ggsw_count() * 4 * N, np.uint64)
        check(load().fhe_server_key_export(self._h, ptr(ksk), ksk.size, ptr(bsk), bsk.size))
        return ksk, bsk


class CompressedServerKey:
    """tfhe-rs' CompressedServerKey: a public 32-byte seed and the bodies of the server key (4.5x smaller
    on the wire; include/fhe_rocm.h "seeded (compressed) server key").  Context.set_server_key(it)
    regenerates the masks on the GPU (decompress_to_gpu); decompress() does it on the host."""

    def __init__(self, handle, params: FheParams):
        self._h = handle
        self.params = params

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_seeded_server_key_destroy(self._h)
            self._h = None

    @classmethod
    def _wrap(cls, h) -> "CompressedServerKey":
        p = FheParams()
        check(load().fhe_seeded_server_key_params(h, C.byref(p)))
        return cls(h, p)

    @classmethod
    def new(cls, client_key: ClientKey, seed: bytes | None = None) -> "CompressedServerKey":
        """seed=None (the default) draws the public mask seed from the OS; a given 32-byte seed is for tests.
        One seed, one object: never reuse it under the same client key.  Advances the client key's
        encryption stream (the noise words)."""
        if seed is not None and len(seed) != 32:
            raise ValueError("the mask seed is 32 bytes")
        h = C.c_void_p()
        check(load().fhe_server_key_generate_seeded(client_key.handle, seed, C.byref(h)))
        return cls._wrap(h)

    def serialize(self) -> bytes:
        return serialize_with(load().fhe_seeded_server_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompressedServerKey":
        h = C.c_void_p()
        check(load().fhe_seeded_server_key_deserialize(data, len(data), C.byref(h)))
        return cls._wrap(h)

    def decompress(self) -> ServerKey:
        """the full key on the host: the word-for-word definition of the GPU install"""
        h = C.c_void_p()
        check(load().fhe_seeded_server_key_expand_host(self._h, C.byref(h)))
        return ServerKey(h, self.params)


class CompactPublicKey:
    """tfhe-rs' CompactPublicKey: a public 32-byte mask seed and the body polynomial B = A S + E under the
    client's big key (include/fhe_rocm.h "public-key encryption").  A host object, about 16.5 KB serialized;
    whoever holds it encrypts with CompactCiphertextList.builder(pk), no secret involved."""

    def __init__(self, handle):
        self._h = handle
        self.params = FheParams()
        check(load().fhe_public_key_params(handle, C.byref(self.params)))

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_public_key_destroy(self._h)
            self._h = None

    @classmethod
    def new(cls, client_key: "ClientKey", seed=None) -> "CompactPublicKey":
        """advances client_key's encryption stream by exactly 2048 words; `seed` (32 bytes, PUBLIC) is for
        tests, None draws it from the OS"""
        if seed is not None:
            seed = bytes(seed)
            if len(seed) != 32:
                raise ValueError("a mask seed is 32 bytes")
        h = C.c_void_p()
        check(load().fhe_public_key_generate(client_key.handle, seed, C.byref(h)))
        return cls(h)

    def export(self):
        """(the 32 seed bytes, the 2048 body words)"""
        seed = (C.c_uint8 * 32)()
        body = np.zeros(2048, np.uint64)
        check(load().fhe_public_key_export(self._h, seed, ptr(body), body.size))
        return bytes(seed), body

    def serialize(self) -> bytes:
        """16,484 bytes: frame, params, seed, 2048 body words"""
        return serialize_with(load().fhe_public_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompactPublicKey":
        h = C.c_void_p()
        check(load().fhe_public_key_deserialize(data, len(data), C.byref(h)))
        return cls(h)


class RekeyKey:
    """tfhe-rs' KeySwitchingKey from the big key of one client key to the small key of another (include/fhe_rocm.h
    "re-keying through the stored form"): seeded only, 82 KB at the defaults.  Context.set_rekey_key installs it;
    x.compress_switched(rekey=True) then gives a stored value under the destination key."""

    def __init__(self, handle):
        self._h = handle

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_rekey_key_destroy(self._h)
            self._h = None

    @classmethod
    def new(cls, src_client_key: "ClientKey", dst_client_key: "ClientKey", seed=None) -> "RekeyKey":
        """advances dst_client_key's encryption stream by exactly 2048 ks_level words; `seed` (32 bytes, PUBLIC) is
        for tests, None draws it from the OS.  One seed, one object."""
        if seed is not None:
            seed = bytes(seed)
            if len(seed) != 32:
                raise ValueError("a mask seed is 32 bytes")
        h = C.c_void_p()
        check(load().fhe_rekey_key_generate(src_client_key.handle, dst_client_key.handle, seed, C.byref(h)))
        return cls(h)

    @property
    def params(self) -> FheParams:
        """the destination's"""
        p = FheParams()
        check(load().fhe_rekey_key_params(self._h, C.byref(p)))
        return p

    def serialize(self) -> bytes:
        """100 + 8 (2048 ks_level) bytes: frame, the destination's params, seed, bodies"""
        return serialize_with(load().fhe_rekey_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "RekeyKey":
        h = C.c_void_p()
        check(load().fhe_rekey_key_deserialize(data, len(data), C.byref(h)))
        return cls(h)

    def expand_host(self) -> np.ndarray:
        """the full KSK [2048][ks_level][n_dst + 1] as flat uint64, in the server key's layout"""
        p = self.params
        ksk = np.zeros(p.polynomial_size * p.ks_level * (p.lwe_dimension + 1), np.uint64)
        check(load().fhe_rekey_key_expand_host(self._h, ptr(ksk), ksk.size))
        return ksk


def default_compression_params() -> CompressionParams:
    p = CompressionParams()
    check(load().fhe_compression_params_default(C.byref(p)))
    return p


class CompressionPrivateKey:
    """tfhe-rs' CompressionPrivateKeys: the client's secret s' of the packed GLWEs (k' N' bits)"""

    def __init__(self, handle):
        self._h = handle
        self.params = CompressionParams()
        check(load().fhe_compression_private_key_params(handle, None, C.byref(self.params)))

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_compression_private_key_destroy(self._h)
            self._h = None

    def export(self) -> np.ndarray:
        sk = np.zeros(self.params.lwe_dim(), np.uint64)
        check(load().fhe_compression_private_key_export(self._h, ptr(sk), sk.size))
        return sk

    def serialize(self) -> bytes:
        return serialize_with(load().fhe_compression_private_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompressionPrivateKey":
        h = C.c_void_p()
        check(load().fhe_compression_private_key_deserialize(data, len(data), C.byref(h)))
        return cls(h)


class CompressionKey:
    """tfhe-rs' CompressionKey + DecompressionKey: the packing keyswitch key and the classic bootstrapping
    key of dimension k' N' (include/fhe_rocm.h); Context.set_compression_key installs it"""

    def __init__(self, handle):
        self._h = handle
        self.main_params, self.params = FheParams(), CompressionParams()
        check(load().fhe_compression_key_params(handle, C.byref(self.main_params), C.byref(self.params)))

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_compression_key_destroy(self._h)
            self._h = None

    def export(self):
        """(packing KSK [2048][level][k' + 1][N'], decompression BSK [k' N'][2][2][2048]) as flat uint64"""
        c = self.params
        pksk = np.zeros(2048 * c.pks_level * (c.glwe_dimension + 1) * c.polynomial_size, np.uint64)
        bsk = np.zeros(c.lwe_dim() * 4 * 2048, np.uint64)
        check(load().fhe_compression_key_export(self._h, ptr(pksk), pksk.size, ptr(bsk), bsk.size))
        return pksk, bsk

    def serialize(self) -> bytes:
        return serialize_with(load().fhe_compression_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompressionKey":
        h = C.c_void_p()
        check(load().fhe_compression_key_deserialize(data, len(data), C.byref(h)))
        return cls(h)


class CompressedCompressionKey:
    """tfhe-rs' CompressedCompressionKey + CompressedDecompressionKey: a public 32-byte seed and the bodies of
    the compression key (3.0x smaller on the wire; include/fhe_rocm.h "seeded (compressed) compression key").
    Context.set_compression_key(it) regenerates the masks on the GPU; decompress() does it on the host."""

    def __init__(self, handle):
        self._h = handle
        self.main_params, self.params = FheParams(), CompressionParams()
        check(load().fhe_seeded_compression_key_params(handle, C.byref(self.main_params), C.byref(self.params)))

    @property
    def handle(self):
        return self._h

    def __del__(self):
        if getattr(self, "_h", None):
            load().fhe_seeded_compression_key_destroy(self._h)
            self._h = None

    def serialize(self) -> bytes:
        """128 + 8 (2048 level N' + 4096 k' N') bytes: frame, both parameter sets, seed, bodies"""
        return serialize_with(load().fhe_seeded_compression_key_serialize, self._h)

    @classmethod
    def deserialize(cls, data: bytes) -> "CompressedCompressionKey":
        h = C.c_void_p()
        check(load().fhe_seeded_compression_key_deserialize(data, len(data), C.byref(h)))
        return cls(h)

    def decompress(self) -> CompressionKey:
        """the full key on the host: the word-for-word definition of the GPU install"""
        h = C.c_void_p()
        check(load().fhe_seeded_compression_key_expand_host(self._h, C.byref(h)))
        return CompressionKey(h)


class CompressionKeys:
    @staticmethod
    def generate_compressed(client_key: ClientKey, params: CompressionParams | None = None, seed: bytes | None = None):
        """(CompressionPrivateKey, CompressedCompressionKey) of client_key; advances its encryption stream by
        k' N' + 2048 level N' + 4096 k' N' words.  seed=None (the default) draws the public mask seed from the
        OS; a given 32-byte seed is for tests.  One seed, one object: never reuse it under the same client key."""
        if seed is not None:
            seed = bytes(seed)
            if len(seed) != 32:
                raise ValueError("the mask seed is 32 bytes")
        a, b = C.c_void_p(), C.c_void_p()
        check(load().fhe_compression_keys_generate_seeded(
            client_key.handle, C.byref(params) if params is not None else None, seed, C.byref(a), C.byref(b)))
        return CompressionPrivateKey(a), CompressedCompressionKey(b)

    @staticmethod
    def generate(client_key: ClientKey, params: CompressionParams | None = None):
        """(CompressionPrivateKey, CompressionKey) of client_key; advances its encryption stream by
        k' N' + 2048 level (k' + 1) N' + 8192 k' N' words"""
        a, b = C.c_void_p(), C.c_void_p()
        check(load().fhe_compression_keys_generate(client_key.handle, C.byref(params) if params is not None else None,
                                                   C.byref(a), C.byref(b)))
        return CompressionPrivateKey(a), CompressionKey(b)


def comm_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it and shares it out of band, e.g. over torch.distributed)."""
    buf = (C.c_uint8 * 128)()
    check(load().fhe_comm_unique_id(buf))
    return bytes(buf)


def generate_keys(params: FheParams | None = None, seed: int | None = None, device: "Context | None" = None):
    """tfhe::generate_keys(ConfigBuilder::default().build()) -- src/schnorr.rs:441-442.

    seed=None (the default) keys every ChaCha20 stream with 32 bytes from os.urandom, as tfhe-rs
    draws from the OS CSPRNG.  An integer seed gives DETERMINISTIC, INSECURE keys (a public
    expansion of 64 bits) for tests and golden vectors only.
    With `device` (a Context), the server key is generated on that GPU: identical key words
    (fhe_generate_keys_device*); the key is returned, not installed."""
    import os

    p = params or default_params()
    ck, sk = C.c_void_p(), C.c_void_p()
    lib = load()
    if seed is None:
        key = (C.c_uint8 * 32).from_buffer_copy(os.urandom(32))
        if device is None:
            check(lib.fhe_generate_keys_keyed(C.byref(p), key, C.byref(ck), C.byref(sk)))
        else:
            check(lib.fhe_generate_keys_device_keyed(device.handle, C.byref(p), key, C.byref(ck), C.byref(sk)))
        C.memset(key, 0, 32)
    elif device is None:
        check(lib.fhe_generate_keys(C.byref(p), seed, C.byref(ck), C.byref(sk)))
    else:
        check(lib.fhe_generate_keys_device(device.handle, C.byref(p), seed, C.byref(ck), C.byref(sk)))
    return ClientKey(ck, p), ServerKey(sk, p)


# fhe_ctx_set_modulus_switch: FHE_MS_STANDARD, FHE_MS_CENTERED
MODULUS_SWITCH_NAMES = ("standard", "centered")
MS_PAD_WORD = 0xA5A55A5AC3C33C3C  # what ms_center_host / Context.ms_center_rows put into a row's padding


def modulus_switch_mode(name: str) -> int:
    """the FHE_MS_* value of a mode name; an unknown one is refused here as the library refuses an unknown value"""
    if name not in MODULUS_SWITCH_NAMES:
        raise FheError(f"fhe error -1: unknown modulus switch mode {name!r} (one of {MODULUS_SWITCH_NAMES})", -1)
    return MODULUS_SWITCH_NAMES.index(name)


def ms_stride(n: int) -> int:
    """words per row of the bootstrap workspace: n + 1 rounded up to 8 (64-byte rows)"""
    return (n + 1 + 7) // 8 * 8


def _ms_center_layout(rows, stride):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[1] < 2:
        raise ValueError("rows must be (count, n + 1) words")
    n = rows.shape[1] - 1
    stride = n + 1 if stride is None else int(stride)
    if stride < n + 1:
        raise ValueError("stride must be at least n + 1")
    buf = np.full((rows.shape[0], stride), MS_PAD_WORD, np.uint64)
    buf[:, :n + 1] = rows
    return buf, n


def ms_center_host(rows, stride=None) -> np.ndarray:
    """the host definition of the centered modulus switch (fhe_ms_center_host) over (count, n + 1) rows:
    body -= (sum of the mask words' signed rounding residues to the 2^52 grid) >> 1.  Laid out and returned as
    Context.ms_center_rows does: (count, stride) words, padding included.  No GPU."""
    buf, n = _ms_center_layout(rows, stride)
    check(load().fhe_ms_center_host(ptr(buf), buf.shape[0], n, buf.shape[1]))
    return buf


def _oprf_seed(seed) -> bytes:
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes")
    return seed


def oprf_rows_host(seed, n: int, count: int, stride=None) -> np.ndarray:
    """the host definition of the oblivious pseudo-random values' rows (fhe_oprf_rows_host): (count, stride) words,
    row b's n mask words from ChaCha blocks [b R, (b + 1) R), R = ceil(n / 8), of the PUBLIC 32-byte seed's stream,
    0 at word n, MS_PAD_WORD above (default stride n + 1; ms_stride(n) is the bootstrap workspace's).  No GPU."""
    stride = n + 1 if stride is None else int(stride)
    out = np.zeros((int(count), max(stride, 1)), np.uint64)
    check(load().fhe_oprf_rows_host(_oprf_seed(seed), int(n), int(count), stride, ptr(out)))
    return out


def oprf_lut_host(bits: int, params: FheParams | None = None) -> np.ndarray:
    """the accumulator polynomial of a `bits`-bit oblivious pseudo-random block (fhe_oprf_lut_host): 2048 words,
    coefficient i = (2 floor(i 2^bits / 4096) + 1) delta / 2.  No GPU."""
    p = params if params is not None else default_params()
    out = np.zeros(2048, np.uint64)
    check(load().fhe_oprf_lut_host(C.byref(p), int(bits), ptr(out)))
    return out


SWITCHED_GAP_BYTE = 0xE7  # what switched_pack_host / Context.switched_pack_rows leave between packed rows


def switched_row_bytes(n: int) -> int:
    """bytes of one modulus-switched stored row: n + 1 values of 12 bits from a byte boundary"""
    return (12 * (n + 1) + 7) // 8


def _switched_pack(call, rows, n, byte_stride):
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2:
        raise ValueError("rows must be (count, stride) words")
    byte_stride = switched_row_bytes(n) if byte_stride is None else int(byte_stride)
    out = np.full((rows.shape[0], max(byte_stride, 1)), SWITCHED_GAP_BYTE, np.uint8)
    check(call(ptr(rows), rows.shape[0], int(n), rows.shape[1], ptr(out, C.c_uint8), byte_stride))
    return out


def _switched_unpack(call, packed, n, stride):
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    if packed.ndim != 2:
        raise ValueError("packed must be (count, byte_stride) bytes")
    stride = n + 1 if stride is None else int(stride)
    out = np.zeros((packed.shape[0], max(stride, 1)), np.uint64)
    check(call(ptr(packed, C.c_uint8), packed.shape[0], int(n), packed.shape[1], ptr(out), stride))
    return out


def switched_pack_host(rows, n: int, byte_stride=None) -> np.ndarray:
    """the host definition of a stored row (fhe_switched_pack_host): (count, stride >= n + 1) words -> (count,
    byte_stride) bytes, each row the 12-bit roundings of its words 0 .. n, little-endian bit-contiguous, the pad nibble
    zero; the bytes above switched_row_bytes(n) keep SWITCHED_GAP_BYTE.  No GPU."""
    return _switched_pack(load().fhe_switched_pack_host, rows, n, byte_stride)


def switched_unpack_host(packed, n: int, stride=None) -> np.ndarray:
    """the inverse (fhe_switched_unpack_host): (count, byte_stride) bytes -> (count, stride) words, value << 52 at
    words 0 .. n, MS_PAD_WORD above.  No GPU."""
    return _switched_unpack(load().fhe_switched_unpack_host, packed, n, stride)


class Context:
    """One GPU + installed server key (tfhe::set_server_key, src/schnorr.rs:443)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(load().fhe_ctx_create(device, C.byref(h)))
        self._h = h
        self.params = None
        self._comp_params = None  # of the key set_compression_key installed last

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            load().fhe_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def set_server_key(self, sk: "ServerKey | CompressedServerKey") -> None:
        """a CompressedServerKey is installed from its bodies: the masks are regenerated on the GPU"""
        if isinstance(sk, CompressedServerKey):
            check(load().fhe_set_server_key_seeded(self._h, sk.handle))
        else:
            check(load().fhe_set_server_key(self._h, sk.handle))
        self.params = sk.params

    def set_compression_key(self, key: "CompressionKey | CompressedCompressionKey") -> None:
        """after set_server_key; the next set_server_key drops it.  A CompressedCompressionKey is installed
        from its bodies: the masks are regenerated on the GPU"""
        if isinstance(key, CompressedCompressionKey):
            check(load().fhe_set_compression_key_seeded(self._h, key.handle))
        else:
            check(load().fhe_set_compression_key(self._h, key.handle))
        self._comp_params = key.params

    def set_public_key(self, pk: "CompactPublicKey") -> None:
        """after set_server_key; the next set_server_key drops it.  Uploads A and B (32 KB) for re_randomize"""
        check(load().fhe_set_public_key(self._h, pk.handle))

    def export_compression_state(self):
        """(byte planes int8, Fourier BSK float64, its E layout float64) of the installed compression key
        (test hook: fhe_ctx_export_compression_state)"""
        lib = load()
        check(lib.fhe_ctx_export_compression_state(self._h, None, 0, None, 0, None, 0))  # FHE_ERR_NO_KEY first
        c = self._comp_params
        if c is None:
            raise RuntimeError("export_compression_state: the key was not installed through set_compression_key")
        cols = (c.glwe_dimension + 1) * c.polynomial_size
        planes = np.zeros(8 * ((cols + 15) // 16) * 32 * c.pks_level * 1024, np.int8)
        bsk = np.zeros(c.lwe_dim() * 4 * 1024 * 2, np.float64)
        bsk_e = np.zeros_like(bsk)
        check(lib.fhe_ctx_export_compression_state(self._h, planes.ctypes.data, planes.size, bsk.ctypes.data, bsk.size,
                                                   bsk_e.ctypes.data, bsk_e.size))
        return planes, bsk, bsk_e

    def pack_keyswitch_words(self, cts: np.ndarray):
        """test hook (fhe_pack_keyswitch_words): the packing keyswitch's contraction alone over (count, 2049) rows
        of any words, launched as compress launches it.  Returns (P, body): the (count, (k' + 1) N') words
        sum_{j, l} d[i, j, l] PKSK[j][l] mod 2^64 and the count body words set aside"""
        check(load().fhe_pack_keyswitch_words(self._h, None, 0, None, 0, None))  # FHE_ERR_NO_KEY first
        c = self._comp_params
        if c is None:
            raise RuntimeError("pack_keyswitch_words: the key was not installed through set_compression_key")
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, BIG_CT)
        P = np.zeros((cts.shape[0], (c.glwe_dimension + 1) * c.polynomial_size), np.uint64)
        body = np.zeros(cts.shape[0], np.uint64)
        check(load().fhe_pack_keyswitch_words(self._h, ptr(cts), cts.shape[0], ptr(P), P.size, ptr(body)))
        return P, body

    def export_fourier_bsk(self) -> np.ndarray:
        out = np.zeros(self.params.ggsw_count() * 4 * 1024 * 2, np.float64)
        check(load().fhe_ctx_export_fourier_bsk(self._h, ptr(out, C.c_double), out.size))
        return out

    def lut(self, table) -> int:
        t = np.ascontiguousarray(np.asarray(table, dtype=np.uint32))
        out = C.c_uint32(0)
        check(load().fhe_lut_register(self._h, ptr(t, C.c_uint32), t.size, C.byref(out)))
        return int(out.value)

    def pbs(self, cts: np.ndarray, lut_ids) -> np.ndarray:
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, BIG_CT)
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(lut_ids, np.uint32), (cts.shape[0],)))
        out = np.zeros_like(cts)
        check(load().fhe_pbs_batch(self._h, ptr(cts), cts.shape[0], ptr(ids, C.c_uint32), ptr(out)))
        return out

    def keyswitch(self, cts: np.ndarray) -> np.ndarray:
        """the keyswitch alone (fhe_keyswitch_batch): (count, 2049) big LWE -> (count, n + 1) small LWE
        words before the modulus switch, on the kernel set_ks_kernel selected"""
        cts = np.ascontiguousarray(cts, dtype=np.uint64).reshape(-1, BIG_CT)
        n = self.params.lwe_dimension if self.params is not None else 0
        out = np.zeros((cts.shape[0], n + 1), np.uint64)
        check(load().fhe_keyswitch_batch(self._h, ptr(cts), cts.shape[0], ptr(out)))
        return out

    def pbs_lincomb(self, blocks: np.ndarray, items, lut_ids, want_small: bool = True, want_out: bool = True):
        """bootstraps of linear combinations through the radix layer's descriptors
        (fhe_pbs_lincomb_batch): `items` is a list of ([(src, coef), ...], cst) over the rows of
        `blocks`, item i through LUT lut_ids[i].  Returns (small, out): the keyswitched (count, n + 1)
        words and the bootstrapped (count, 2049) blocks, None for the one not wanted."""
        blocks = np.ascontiguousarray(blocks, dtype=np.uint64).reshape(-1, BIG_CT)
        count = len(items)
        off = np.zeros(count + 1, np.uint32)
        src, coef = [], []
        for i, (terms, _) in enumerate(items):
            src += [s for s, _ in terms]
            coef += [c for _, c in terms]
            off[i + 1] = len(src)
        src = np.array(src + [0], np.uint32)  # never empty: a valid pointer for an item list without terms
        coef = np.array(coef + [0], np.int64)
        cst = np.array([c % (1 << 64) for _, c in items] + [0], np.uint64)
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(lut_ids, np.uint32), (count,)))
        n = self.params.lwe_dimension if self.params is not None else 0
        small = np.zeros((count, n + 1), np.uint64) if want_small else None
        out = np.zeros((count, BIG_CT), np.uint64) if want_out else None
        check(load().fhe_pbs_lincomb_batch(
            self._h, ptr(blocks), blocks.shape[0], ptr(off, C.c_uint32), ptr(src, C.c_uint32), ptr(coef, C.c_int64),
            ptr(cst), ptr(ids, C.c_uint32), count, ptr(small) if want_small else None,
            ptr(out) if want_out else None))
        return small, out

    # device-resident helpers (bench)
    def alloc(self, nbytes: int) -> int:
        p = load().fhe_device_alloc(self._h, nbytes)
        if not p:
            check(-4)
        return p

    def free(self, p: int) -> None:
        check(load().fhe_device_free(self._h, C.c_void_p(p)))

    def h2d(self, dst: int, arr: np.ndarray) -> None:
        check(load().fhe_memcpy_h2d(self._h, C.c_void_p(dst), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def d2h(self, arr: np.ndarray, src: int) -> None:
        check(load().fhe_memcpy_d2h(self._h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(src), arr.nbytes))

    def pbs_device(self, d_in: int, count: int, d_lut: int, d_out: int) -> None:
        check(load().fhe_pbs_batch_device(self._h, C.c_void_p(d_in), count, C.c_void_p(d_lut), C.c_void_p(d_out)))

    def sync(self) -> None:
        check(load().fhe_ctx_sync(self._h))

    def set_br_kernel(self, kind: int) -> None:
        """4 = br_qy.hip, the throughput kernel (classic and multi-bit); the retired kernels 0 (2-wave), 1 (quad),
        2 (pair) and 3 (qx) are refused (FHE_ERR_INVALID)."""
        check(load().fhe_ctx_set_br_kernel(self._h, int(kind)))

    def set_ks_kernel(self, kind: int) -> None:
        """0 = 64-bit VALU keyswitch, 1 = int8 matrix-core keyswitch (default); identical results"""
        check(load().fhe_ctx_set_ks_kernel(self._h, int(kind)))

    def time_ct_digest(self, nblocks: int, reps: int) -> float:
        """measurement hook (fhe_ctx_time_ct_digest): mean milliseconds of k_ct_digest over nblocks resident rows"""
        ms = C.c_float()
        check(load().fhe_ctx_time_ct_digest(self._h, nblocks, reps, C.byref(ms)))
        return ms.value

    def set_modulus_switch(self, mode: str) -> None:
        """"standard" (default) or "centered" (fhe_ctx_set_modulus_switch): in centered mode every keyswitch this
        context launches from now on is followed by k_ms_center, which takes the public half of the modulus
        switch's rounding error out of the body (sigma 5.9 -> 4.2 grid steps at n = 834).  Launches nothing itself;
        under a communicator every rank sets the same mode."""
        check(load().fhe_ctx_set_modulus_switch(self._h, modulus_switch_mode(mode)))

    @property
    def modulus_switch(self) -> str:
        m = C.c_int(-1)
        check(load().fhe_ctx_get_modulus_switch(self._h, C.byref(m)))
        return MODULUS_SWITCH_NAMES[m.value]

    def ms_center_rows(self, rows: np.ndarray, stride=None) -> np.ndarray:
        """test hook (fhe_ms_center_rows): k_ms_center over (count, n + 1) host rows, laid out with `stride` words
        per row (default n + 1; ms_stride(n) is the bootstrap workspace's), the padding filled with MS_PAD_WORD.
        Returns all (count, stride) words as they come back, padding included.  Needs no server key."""
        buf, n = _ms_center_layout(rows, stride)
        check(load().fhe_ms_center_rows(self._h, ptr(buf), buf.shape[0], n, buf.shape[1]))
        return buf

    def time_ms_center(self, count: int, n: int, stride: int, reps: int = 30) -> float:
        """measurement hook (fhe_ctx_time_ms_center): mean ms of one k_ms_center launch over count rows"""
        ms = C.c_float()
        check(load().fhe_ctx_time_ms_center(self._h, int(count), int(n), int(stride), int(reps), C.byref(ms)))
        return float(ms.value)

    def oprf_rows(self, seed, n: int, count: int, stride=None) -> np.ndarray:
        """test hook (fhe_oprf_rows): k_oprf_rows over a scratch buffer, returned as oprf_rows_host lays its rows
        out: (count, stride) words, padding included.  Needs no server key."""
        stride = n + 1 if stride is None else int(stride)
        out = np.zeros((int(count), max(stride, 1)), np.uint64)
        check(load().fhe_oprf_rows(self._h, _oprf_seed(seed), int(n), int(count), stride, ptr(out)))
        return out

    def oprf_blocks(self, seed, count: int, bits: int) -> np.ndarray:
        """test hook (fhe_oprf_blocks): the raw (count, 2049) words of blocks 0 .. count - 1 of the seed at `bits`"""
        out = np.zeros((int(count), BIG_CT), np.uint64)
        check(load().fhe_oprf_blocks(self._h, _oprf_seed(seed), int(count), int(bits), ptr(out)))
        return out

    def time_oprf_rows(self, count: int, n: int, reps: int = 30) -> float:
        """measurement hook (fhe_ctx_time_oprf_rows): mean ms of one k_oprf_rows launch over count workspace rows"""
        ms = C.c_float()
        check(load().fhe_ctx_time_oprf_rows(self._h, int(count), int(n), int(reps), C.byref(ms)))
        return float(ms.value)

    def set_rekey_key(self, key: "RekeyKey") -> None:
        """after set_server_key, dropped by the next one (fhe_set_rekey_key): x.compress_switched(rekey=True) then
        stores values under the key's destination"""
        check(load().fhe_set_rekey_key(self._h, key.handle))

    def switched_pack_rows(self, rows, n: int, byte_stride=None) -> np.ndarray:
        """test hook (fhe_switched_pack_rows): k_ms_pack over a scratch copy of the rows in the bootstrap workspace's
        layout, returned as switched_pack_host returns its bytes.  Needs no server key."""
        h = self._h
        return _switched_pack(lambda *a: load().fhe_switched_pack_rows(h, *a), rows, n, byte_stride)

    def switched_unpack_rows(self, packed, n: int, stride=None) -> np.ndarray:
        """test hook (fhe_switched_unpack_rows): k_ms_unpack over a scratch buffer, returned as switched_unpack_host
        lays its rows out.  Needs no server key."""
        h = self._h
        return _switched_unpack(lambda *a: load().fhe_switched_unpack_rows(h, *a), packed, n, stride)

    def time_switched(self, count: int, n: int, reps: int = 30):
        """measurement hook (fhe_ctx_time_switched): mean ms of one k_ms_pack and of one k_ms_unpack launch over
        count workspace rows"""
        a, b = C.c_float(), C.c_float()
        check(load().fhe_ctx_time_switched(self._h, int(count), int(n), int(reps), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def set_client_key(self, ck: "ClientKey") -> None:
        """after set_server_key, for a process that holds the client key anyway (fhe_ctx_set_client_key): the big
        secret key's 2048 bits become resident on the GPU, and encryptions and decryptions that pass this key run
        there.  A server that only evaluates never calls it."""
        check(load().fhe_ctx_set_client_key(self._h, ck.handle))

    def clear_client_key(self) -> None:
        """zeros over the resident key's device and host copies, then frees them (fhe_ctx_clear_client_key)"""
        check(load().fhe_ctx_clear_client_key(self._h))

    def client_ops_info(self):
        """(a key is resident, blocks encrypted on the device path, blocks whose phase was taken there)"""
        r, a, b = C.c_int(), C.c_uint64(), C.c_uint64()
        check(load().fhe_ctx_client_ops_info(self._h, C.byref(r), C.byref(a), C.byref(b)))
        return bool(r.value), int(a.value), int(b.value)

    def client_encrypt_rows(self, ck: "ClientKey", values) -> np.ndarray:
        """test hook (fhe_client_encrypt_rows): the encryption kernel into scratch rows under the resident key,
        returned as ClientKey.encrypt_blocks returns its rows; ck's stream advances the same way"""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
        out = np.zeros((v.size, BIG_CT), np.uint64)
        check(load().fhe_client_encrypt_rows(self._h, ck.handle, ptr(v), v.size, ptr(out)))
        return out

    def client_phase_rows(self, cts) -> np.ndarray:
        """test hook (fhe_client_phase_rows): the phase kernel over a scratch copy of the rows"""
        cts = np.ascontiguousarray(np.asarray(cts, dtype=np.uint64).reshape(-1, BIG_CT))
        out = np.zeros(cts.shape[0], np.uint64)
        check(load().fhe_client_phase_rows(self._h, ptr(cts), cts.shape[0], ptr(out)))
        return out

    def time_client_ops(self, count: int, iters: int = 30):
        """measurement hook (fhe_ctx_time_client_ops): mean ms of one encryption and of one phase kernel launch
        over count scratch rows"""
        a, b = C.c_float(), C.c_float()
        check(load().fhe_ctx_time_client_ops(self._h, int(count), int(iters), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def set_wide_threshold(self, threshold: int) -> None:
        check(load().fhe_ctx_set_wide_threshold(self._h, int(threshold)))

    # ---- multi-GPU fan-out (one process per GPU)
    def attach_comm(self, unique_id: bytes, nranks: int, rank: int, timeout_ms: int = 120000) -> None:
        """non-blocking RCCL init polled against `timeout_ms`: a peer that never joins gives an error
        (FHE_ERR_TIMEOUT), not a hang"""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(load().fhe_ctx_attach_comm_timeout(self._h, buf, nranks, rank, int(timeout_ms)))

    def set_comm_timeout(self, timeout_ms: int) -> None:
        """the attached communicator's deadline: time a bounded wait may pass without progress"""
        check(load().fhe_ctx_set_comm_timeout(self._h, int(timeout_ms)))

    def ready(self) -> bool:
        """the context exists and its device is usable (checked before any collective is entered)"""
        return bool(getattr(self, "_h", None)) and load().fhe_ctx_sync(self._h) == 0

    def broadcast_server_key(self, root: int = 0) -> None:
        """collective: replicate rank `root`'s installed server key to every rank (RCCL)"""
        check(load().fhe_ctx_broadcast_server_key(self._h, int(root)))
        p = FheParams()
        check(load().fhe_ctx_params(self._h, C.byref(p)))
        self.params = p

    def detach_comm(self) -> None:
        check(load().fhe_ctx_detach_comm(self._h))

    def set_fanout(self, min_level: int = 257, emulate_ranks: int = 0) -> None:
        check(load().fhe_ctx_set_fanout(self._h, int(min_level), int(emulate_ranks)))

    def fanout_info(self):
        r, n, lv = C.c_int(), C.c_int(), C.c_uint64()
        check(load().fhe_ctx_fanout_info(self._h, C.byref(r), C.byref(n), C.byref(lv)))
        return int(r.value), int(n.value), int(lv.value)

    def enable_timing(self, on: bool = True) -> None:
        check(load().fhe_ctx_enable_timing(self._h, 1 if on else 0))

    def last_pbs_timing(self):
        ks, br = C.c_float(), C.c_float()
        check(load().fhe_ctx_last_pbs_timing(self._h, C.byref(ks), C.byref(br)))
        return float(ks.value), float(br.value)

    def enable_clock(self, on: bool = True) -> None:
        """clock probe of the throughput blind rotate (fhe_ctx_enable_clock); enabling resets its sums"""
        check(load().fhe_ctx_enable_clock(self._h, 1 if on else 0))

    def read_clock(self):
        """(shader cycles, 100 MHz ticks, workgroups) summed over the probed launches' workgroups"""
        cy, tk, wg = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(load().fhe_ctx_read_clock(self._h, C.byref(cy), C.byref(tk), C.byref(wg)))
        return int(cy.value), int(tk.value), int(wg.value)


class SimContext(Context):
    """Test hook (fhe_host_sim_ctx_create): a context without a device, whose engine shadows every block's
    plaintext on the host.  set_server_key(SimContext()) makes FheUint / BigUintFHE run through the C ABI's
    real code on the CPU; SimKey() stands where a client key is asked for.  What needs device memory or a real
    key raises FheError.  The shadow evaluates a bootstrap when it is recorded: a decryption sees every recorded
    graph and every value; the launch order is seen through the launch trace (trace_enable / trace_read)."""

    def __init__(self):
        h = C.c_void_p()
        check(load().fhe_host_sim_ctx_create(C.byref(h)))
        self._h = h
        self.params = default_params()
        self._comp_params = None


class SimKey:
    """The key of a SimContext's encryptions and decryptions: a NULL handle, which only that context accepts."""
    handle = None
    params = None


def noise_audit(ctx: Context, reset: bool = False):
    """(largest label, largest merged noise, bootstraps whose merged noise exceeds their label) since the last
    reset (fhe_ctx_noise_audit): the budget of 25 units is held against the merged figure."""
    a, b, n = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(load().fhe_ctx_noise_audit(ctx.handle, C.byref(a), C.byref(b), C.byref(n), 1 if reset else 0))
    return int(a.value), int(b.value), int(n.value)


TUNE_KEYS = {"kara_min": 1, "kara_compat_min": 2, "kara_force": 3, "div_r16_lead": 4, "scalar_div_residue": 5,
             "flush_depth": 6}
FAULT_SITES_KEY, FAULT_AFTER_KEY = 7, 8
FAULT_LEVEL, FAULT_STAGE, FAULT_WORKSPACE, FAULT_DEFERRED, FAULT_RECORD, FAULT_CLIENT = 1, 2, 4, 8, 16, 32
FAULT_ALL = 63


def fault_arm(sites: int, after: int = 0) -> int:
    """Test hook (FHE_TUNE_FAULT_SITES / FHE_TUNE_FAULT_AFTER): enable the sites and let their `after`-th crossing
    from now on fail its call with FHE_ERR_HIP, "injected fault at <site>" (0: only count).  Returns the crossings
    counted since the hook was last armed.  Process-wide; fault_arm(0) turns it off."""
    prev = C.c_int64()
    check(load().fhe_host_set_tuning(FAULT_SITES_KEY, int(sites), None))
    check(load().fhe_host_set_tuning(FAULT_AFTER_KEY, int(after), C.byref(prev)))
    return int(prev.value)


@contextlib.contextmanager
def tuning(**values):
    """Test hook (fhe_host_set_tuning): move the radix algorithms' size rules for the duration of a
    with-block -- e.g. tuning(kara_min=6) -- and restore them after.  Process-wide."""
    old = {}
    try:
        for k, v in values.items():
            prev = C.c_int64()
            check(load().fhe_host_set_tuning(TUNE_KEYS[k], int(v), C.byref(prev)))
            old[k] = prev.value
        yield
    finally:
        for k, v in old.items():
            check(load().fhe_host_set_tuning(TUNE_KEYS[k], v, None))
