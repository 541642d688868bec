"""Schnorr / BIP-340 signer (src/schnorr.rs) over the C ABI.

`Schnorr` mirrors the reference struct: sign, sign_with_k0, sign_fhe, sign_fhe_with_k0, verify,
plus compute_nonce / get_public_key_with_even_y.  Scalars are Python ints; signatures bytes.
"""
from __future__ import annotations

import ctypes as C

from ._lib import check, load
from .integer import COMPAT, _ctx


CURVE_ORDER = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141  # secp256k1 n


def _b32(x: int) -> bytes:
    return int(x).to_bytes(32, "big")


def _buf(b: bytes):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if b else b"\0")


def public_key_x(privkey: int) -> bytes:
    out = (C.c_uint8 * 32)()
    check(load().fhe_schnorr_public_key(_buf(_b32(privkey)), out))
    return bytes(out)


def compute_nonce(privkey: int, message: bytes, aux_rand: bytes) -> int:
    out = (C.c_uint8 * 32)()
    check(load().fhe_schnorr_compute_nonce(_buf(_b32(privkey)), _buf(message), len(message), _buf(aux_rand), out))
    return int.from_bytes(bytes(out), "big")


class Schnorr:
    def sign(self, message: bytes, aux_rand: bytes, privkey: int) -> bytes:
        sig = (C.c_uint8 * 64)()
        check(load().fhe_schnorr_sign(_buf(message), len(message), _buf(aux_rand), _buf(_b32(privkey)), sig))
        return bytes(sig)

    def sign_with_k0(self, message: bytes, k0: int, privkey: int) -> bytes:
        sig = (C.c_uint8 * 64)()
        check(load().fhe_schnorr_sign_with_k0(_buf(message), len(message), _buf(_b32(k0)), _buf(_b32(privkey)), sig))
        return bytes(sig)

    def sign_prologue(self, message: bytes, k0: int, privkey: int):
        """(k, e, r_x) of sign_fhe_with_k0's plaintext steps 1-5 (src/schnorr.rs:239-267)"""
        k, e, rx = (C.c_uint8 * 32)(), (C.c_uint8 * 32)(), (C.c_uint8 * 32)()
        check(load().fhe_schnorr_sign_prologue(_buf(message), len(message), _buf(_b32(k0)), _buf(_b32(privkey)), k, e,
                                               rx))
        return int.from_bytes(bytes(k), "big"), int.from_bytes(bytes(e), "big"), bytes(rx)

    def eval_s(self, e, k, privkey_fhe, mode: int = COMPAT):
        """The server's half of the signature alone: Enc(s), s = (k + e * d') mod n, as an FheUint256 -- no client
        key involved, so whoever holds it decrypts 256 bits that are the signature's s and nothing else.
        mode COMPAT / FAST: e and k are BigUintFHE (fhe_schnorr_eval_s); mode PUBLIC: e and k are ints below n
        (fhe_schnorr_eval_s_public).  (k, e) come from sign_prologue."""
        from .integer import PUBLIC, FheUint
        h = C.c_void_p()
        if mode == PUBLIC:
            e, k = int(e), int(k)
            if not (0 <= e < CURVE_ORDER and 0 <= k < CURVE_ORDER):
                raise ValueError("e and k must be below the curve order")
            check(load().fhe_schnorr_eval_s_public(_ctx().handle, _buf(_b32(e)), _buf(_b32(k)), privkey_fhe.handle,
                                                   C.byref(h)))
        else:
            check(load().fhe_schnorr_eval_s(_ctx().handle, e.handle, k.handle, privkey_fhe.handle, mode, C.byref(h)))
        return FheUint._wrap(h, 256)

    def sign_fhe_with_k0_callsite(self, message: bytes, k0: int, privkey: int, privkey_fhe, client_key,
                                  mode: int = COMPAT, reduce: bool = False) -> bytes:
        """sign_fhe_with_k0 exactly as the reference's call site runs it (src/schnorr.rs:271-276), each
        operator through its own C entry point -- what INTEGRATION.md 2's impl Add / impl Mul binding
        dispatches: e_fhe = BigUintFHE::new(e), k_fhe = BigUintFHE::new(k), k_fhe + (e_fhe * privkey_fhe),
        to_biguint, % n.  Signature identical to sign_fhe_with_k0 (which fuses the block into one
        column-form schedule).  reduce: the sum is reduced mod n under encryption (rem_pseudo_mersenne) and one
        256-bit decryption replaces to_biguint + % n."""
        from .integer import SECP256K1_N_C, BigUintFHE
        k, e, rx = self.sign_prologue(message, k0, privkey)
        e_fhe = BigUintFHE.new(e, client_key)
        k_fhe = BigUintFHE.new(k, client_key)
        if reduce:
            s = k_fhe.add(e_fhe.mul(privkey_fhe, mode), mode).rem_pseudo_mersenne(256, SECP256K1_N_C).decrypt(client_key)
            if s >= CURVE_ORDER:
                raise RuntimeError("reduced signer: the decrypted s is not below the curve order")
            return rx + _b32(s)
        s_without_mod = k_fhe.add(e_fhe.mul(privkey_fhe, mode), mode).to_biguint(client_key)
        return rx + _b32(s_without_mod % CURVE_ORDER)

    def sign_fhe_with_k0(self, message: bytes, k0: int, privkey: int, privkey_fhe, client_key, mode: int = COMPAT,
                         rerandomize_domain=None, reduce: bool = False) -> bytes:
        """rerandomize_domain (bytes): sign with a re-randomized copy of privkey_fhe, the seed bound to the domain,
        r_x || pubkey_x || message and the ciphertext's own digest (fhe_schnorr_sign_fhe_with_k0_rerand; needs
        Context.set_public_key).  The signature is the same bytes either way.
        reduce: s is reduced mod n under encryption (fhe_schnorr_sign_fhe_with_k0_reduced), so the one value this
        call decrypts is the signature's s (256 bits).  Without it the plaintext is k + e * d' (about 513 bits, the
        reference's behaviour), and floor of that over the public e is d' or a neighbour.  Same bytes either way."""
        sig = (C.c_uint8 * 64)()
        lib, sfx = load(), "_reduced" if reduce else ""
        if rerandomize_domain is not None:
            dom = bytes(rerandomize_domain)
            check(getattr(lib, "fhe_schnorr_sign_fhe_with_k0_rerand" + sfx)(
                _ctx().handle, client_key.handle, _buf(message), len(message), _buf(_b32(k0)), _buf(_b32(privkey)),
                privkey_fhe.handle, mode, dom, len(dom), sig))
            return bytes(sig)
        check(getattr(lib, "fhe_schnorr_sign_fhe_with_k0" + sfx)(
            _ctx().handle, client_key.handle, _buf(message), len(message), _buf(_b32(k0)), _buf(_b32(privkey)),
            privkey_fhe.handle, mode, sig))
        return bytes(sig)

    def sign_fhe_with_k0_batch(self, jobs, client_key, mode: int = COMPAT, reduce: bool = False) -> list:
        """jobs: [(message, k0, privkey, privkey_fhe)]; one engine schedule for all, signatures
        identical to sign_fhe_with_k0 one by one (reduce: as sign_fhe_with_k0's)"""
        n = len(jobs)
        bufs = [C.create_string_buffer(bytes(m), max(1, len(m))) for m, _, _, _ in jobs]
        msgs = (C.c_void_p * max(1, n))(*[C.cast(b, C.c_void_p) for b in bufs])
        lens = (C.c_size_t * max(1, n))(*[len(m) for m, _, _, _ in jobs])
        k0s = b"".join(_b32(k) for _, k, _, _ in jobs)
        pks = b"".join(_b32(d) for _, _, d, _ in jobs)
        fh = (C.c_void_p * max(1, n))(*[f.handle for _, _, _, f in jobs])
        sigs = C.create_string_buffer(64 * max(1, n))
        fn = load().fhe_schnorr_sign_fhe_with_k0_batch_reduced if reduce else load().fhe_schnorr_sign_fhe_with_k0_batch
        check(fn(_ctx().handle, client_key.handle, n, msgs, lens, k0s, pks, fh, mode, sigs))
        return [sigs.raw[64 * i:64 * i + 64] for i in range(n)]

    def sign_fhe(self, message: bytes, aux_rand: bytes, privkey: int, client_key, mode: int = COMPAT,
                 reduce: bool = False) -> bytes:
        if reduce:  # fhe_schnorr_sign_fhe's steps with the reduced signer in the middle
            from .integer import BigUintFHE
            _ctx()  # no server key on this thread: refuse before anything is computed
            k0 = compute_nonce(privkey, message, aux_rand)
            d_fhe = BigUintFHE.new(privkey % CURVE_ORDER, client_key)
            return self.sign_fhe_with_k0(message, k0, privkey, d_fhe, client_key, mode, reduce=True)
        sig = (C.c_uint8 * 64)()
        check(load().fhe_schnorr_sign_fhe(_ctx().handle, client_key.handle, _buf(message), len(message),
                                          _buf(aux_rand), _buf(_b32(privkey)), mode, sig))
        return bytes(sig)

    @staticmethod
    def verify(message: bytes, pubkey: bytes, sig: bytes) -> bool:
        return load().fhe_schnorr_verify(_buf(message), len(message), _buf(pubkey), len(pubkey), _buf(sig), len(sig)) == 1
