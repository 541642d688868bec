#!/usr/bin/env python3
"""Bringing a 256-bit ciphertext from bytes to a usable GPU operand, four ways: the compact list a holder of
the PUBLIC key made, packed (fhe_compact_list_deserialize + fhe_compact_list_expand_radix, which records the
unpacking bootstraps, + fhe_ctx_sync, which launches their one level) and unpacked, against the two forms only
the holder of the client key can make: the seeded form (fhe_seeded_deserialize + fhe_seeded_expand_radix +
fhe_ctx_sync) and the full form (fhe_radix_deserialize + fhe_ctx_sync).  Same process, alternating, medians
after a warm-up, wall clock; a record, not a pass / fail condition.

    python tools/compact_timing.py [--bits 256] [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import (CompactCiphertextList, CompactPublicKey, CompressedFheUint, Context, FheUint, generate_keys,  # noqa: E402
                      set_server_key)
from fhe_sign._lib import check, load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = load()
    ck, sk = generate_keys(seed=0x71AE)
    pk = CompactPublicKey.new(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    value = (1 << a.bits) - 0xF11E51
    blobs = {
        "packed": CompactCiphertextList.builder(pk).push(value, bits=a.bits).build_packed().serialize(),
        "unpacked": CompactCiphertextList.builder(pk).push(value, bits=a.bits).build().serialize(),
        "seeded": CompressedFheUint.try_encrypt(value, ck, bits=a.bits).serialize(),
        "full": FheUint.try_encrypt(value, ck, bits=a.bits).serialize(),
    }

    def via_compact(blob):
        def run():
            s, h = C.c_void_p(), C.c_void_p()
            t0 = time.perf_counter()
            check(lib.fhe_compact_list_deserialize(blob, len(blob), C.byref(s)))
            check(lib.fhe_compact_list_expand_radix(ctx.handle, s, 0, C.byref(h)))
            check(lib.fhe_ctx_sync(ctx.handle))  # packed: the unpacking level runs here
            dt = time.perf_counter() - t0
            lib.fhe_compact_list_destroy(s)
            return dt, h
        return run

    def via_seeded():
        s, h = C.c_void_p(), C.c_void_p()
        t0 = time.perf_counter()
        check(lib.fhe_seeded_deserialize(blobs["seeded"], len(blobs["seeded"]), C.byref(s)))
        check(lib.fhe_seeded_expand_radix(ctx.handle, s, C.byref(h)))
        check(lib.fhe_ctx_sync(ctx.handle))
        dt = time.perf_counter() - t0
        lib.fhe_seeded_destroy(s)
        return dt, h

    def via_full():
        h = C.c_void_p()
        t0 = time.perf_counter()
        check(lib.fhe_radix_deserialize(ctx.handle, blobs["full"], len(blobs["full"]), C.byref(h)))
        check(lib.fhe_ctx_sync(ctx.handle))
        return time.perf_counter() - t0, h

    ways = (("packed", via_compact(blobs["packed"])), ("unpacked", via_compact(blobs["unpacked"])),
            ("seeded", via_seeded), ("full", via_full))
    times = {name: [] for name, _ in ways}
    for i in range(a.warmup + a.reps):
        for name, fn in ways:
            dt, h = fn()
            if i == 0:  # every form holds the value
                assert FheUint._wrap(C.c_void_p(h.value), a.bits).decrypt(ck) == value, name
            else:
                lib.fhe_radix_destroy(h)
            if i >= a.warmup:
                times[name].append(dt)
    lines = [f"{a.bits}-bit ciphertext, bytes -> usable GPU operand, {a.reps} alternating runs after {a.warmup} warm-ups, "
             "wall clock incl. fhe_ctx_sync",
             f"public key: {len(pk.serialize())} bytes.  packed = extraction + one level of {a.bits // 2} unpacking bootstraps"]
    for name, _ in ways:
        t = sorted(times[name])
        who = "public key" if name in ("packed", "unpacked") else "client key"
        lines.append(f"{name:8s} ({who:10s}) {len(blobs[name]):9d} bytes  median {1e3 * statistics.median(t):8.3f} ms  "
                     f"min {1e3 * t[0]:8.3f}  max {1e3 * t[-1]:8.3f}")
    d = statistics.median(times["packed"]) - statistics.median(times["unpacked"])
    lines.append(f"packed - unpacked: {1e3 * d:.3f} ms (the unpacking level)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    set_server_key(None)
    ctx.close()


if __name__ == "__main__":
    main()
