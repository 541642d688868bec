#!/usr/bin/env python3
"""Bringing a stored 256-bit ciphertext to the GPU: the seeded form (fhe_seeded_deserialize +
fhe_seeded_expand_radix + fhe_ctx_sync) against the full form (fhe_radix_deserialize + fhe_ctx_sync).
Same process, alternating, medians after a warm-up; a record, not a pass / fail condition.

    python tools/seeded_timing.py [--bits 256] [--reps 30] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import CompressedFheUint, Context, FheUint, generate_keys, set_server_key  # noqa: E402
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
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    value = (1 << a.bits) - 0xF11E51
    seeded = CompressedFheUint.try_encrypt(value, ck, bits=a.bits).serialize()
    full = FheUint.try_encrypt(value, ck, bits=a.bits).serialize()

    def via_seeded():
        s, h = C.c_void_p(), C.c_void_p()
        t0 = time.perf_counter()
        check(lib.fhe_seeded_deserialize(seeded, len(seeded), C.byref(s)))
        check(lib.fhe_seeded_expand_radix(ctx.handle, s, C.byref(h)))
        check(lib.fhe_ctx_sync(ctx.handle))
        dt = time.perf_counter() - t0
        lib.fhe_seeded_destroy(s)
        return dt, h

    def via_full():
        h = C.c_void_p()
        t0 = time.perf_counter()
        check(lib.fhe_radix_deserialize(ctx.handle, full, len(full), C.byref(h)))
        check(lib.fhe_ctx_sync(ctx.handle))
        return time.perf_counter() - t0, h

    times = {"seeded": [], "full": []}
    for i in range(a.warmup + a.reps):
        for name, fn in (("seeded", via_seeded), ("full", via_full)):
            dt, h = fn()
            if i == 0:  # both forms hold the value
                assert FheUint._wrap(C.c_void_p(h.value), a.bits).decrypt(ck) == value
            else:
                lib.fhe_radix_destroy(h)
            if i >= a.warmup:
                times[name].append(dt)
    lines = [f"stored {a.bits}-bit ciphertext -> GPU slots, {a.reps} alternating runs after {a.warmup} warm-ups, wall clock"]
    for name, blob in (("seeded", seeded), ("full", full)):
        t = sorted(times[name])
        lines.append(f"{name:7s} {len(blob):9d} bytes  median {1e3 * statistics.median(t):8.3f} ms  "
                     f"min {1e3 * t[0]:8.3f}  max {1e3 * t[-1]:8.3f}")
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
