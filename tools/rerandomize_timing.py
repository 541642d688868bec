#!/usr/bin/env python3
"""Refreshing an operand that already sits on the GPU: fhe_biguint_rerandomize (a 32-byte seed; A and B of the
installed public key are resident) at 128 blocks (a 256-bit operand) and 4096 blocks, against, in the same run,
expand() of an unpacked compact list of the same block count (the same extraction traffic, but C_A / C_B come
over the bus) and fhe_biguint_deserialize of the full form (the only way to refresh an operand before; it needs
the client key and moves 16 KB per block).  Wall clock to fhe_ctx_sync, alternating, medians after a warm-up; and
k_rerand_zero alone by HIP events (fhe_ctx_time_rerand_zero).  A record, not a pass / fail condition.

    python tools/rerandomize_timing.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import BigUintFHE, CompactCiphertextList, CompactPublicKey, Context, generate_keys, set_server_key  # noqa: E402
from fhe_sign._lib import check, load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = load()
    ck, sk = generate_keys(seed=0x71AF)
    pk = CompactPublicKey.new(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    seed = bytes(range(32))
    lines = [f"refreshing a GPU operand, {a.reps} alternating runs after {a.warmup} warm-ups, wall clock incl. fhe_ctx_sync",
             f"public key: {len(pk.serialize())} bytes on the wire, 32 KB (A and B) resident; per call a 32-byte seed"]
    for blocks in (128, 4096):
        limbs = blocks // 16
        value = (1 << (32 * limbs)) - 0xF11E51
        x = BigUintFHE.new(value, ck)
        blobs = {"compact": CompactCiphertextList.builder(pk).push_biguint(value).build().serialize(), "full": x.serialize()}
        ctx.sync()

        def rerand():
            h = C.c_void_p()
            t0 = time.perf_counter()
            check(lib.fhe_biguint_rerandomize(ctx.handle, x.handle, seed, C.byref(h)))
            check(lib.fhe_ctx_sync(ctx.handle))
            return time.perf_counter() - t0, h

        def compact():
            s, h = C.c_void_p(), C.c_void_p()
            t0 = time.perf_counter()
            check(lib.fhe_compact_list_deserialize(blobs["compact"], len(blobs["compact"]), C.byref(s)))
            check(lib.fhe_compact_list_expand_biguint(ctx.handle, s, 0, C.byref(h)))
            check(lib.fhe_ctx_sync(ctx.handle))
            dt = time.perf_counter() - t0
            lib.fhe_compact_list_destroy(s)
            return dt, h

        def full():
            h = C.c_void_p()
            t0 = time.perf_counter()
            check(lib.fhe_biguint_deserialize(ctx.handle, blobs["full"], len(blobs["full"]), C.byref(h)))
            check(lib.fhe_ctx_sync(ctx.handle))
            return time.perf_counter() - t0, h

        ways = (("re-randomize", rerand, 32), ("compact expand", compact, len(blobs["compact"])),
                ("full deserialize", full, len(blobs["full"])))
        times = {name: [] for name, _, _ in ways}
        for i in range(a.warmup + a.reps):
            for name, fn, _ in ways:
                dt, h = fn()
                if i == 0:  # every way holds the value
                    assert BigUintFHE(C.c_void_p(h.value)).to_biguint(ck) == value, name
                else:
                    lib.fhe_biguint_destroy(h)
                if i >= a.warmup:
                    times[name].append(dt)
        lines.append(f"{blocks} blocks ({32 * limbs}-bit operand)")
        for name, _, nbytes in ways:
            t = sorted(times[name])
            lines.append(f"  {name:16s} {nbytes:9d} bytes in  median {1e3 * statistics.median(t):8.3f} ms  "
                         f"min {1e3 * t[0]:8.3f}  max {1e3 * t[-1]:8.3f}")
        ms = C.c_float()
        check(lib.fhe_ctx_time_rerand_zero(ctx.handle, seed, blocks, 5, C.byref(ms)))  # warm-up
        check(lib.fhe_ctx_time_rerand_zero(ctx.handle, seed, blocks, a.reps, C.byref(ms)))
        lines.append(f"  k_rerand_zero alone (HIP events, mean of {a.reps} back-to-back launches): {1e3 * ms.value:8.1f} us "
                     f"for {(blocks + 2047) // 2048} chunk(s)")
        del x
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
