#!/usr/bin/env python3
"""What an oblivious pseudo-random value costs (fhe_radix_random / fhe_biguint_random, oprf.hip): k_oprf_rows alone by
HIP events (fhe_ctx_time_oprf_rows) at 128, 256 and 32768 rows of n = 834, next to the keyswitch it stands in for
at the same counts (fhe_pbs_batch_device under enable_timing); and seed -> usable 256-bit operand
(BigUintFHE.random(256), 128 blocks) against the other ways a 256-bit operand reaches the GPU -- the seeded
ciphertext's expansion and the full ciphertext's upload, both from their serialized bytes -- and against a
128-bootstrap latency level.  One process, the wall-clock cases alternated, medians after a warm-up.  A record,
not a pass / fail condition.

    python tools/oprf_timing.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import (BigUintFHE, CompressedBigUintFHE, Context, generate_keys, rerandomization_seed,  # noqa: E402
                      set_server_key)


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ck, sk = generate_keys(seed=0x71B0)
    n = ck.params.lwe_dimension
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    lines = [f"k_oprf_rows alone, n = {n} (HIP events; each figure the mean of 50 back-to-back launches, median / min / max of 7 "
             "such figures after one discarded):"]
    for rows in (128, 256, 32768):
        ctx.time_oprf_rows(rows, n, 50)
        m, lo, hi = med([ctx.time_oprf_rows(rows, n, 50) for _ in range(7)])
        stored = rows * ((n + 8) // 8 * 8) * 8
        lines.append(f"  {rows:6d} rows  {1e3 * m:8.2f} us  ({1e3 * lo:.2f} .. {1e3 * hi:.2f})   {stored / 1e6:8.2f} MB stored   "
                     f"{stored / m / 1e6:8.1f} GB/s")
    lines.append(f"PBS levels of the same counts (fhe_pbs_batch_device, HIP events), median of {a.reps} after {a.warmup}; "
                 "ks = the keyswitch the row kernel stands in for, br = blind rotation")
    lid = ctx.lut([(3 * m + 1) % 16 for m in range(16)])
    base = ck.encrypt_blocks([i % 16 for i in range(64)])
    ctx.enable_timing(True)
    for B in (128, 256, 32768):
        cts = np.resize(base, (B, 2049))
        d_in, d_out, d_lut = ctx.alloc(cts.nbytes), ctx.alloc(cts.nbytes), ctx.alloc(4 * B)
        ctx.h2d(d_in, cts)
        ctx.h2d(d_lut, np.full(B, lid, np.uint32))
        reps = a.reps if B < 32768 else max(3, a.reps // 4)
        t = []
        for i in range(a.warmup + reps):
            ctx.pbs_device(d_in, B, d_lut, d_out)
            ctx.sync()
            if i >= a.warmup:
                t.append(ctx.last_pbs_timing())
        ks, br = (statistics.median(x[k] for x in t) for k in (0, 1))
        lines.append(f"  B = {B:6d} ({reps} runs)  ks {1e3 * ks:10.2f} us   br {br:9.4f} ms   level {ks + br:9.4f} ms")
        for p in (d_in, d_out, d_lut):
            ctx.free(p)
    ctx.enable_timing(False)

    # a 256-bit operand on the GPU, four ways
    value = (1 << 256) - 0xF11E51
    seeded = CompressedBigUintFHE.new(value, ck).serialize()
    full = BigUintFHE.new(value, ck).serialize()
    seeds = [rerandomization_seed(b"oprf-timing", i.to_bytes(4, "little")) for i in range(a.warmup + a.reps)]

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        x = fn()
        ctx.sync()
        return time.perf_counter() - t0, x

    cases = {
        "random(256)": lambda i: BigUintFHE.random(256, seeds[i]),
        "seeded expansion": lambda i: CompressedBigUintFHE.deserialize(seeded).decompress(),
        "full upload": lambda i: BigUintFHE.deserialize(full),
    }
    times = {k: [] for k in cases}
    for i in range(a.warmup + a.reps):
        for name, fn in cases.items():
            dt, x = timed(lambda: fn(i))
            if i == 0 and name != "random(256)":
                assert sum(v << (32 * k) for k, v in enumerate(x.decrypt_limbs(ck))) == value
            if i >= a.warmup:
                times[name].append(dt)
            del x
    lines.append(f"a 256-bit operand (128 blocks) resident on the GPU, wall clock incl. the final wait, {a.reps} alternating runs "
                 f"after {a.warmup} warm-ups:")
    sizes = {"random(256)": 32, "seeded expansion": len(seeded), "full upload": len(full)}
    for name in cases:
        m, lo, hi = med(times[name])
        lines.append(f"  {name:17s} {sizes[name]:9d} bytes in   median {1e3 * m:8.3f} ms   min {1e3 * lo:8.3f}   max {1e3 * hi:8.3f}")
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
