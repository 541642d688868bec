#!/usr/bin/env python3
"""Digesting an operand that already sits on the GPU: fhe_biguint_digest (k_ct_digest, 32 bytes per block back)
at 128 blocks (a 256-bit operand) and 4096 blocks, against, in the same run, the host route it replaces --
export() of the blocks (16 KB each over the bus) plus fhe_ct_digest_host -- and the re-randomization the digest
feeds (fhe_biguint_rerandomize).  Wall clock to the returned bytes (re-randomize: to fhe_ctx_sync), alternating,
medians after a warm-up; and k_ct_digest alone by HIP events (fhe_ctx_time_ct_digest), every run listed.  A
record, not a pass / fail condition.

    python tools/ct_digest_timing.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import BigUintFHE, CompactPublicKey, Context, ct_digest_host, generate_keys, set_server_key  # noqa: E402
from fhe_sign._lib import check, load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = load()
    ck, sk = generate_keys(seed=0x71B0)
    pk = CompactPublicKey.new(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_public_key(pk)
    set_server_key(ctx)
    seed = bytes(range(32))
    lines = [f"digesting a GPU operand, {a.reps} alternating runs after {a.warmup} warm-ups, wall clock to the returned bytes",
             f"host route: export() + fhe_ct_digest_host on {os.cpu_count()} host threads at most"]
    for blocks in (128, 4096):
        limbs = blocks // 16
        value = (1 << (32 * limbs)) - 0xF11E51
        x = BigUintFHE.new(value, ck)
        # the host route's export in as few calls as the API allows: radix views of up to 2048 blocks (4096 bits)
        ds = x.digits
        digits = [BigUintFHE.from_encrypted_digits(ds[i:i + 128]).to_radix(32 * len(ds[i:i + 128])) for i in range(0, limbs, 128)]
        del ds
        ctx.sync()

        def device():
            out = (C.c_uint8 * 32)()
            t0 = time.perf_counter()
            check(lib.fhe_biguint_digest(ctx.handle, x.handle, out))
            return time.perf_counter() - t0, bytes(out)

        def host():
            t0 = time.perf_counter()
            rows = np.concatenate([d.export() for d in digits])
            d = ct_digest_host(rows)
            return time.perf_counter() - t0, d

        def rerand():
            h = C.c_void_p()
            t0 = time.perf_counter()
            check(lib.fhe_biguint_rerandomize(ctx.handle, x.handle, seed, C.byref(h)))
            check(lib.fhe_ctx_sync(ctx.handle))
            dt = time.perf_counter() - t0
            lib.fhe_biguint_destroy(h)
            return dt, None

        ways = (("device digest", device), ("host route", host), ("re-randomize alone", rerand))
        times = {name: [] for name, _ in ways}
        for i in range(a.warmup + a.reps):
            for name, fn in ways:
                dt, _ = fn()
                if i >= a.warmup:
                    times[name].append(dt)
        lines.append(f"{blocks} blocks ({32 * limbs}-bit operand, {blocks * 2049 * 8} bytes resident)")
        med = {}
        for name, _ in ways:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:24s} median {1e3 * med[name]:9.3f} ms  min {1e3 * t[0]:9.3f}  max {1e3 * t[-1]:9.3f}")
        lines.append(f"  device digest / host route = {med['device digest'] / med['host route']:.4f};  / re-randomize alone = "
                     f"{med['device digest'] / med['re-randomize alone']:.3f}")
        # the kernel alone, HIP events: `reps` measurements of the mean of 10 back-to-back launches
        ev = [1e3 * ctx.time_ct_digest(blocks, 10) for _ in range(a.warmup + a.reps)][a.warmup:]
        lines.append(f"  k_ct_digest alone (HIP events, mean of 10 launches per run): median {statistics.median(ev):8.1f} us  "
                     f"min {min(ev):8.1f}  max {max(ev):8.1f}")
        lines.append("    runs: " + " ".join(f"{u:.1f}" for u in ev))
        del x, digits
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
