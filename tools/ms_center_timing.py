#!/usr/bin/env python3
"""What the centered modulus switch (fhe_ctx_set_modulus_switch, ms_center.hip) costs: k_ms_center alone by HIP
events (fhe_ctx_time_ms_center) at 1, 256, 4096 and 32768 rows of n = 834 at the workspace's stride, and whole
PBS levels (fhe_pbs_batch_device under enable_timing: keyswitch and blind rotation by HIP events) at B = 1, 256
and 32768 in standard and centered mode, alternated in one process, medians after a warm-up.  In centered mode
the keyswitch figure includes k_ms_center (it is launched by fhe_ctx::keyswitch).  A record, not a pass / fail
condition.

    python tools/ms_center_timing.py [--reps 20] [--warmup 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import Context, generate_keys, ms_stride  # noqa: E402

MODES = ("standard", "centered")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ck, sk = generate_keys(seed=0x71AF)
    n = ck.params.lwe_dimension
    stride = ms_stride(n)
    ctx = Context(0)
    ctx.set_server_key(sk)
    lines = [f"k_ms_center alone, n = {n}, stride {stride} words (HIP events, mean of 50 back-to-back launches after 5):"]
    for rows in (1, 256, 4096, 32768):
        ctx.time_ms_center(rows, n, stride, 5)
        ms = ctx.time_ms_center(rows, n, stride, 50)
        moved = rows * (n + 2) * 8  # n + 1 words read, one written
        lines.append(f"  {rows:6d} rows  {1e3 * ms:8.2f} us   {moved / 1e6:8.2f} MB moved   {moved / ms / 1e6:8.1f} GB/s")
    lines.append(f"PBS levels (fhe_pbs_batch_device, HIP events), modes alternated, median of {a.reps} after {a.warmup} warm-ups; "
                 "ks = keyswitch (+ k_ms_center when centered), br = blind rotation")
    lid = ctx.lut([(3 * m + 1) % 16 for m in range(16)])
    base = ck.encrypt_blocks([i % 16 for i in range(64)])
    ctx.enable_timing(True)
    for B in (1, 256, 32768):
        cts = np.resize(base, (B, 2049))
        d_in, d_out, d_lut = ctx.alloc(cts.nbytes), ctx.alloc(cts.nbytes), ctx.alloc(4 * B)
        ctx.h2d(d_in, cts)
        ctx.h2d(d_lut, np.full(B, lid, np.uint32))
        reps = a.reps if B < 32768 else max(3, a.reps // 4)
        t = {m: [] for m in MODES}
        for i in range(a.warmup + reps):
            for m in MODES:
                ctx.set_modulus_switch(m)
                ctx.pbs_device(d_in, B, d_lut, d_out)
                ctx.sync()
                if i >= a.warmup:
                    t[m].append(ctx.last_pbs_timing())
        ctx.set_modulus_switch("standard")
        med = {m: [statistics.median(x[k] for x in t[m]) for k in (0, 1)] for m in MODES}
        spread = {m: max(sum(x) for x in t[m]) - min(sum(x) for x in t[m]) for m in MODES}
        lines.append(f"  B = {B} ({reps} runs each)")
        for m in MODES:
            ks, br = med[m]
            lines.append(f"    {m:9s} ks {ks:9.4f} ms   br {br:9.4f} ms   level {ks + br:9.4f} ms   (max - min of the level {spread[m]:.4f} ms)")
        d = sum(med["centered"]) - sum(med["standard"])
        lines.append(f"    centered - standard: {1e3 * d:+9.2f} us  ({100 * d / sum(med['standard']):+.3f} % of the level)")
        for p in (d_in, d_out, d_lut):
            ctx.free(p)
    ctx.enable_timing(False)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
