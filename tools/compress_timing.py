#!/usr/bin/env python3
"""A computed 256-bit value between GPU slots and serialized bytes, both ways: the compressed list
(fhe_radix_compress + fhe_compressed_serialize; fhe_compressed_deserialize + fhe_compressed_expand_radix)
against the full blocks (fhe_radix_serialize; fhe_radix_deserialize).  One MI355X, one process, alternating,
medians after warm-ups, wall clock to fhe_ctx_sync; a record, not a pass / fail condition.  The claim is the
BYTES, which are exact by formula; the times are what they are, and the decompression bootstrap's share is
named (decompress = unpack + one blind rotation of 128 blocks at n = 1024).

    python tools/compress_timing.py [--reps 15] [--warmup 3] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/compress_timing.py --kernels
    python tools/compress_timing.py --analyze DIR [--out FILE]      # per-kernel medians at B = 128 and 32768
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

import numpy as np  # noqa: E402

from fhe_sign import (BigUintFHE, CompressedCiphertextList, CompressionKeys, Context, FheUint, generate_keys,  # noqa: E402
                      set_server_key)

KERNELS = ("k_pk_digits", "k_pk_mfma", "k_pk_pack", "k_pk_unpack", "k_blind_rotate", "k_ks_digits", "k_ks_mfma")


def setup():
    ck, sk = generate_keys(seed=0x71AE)
    priv, key = CompressionKeys.generate(ck)
    ctx = Context(0)
    ctx.set_server_key(sk)
    ctx.set_compression_key(key)
    set_server_key(ctx)
    return ck, priv, ctx


def med(ts):
    ts = sorted(ts)
    return f"median {1e3 * statistics.median(ts):8.3f} ms  min {1e3 * ts[0]:8.3f}  max {1e3 * ts[-1]:8.3f}"


def wall(reps, warmup):
    ck, priv, ctx = setup()
    v = int.from_bytes(np.random.default_rng(7).bytes(32), "little")
    x = FheUint.try_encrypt(v, ck, bits=256) + 1  # a computed value: bootstrapped blocks in engine slots
    ctx.sync()
    t = {k: [] for k in ("compress", "serialize", "full", "deserialize", "decompress", "full_back")}
    small = full = None
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        lst = x.compress()
        t1 = time.perf_counter()
        small = lst.serialize()
        t2 = time.perf_counter()
        full = x.serialize()
        t3 = time.perf_counter()
        back = CompressedCiphertextList.deserialize(small)
        t4 = time.perf_counter()
        y = back.decompress()
        ctx.sync()
        t5 = time.perf_counter()
        z = FheUint.deserialize(full)
        ctx.sync()
        t6 = time.perf_counter()
        if i == 0:
            assert back.decrypt(priv) == (v + 1) % 2**256 == y.decrypt(ck) == z.decrypt(ck)
        if i >= warmup:
            for k, dt in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, t6 - t5)):
                t[k].append(dt)
        del y, z
    both = [a + b for a, b in zip(t["compress"], t["serialize"])]
    back_ = [a + b for a, b in zip(t["deserialize"], t["decompress"])]
    lines = [f"a computed 256-bit value (128 blocks), {reps} alternating runs after {warmup} warm-ups, wall clock to fhe_ctx_sync",
             f"  GPU slots -> bytes   compressed {len(small):9d} bytes  {med(both)}  (compress {1e3 * statistics.median(t['compress']):.3f}, "
             f"serialize {1e3 * statistics.median(t['serialize']):.3f})",
             f"                       full       {len(full):9d} bytes  {med(t['full'])}",
             f"  bytes -> GPU slots   compressed {len(small):9d} bytes  {med(back_)}  (deserialize "
             f"{1e3 * statistics.median(t['deserialize']):.3f}, decompress = unpack + blind rotation of 128 blocks at n = 1024 "
             f"{1e3 * statistics.median(t['decompress']):.3f})",
             f"                       full       {len(full):9d} bytes  {med(t['full_back'])}",
             f"  bytes: {len(full)} / {len(small)} = {len(full) / len(small):.0f}x"]
    set_server_key(None)
    ctx.close()
    return lines


def kernels():
    """the workload of the per-kernel record: B = 128 and B = 32768 (a BigUintFHE of 2048 limbs), compressed and
    decompressed five times each; plus 128 and 32768 plain bootstraps, the keyswitch contraction's own shape"""
    ck, priv, ctx = setup()
    lut = ctx.lut(list(range(16)))
    for B in (128, 32768):
        cts = ck.encrypt_blocks(np.arange(B) % 4)
        x = BigUintFHE.deserialize(_raw_biguint(cts))
        for _ in range(5):
            lst = x.compress()
            y = lst.decompress()
            ctx.sync()
            del y
        for _ in range(3):
            ctx.pbs(cts, lut)
    set_server_key(None)
    ctx.close()
    print("kernels: done")


def _raw_biguint(cts):
    import struct
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import compress_ref as R
    return R.raw_biguint_blob(struct.pack("<9I", 834, 23, 3, 5, 45, 17, 4, 4, 1), cts, 3, 1)


def analyze(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    groups = {}
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        short = next((k for k in KERNELS if k in name), None)
        if short is None:
            continue
        if short == "k_pk_mfma":
            short += "<4>" if "Li4E" in name or "<4>" in name else "<1>"
        grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) * int(r.get("Grid_Size_Y") or 1)
        wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1)
        groups.setdefault((short, grid // wg), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    lines = ["per-kernel device time (rocprofv3 --kernel-trace), median over the dispatches of one shape",
             f"  {'kernel':18s} {'workgroups':>10s} {'dispatches':>10s} {'median us':>10s} {'min us':>10s}"]
    for (name, wgs), ds in sorted(groups.items()):
        lines.append(f"  {name:18s} {wgs:10d} {len(ds):10d} {statistics.median(ds) / 1e3:10.1f} {min(ds) / 1e3:10.1f}")
    # int8 rate of the two contractions at 32768 rows: 2 * rows * K * columns * 8 planes
    def rate(name, rows, K, cols):
        ds = [v for (n, _), v in groups.items() if n == name]
        if not ds:
            return None
        t = statistics.median(max(ds, key=lambda v: statistics.median(v))) * 1e-9
        return 2.0 * rows * K * cols * 8 / t
    pk, ks = rate("k_pk_mfma<4>", 32768, 8192, 1280), rate("k_ks_mfma", 32768, 10240, 835)
    if pk and ks:
        lines.append(f"  int8 rate at 32768 rows: packing contraction (8192 x 1280 x 8 planes) {pk / 1e12:.1f} Top/s, keyswitch "
                     f"(10240 x 835 x 8 planes) {ks / 1e12:.1f} Top/s: {pk / ks:.2f} of ks_mfma's")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--analyze", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels:
        return kernels()
    lines = analyze(a.analyze) if a.analyze else wall(a.reps, a.warmup)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.analyze else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
