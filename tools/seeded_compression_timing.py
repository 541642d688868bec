#!/usr/bin/env python3
"""Bringing a serialized compression key to the GPU: the seeded form (fhe_seeded_compression_key_deserialize +
fhe_set_compression_key_seeded + fhe_ctx_sync) against the full kind-8 form (fhe_compression_key_deserialize +
fhe_set_compression_key + fhe_ctx_sync), the same key at the default parameters.  Same process, alternating,
medians after warm-ups; a record, not a pass / fail condition.  The claim of the seeded form is the BYTES.

    python tools/seeded_compression_timing.py [--reps 15] [--warmup 3] [--out FILE]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/seeded_compression_timing.py --kernels
    python tools/seeded_compression_timing.py --analyze DIR [--out FILE]    # per-kernel medians of the installs
"""
import argparse
import csv
import ctypes as C
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

import numpy as np  # noqa: E402

from fhe_sign import CompressionKeys, Context, default_compression_params, generate_keys  # noqa: E402
from fhe_sign._lib import check, load  # noqa: E402

KERNELS = ("k_expand_pksk_planes", "k_pksk_to_planes", "k_expand_bsk_fourier", "k_bsk_to_fourier", "k_bsk_to_e")


def setup():
    ck, sk = generate_keys(seed=0x71AE)
    _, sck = CompressionKeys.generate_compressed(ck)
    seeded = sck.serialize()
    full = sck.decompress().serialize()  # the same key, every mask word included
    del sck
    ctx = Context(0)
    ctx.set_server_key(sk)
    lib = load()
    paths = (("seeded", lib.fhe_seeded_compression_key_deserialize, lib.fhe_set_compression_key_seeded,
              lib.fhe_seeded_compression_key_destroy, seeded),
             ("full", lib.fhe_compression_key_deserialize, lib.fhe_set_compression_key,
              lib.fhe_compression_key_destroy, full))
    return ctx, paths


def via(ctx, deserialize, install, destroy, blob):
    lib = load()
    h = C.c_void_p()
    t0 = time.perf_counter()
    check(deserialize(blob, len(blob), C.byref(h)))
    t1 = time.perf_counter()
    check(install(ctx.handle, h))
    check(lib.fhe_ctx_sync(ctx.handle))
    t2 = time.perf_counter()
    destroy(h)
    return t2 - t0, t1 - t0


def wall(reps, warmup):
    ctx, paths = setup()
    times = {p[0]: [] for p in paths}
    state = {}
    for i in range(warmup + reps):
        for pname, de, inst, destroy, blob in paths:
            dt = via(ctx, de, inst, destroy, blob)
            if i == 0:  # both paths leave the same key on the device
                ctx._comp_params = default_compression_params()  # installed through the C ABI, not the wrapper
                state[pname] = [a.view(np.uint64 if a.dtype == np.float64 else np.uint8) for a in ctx.export_compression_state()]
            if i >= warmup:
                times[pname].append(dt)
    assert all(np.array_equal(a, b) for a, b in zip(state["seeded"], state["full"]))
    ctx.close()
    lines = [f"defaults (k' 4, N' 256, level 4): serialized compression key -> installed (wall clock to fhe_ctx_sync), "
             f"{reps} alternating runs after {warmup} warm-ups"]
    for pname, *_, blob in paths:
        tot = sorted(t[0] for t in times[pname])
        de = statistics.median(t[1] for t in times[pname])
        lines.append(f"  {pname:7s} {len(blob):10d} bytes  median {1e3 * statistics.median(tot):8.2f} ms  "
                     f"min {1e3 * tot[0]:8.2f}  max {1e3 * tot[-1]:8.2f}  (of which deserialize {1e3 * de:7.2f})")
        lines.append("          runs, in order: " + " ".join(f"{1e3 * t[0]:.1f}" for t in times[pname]))
    lines.append(f"  bytes: {len(paths[1][4])} / {len(paths[0][4])} = {len(paths[1][4]) / len(paths[0][4]):.2f}x")
    return lines


def kernels():
    """the workload of the rocprofv3 run: five installs of each form"""
    ctx, paths = setup()
    for _ in range(5):
        for _, de, inst, destroy, blob in paths:
            via(ctx, de, inst, destroy, blob)
    ctx.close()
    print("kernels: done")


def analyze(d):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    groups = {}
    for r in csv.DictReader(open(f)):
        short = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
        if short is None:
            continue
        grid = int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0) * int(r.get("Grid_Size_Y") or 1)
        wg = int(r.get("Workgroup_Size_X") or r.get("Workgroup_Size") or 1)
        groups.setdefault((short, grid // wg), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    lines = ["per-kernel device time (rocprofv3 --kernel-trace), median over the dispatches of one shape",
             f"  {'kernel':22s} {'workgroups':>10s} {'dispatches':>10s} {'median us':>10s} {'min us':>10s}"]
    for (name, wgs), ds in sorted(groups.items()):
        lines.append(f"  {name:22s} {wgs:10d} {len(ds):10d} {statistics.median(ds) / 1e3:10.1f} {min(ds) / 1e3:10.1f}")
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
