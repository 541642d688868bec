#!/usr/bin/env python3
"""Bringing a serialized server key to the GPU: the seeded form (fhe_seeded_server_key_deserialize +
fhe_set_server_key_seeded + fhe_ctx_sync) against the full form (fhe_server_key_deserialize +
fhe_set_server_key + fhe_ctx_sync), the same key at n = 834, classic and then multi-bit parameters.
Same process, alternating, medians after warm-ups; a record, not a pass / fail condition.

    python tools/seeded_key_timing.py [--reps 15] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

import numpy as np  # noqa: E402

from fhe_sign import CompressedServerKey, Context, default_params, generate_keys, multi_bit_params  # noqa: E402
from fhe_sign._lib import check, load  # noqa: E402


def measure(name, params, reps, warmup):
    lib = load()
    ck, _ = generate_keys(params, seed=0x71AE)
    ssk = CompressedServerKey.new(ck)
    seeded = ssk.serialize()
    full = ssk.decompress().serialize()  # the same key, every mask word included
    del ssk
    ctx = Context(0)

    def via(deserialize, install, destroy, blob):
        h = C.c_void_p()
        t0 = time.perf_counter()
        check(deserialize(blob, len(blob), C.byref(h)))
        t1 = time.perf_counter()
        check(install(ctx.handle, h))
        check(lib.fhe_ctx_sync(ctx.handle))
        t2 = time.perf_counter()
        destroy(h)
        return t2 - t0, t1 - t0

    paths = (("seeded", lib.fhe_seeded_server_key_deserialize, lib.fhe_set_server_key_seeded,
              lib.fhe_seeded_server_key_destroy, seeded),
             ("full", lib.fhe_server_key_deserialize, lib.fhe_set_server_key, lib.fhe_server_key_destroy, full))
    times = {p[0]: [] for p in paths}
    fourier = {}
    for i in range(warmup + reps):
        for pname, de, inst, destroy, blob in paths:
            dt = via(de, inst, destroy, blob)
            if i == 0:  # both paths leave the same key on the device
                out = np.zeros(params.ggsw_count() * 4 * 1024 * 2, np.float64)
                check(lib.fhe_ctx_export_fourier_bsk(ctx.handle, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
                fourier[pname] = out.view(np.uint64)
            if i >= warmup:
                times[pname].append(dt)
    assert np.array_equal(fourier["seeded"], fourier["full"])
    ctx.close()
    lines = [f"{name}: serialized server key -> installed (wall clock to fhe_ctx_sync), {reps} alternating runs "
             f"after {warmup} warm-ups"]
    for pname, *_, blob in paths:
        tot = sorted(t[0] for t in times[pname])
        de = statistics.median(t[1] for t in times[pname])
        lines.append(f"  {pname:7s} {len(blob):10d} bytes  median {1e3 * statistics.median(tot):8.2f} ms  "
                     f"min {1e3 * tot[0]:8.2f}  max {1e3 * tot[-1]:8.2f}  (of which deserialize {1e3 * de:7.2f})")
        lines.append("          runs, in order: " + " ".join(f"{1e3 * t[0]:.1f}" for t in times[pname]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, params in (("classic n = 834", default_params()), ("multi-bit n = 834", multi_bit_params())):
        lines += measure(name, params, a.reps, a.warmup)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
