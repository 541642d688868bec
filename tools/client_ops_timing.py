#!/usr/bin/env python3
"""What the two host ends of a client-side call cost, and what the resident client key makes of them.
Two contexts under one server key in one process: A holds the client key resident (device paths), B holds none
(host paths, the parent commit's code).  Every wall-clock case runs A and B alternately in one loop, after a
warm-up, and reports the median and the range.  A record, not a pass / fail condition.

  - client_ops.hip's two kernels alone by HIP events (fhe_ctx_time_client_ops) at 128, 256 and 32768 blocks;
  - a 256-bit value to a usable operand (BigUintFHE.new: 128 blocks);
  - a resident 256-bit value (128 clean blocks) and the signer's column form (544 bits at the default limbs) to plaintext;
  - sign_fhe_with_k0 on BIP-340 vector 0, the call-site form and the fused one.

    python tools/client_ops_timing.py [--reps 15] [--warmup 3] [--out profiles/r23/client_ops_timing.txt]
"""
import argparse
import csv
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

from fhe_sign import (COMPAT, BigUintFHE, ClientKey, Context, Schnorr, _lib, compute_nonce, generate_keys,  # noqa: E402
                      set_server_key)


def med(xs):
    xs = sorted(xs)
    return statistics.median(xs), xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "client_ops_timing.txt"))
    a = ap.parse_args()
    reps = max(15, a.reps)
    lib = _lib.load()
    ck, sk = generate_keys(seed=0x71B0)
    kb = ck.serialize()
    A, B = Context(0), Context(0)
    A.set_server_key(sk)
    B.set_server_key(sk)
    A.set_client_key(ck)
    keys = {A: ClientKey.deserialize(kb), B: ClientKey.deserialize(kb)}
    names = {A: "device", B: "host"}
    lines = ["client_ops.hip alone (HIP events; each figure the mean of 20 back-to-back launches, median / min / max of 7 such "
             "figures after one discarded):"]
    for rows in (128, 256, 32768):
        A.time_client_ops(rows, 20)
        t = [A.time_client_ops(rows, 20) for _ in range(7)]
        for k, name in ((0, "k_client_encrypt"), (1, "k_client_phase  ")):
            m, lo, hi = med([x[k] for x in t])
            mb = rows * 2049 * 8 / 1e6
            lines.append(f"  {name} {rows:6d} blocks  {1e3 * m:9.2f} us  ({1e3 * lo:.2f} .. {1e3 * hi:.2f})   {mb:8.2f} MB of rows   "
                         f"{mb / m:8.1f} GB/s")

    def timed(ctx, fn):
        set_server_key(ctx)
        ctx.sync()
        t0 = time.perf_counter()
        x = fn(ctx, keys[ctx])
        ctx.sync()
        return time.perf_counter() - t0, x

    def alternate(title, fn, check=None):
        times = {A: [], B: []}
        for i in range(a.warmup + reps):
            for ctx in (A, B):
                dt, x = timed(ctx, fn)
                if check is not None:
                    check(x)
                if i >= a.warmup:
                    times[ctx].append(dt)
                del x
        lines.append(f"{title}, wall clock incl. the final wait, {reps} alternating runs after {a.warmup} warm-ups:")
        for ctx in (B, A):
            m, lo, hi = med(times[ctx])
            lines.append(f"  {names[ctx]:6s} path   median {1e3 * m:8.3f} ms   min {1e3 * lo:8.3f}   max {1e3 * hi:8.3f}")

    value = (1 << 256) - 0xF11E51
    alternate("a 256-bit value to a usable operand (BigUintFHE.new, 128 blocks)", lambda ctx, k: BigUintFHE.new(value, k))

    resident = {}
    cols = {}
    for ctx in (A, B):
        set_server_key(ctx)
        resident[ctx] = BigUintFHE.new(value, keys[ctx])
        e, d, k = (BigUintFHE.new(v, keys[ctx]) for v in (value - 12345, value // 3, value // 7))
        h = C.c_void_p()
        _lib.check(lib.fhe_biguint_mul_add_columns(ctx.handle, e.handle, d.handle, k.handle, COMPAT, C.byref(h)))
        bits = C.c_uint32()
        _lib.check(lib.fhe_columns_bits(h, C.byref(bits)))
        cols[ctx] = (h, int(bits.value))

    def read_cols(ctx, k):
        h, bits = cols[ctx]
        w = np.zeros((bits + 63) // 64, np.uint64)
        _lib.check(lib.fhe_columns_decrypt(ctx.handle, k.handle, h, _lib.ptr(w), w.size))
        return sum(int(x) << (64 * i) for i, x in enumerate(w))

    def same(box):
        def check(x):
            box.setdefault("v", x)
            assert box["v"] == x
        return check

    alternate("a resident 256-bit value (128 clean blocks) to plaintext", lambda ctx, k: resident[ctx].to_biguint(k), same({}))
    alternate(f"the signer's column form ({cols[A][1]} bits, launched) to plaintext", read_cols, same({}))
    for h, _ in cols.values():
        lib.fhe_columns_destroy(h)

    row = next(r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv"))) if r["index"] == "0")
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    s = Schnorr()
    dk = {}
    for ctx in (A, B):
        set_server_key(ctx)
        dk[ctx] = BigUintFHE.new(d, keys[ctx])

    def is_row0(sig):
        assert sig.hex().upper() == row["signature"].upper()

    alternate("sign_fhe_with_k0, BIP-340 vector 0, the call-site form (new, new, mul, add, to_biguint)",
              lambda ctx, k: s.sign_fhe_with_k0_callsite(msg, k0, d, dk[ctx], k, COMPAT), is_row0)
    alternate("sign_fhe_with_k0, BIP-340 vector 0, the fused call",
              lambda ctx, k: s.sign_fhe_with_k0(msg, k0, d, dk[ctx], k, COMPAT), is_row0)
    res, enc, ph = A.client_ops_info()
    lines.append(f"device-path blocks over the run: {enc} encrypted, {ph} phases; the host-path context: {B.client_ops_info()[1:]}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    set_server_key(None)
    del resident, dk
    A.close()
    B.close()


if __name__ == "__main__":
    main()
