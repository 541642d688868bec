#!/usr/bin/env python3
"""What reducing s mod n under encryption costs (fhe_schnorr_sign_fhe_with_k0_reduced, fhe_radix_rem_pseudo_mersenne):

  sign     sign_fhe_with_k0 on BIP-340 vectors 0 (a one-limb key) and 1 (eight limbs) with and without
           reduce=True, compat / fast / public-operand modes, the two alternated call by call; wall clock of
           the whole call (prologue, encryptions, FHE block, decryption); median / min / max.
           --unreduced-only also runs on a tree without the feature (the parent commit's, for the A/B of the
           untouched path).
  reduce   a 514-bit FheUint mod n through the folds and through the general `%`, alternated; wall clock to the
           final wait; bootstraps, launch levels and level sizes of each from the context's counters.
  counts   the dry schedules (no GPU): the reduction alone, and the signer's FHE block with and without it.

Each step runs in a fresh child process under its own time limit; the tool stops at the first step that fails or
runs out of time.  A record, not a pass / fail condition.

    python tools/sign_reduced_timing.py [--reps 10] [--warmup 2] [--steps sign,reduce,counts] [--unreduced-only] [--out FILE]
"""
import argparse
import csv
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fhe-sign_amd"))

LIMITS = {"sign": 240, "reduce": 180, "counts": 120}  # seconds per step
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
NC = 2**256 - N


def med(xs):
    xs = sorted(xs)
    return f"median {1e3 * statistics.median(xs):8.2f} ms   min {1e3 * xs[0]:8.2f}   max {1e3 * xs[-1]:8.2f}"


def words(x, n):
    return (C.c_uint64 * n)(*[(x >> (64 * i)) & (2**64 - 1) for i in range(n)])


def gpu_env():
    from fhe_sign import Context, generate_keys, set_server_key
    ck, sk = generate_keys(seed=0x51D)
    ctx = Context(0)
    ctx.set_server_key(sk)
    set_server_key(ctx)
    return ck, ctx


def step_sign(a):
    from fhe_sign import COMPAT, FAST, PUBLIC, BigUintFHE, Schnorr, compute_nonce, set_server_key
    ck, ctx = gpu_env()
    rows = {r["index"]: r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))}
    s = Schnorr()
    print(f"sign_fhe_with_k0, wall clock of the call, {a.reps} alternating runs after {a.warmup} warm-ups "
          "(vector 0: a one-limb private key; vector 1: eight limbs, the 8 x 8 limb block):")
    for idx in ("0", "1"):
        row = rows[idx]
        d = int(row["secret key"], 16)
        msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
        k0 = compute_nonce(d, msg, aux)
        d_fhe = BigUintFHE.new(d, ck)
        want = bytes.fromhex(row["signature"])
        for name, mode in (("compat", COMPAT), ("fast", FAST), ("public", PUBLIC)):
            kinds = [("unreduced", {})] + ([] if a.unreduced_only else [("reduce=True", {"reduce": True})])
            t = {k: [] for k, _ in kinds}
            for i in range(a.warmup + a.reps):
                for kind, kw in kinds:
                    ctx.sync()
                    t0 = time.perf_counter()
                    sig = s.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, mode, **kw)
                    dt = time.perf_counter() - t0
                    assert sig == want, (idx, name, kind)
                    if i >= a.warmup:
                        t[kind].append(dt)
            for kind, _ in kinds:
                print(f"  vector {idx} {name:7s} {kind:12s} {med(t[kind])}")
        del d_fhe
    set_server_key(None)
    ctx.close()


def step_reduce(a):
    import random

    from fhe_sign import FheUint, level_log, set_server_key, stats
    ck, ctx = gpu_env()
    v = random.Random(514).getrandbits(514)
    x = FheUint.try_encrypt(v, ck, bits=514)
    cases = {"folds (rem_pseudo_mersenne)": lambda: x.rem_pseudo_mersenne(256, NC), "general %": lambda: x % N}
    t = {k: [] for k in cases}
    shape = {}
    for i in range(a.warmup + a.reps):
        for name, fn in cases.items():
            ctx.sync()
            level_log(ctx)
            s0 = stats(ctx)
            t0 = time.perf_counter()
            r = fn()
            ctx.sync()
            dt = time.perf_counter() - t0
            s1 = stats(ctx)
            shape[name] = (s1[0] - s0[0], s1[1] - s0[1], level_log(ctx))
            if i == 0:
                assert r.decrypt(ck) == v % N, name
            if i >= a.warmup:
                t[name].append(dt)
            del r
    print(f"a 514-bit FheUint mod n = 2^256 - c (secp256k1's order), wall clock to the final wait, {a.reps} alternating runs "
          f"after {a.warmup} warm-ups:")
    for name in cases:
        p, lev, sizes = shape[name]
        print(f"  {name:28s} {med(t[name])}   {p} bootstraps, {lev} levels")
        print(f"      level sizes: {sizes}")
    del x
    set_server_key(None)
    ctx.close()


def step_counts(a):
    from fhe_sign import _lib
    lib = _lib.load()
    cw = words(NC, 3)
    print("dry schedules (engine host mode, nothing launched): bootstraps / launch levels / folds, level sizes")
    for bits in (512, 514):
        p, lev, f = C.c_uint64(), C.c_uint64(), C.c_uint32()
        sizes = (C.c_uint32 * 1024)()
        assert lib.fhe_host_rem_pseudo_mersenne_stats(bits, 256, cw, 3, C.byref(p), C.byref(lev), sizes, 1024, C.byref(f),
                                                      None) == 0
        print(f"  reduction alone, {bits} -> 256 bits: {p.value} / {lev.value} / {f.value}   {list(sizes[:lev.value])}")
    ones = (C.c_uint32 * 8)(*([1] * 8))
    for name, mode in (("compat", 0), ("fast", 1)):
        p, lev = C.c_uint64(), C.c_uint64()
        assert lib.fhe_host_biguint_mul_stats(8, 8, 8, mode | 0x100, C.byref(p), C.byref(lev), None, 0) == 0
        f = C.c_uint32()
        q, lv = C.c_uint64(), C.c_uint64()
        sizes = (C.c_uint32 * 1024)()
        assert lib.fhe_host_biguint_mul_add_rem(0, ones, 8, ones, 8, ones, 8, mode, 256, cw, 3, None, 0, None, 0, None,
                                                C.byref(q), C.byref(lv), sizes, 1024, C.byref(f), None) == 0
        print(f"  signer block 8 x 8 + 8 limbs, {name}: unreduced {p.value} / {lev.value}, reduced {q.value} / {lv.value} / "
              f"{f.value}   {list(sizes[:lv.value])}")
    # public operands: the graph depends on the clear digits, so real ones (vector 1's e and k) on simulated d
    from fhe_sign import Schnorr, compute_nonce
    row = next(r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv"))) if r["index"] == "1")
    d = int(row["secret key"], 16)
    msg = bytes.fromhex(row["message"])
    k, e, _ = Schnorr().sign_prologue(msg, compute_nonce(d, msg, bytes.fromhex(row["aux_rand"])), d)
    lim = lambda v: (C.c_uint32 * 8)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)])  # noqa: E731
    for name, mode in (("reduced as it is formed", 2), ("multiply, then fold", 2 | 0x800)):
        out = (C.c_uint64 * 4)()
        f, q, lv = C.c_uint32(), C.c_uint64(), C.c_uint64()
        assert lib.fhe_host_biguint_mul_add_rem(1, lim(e), 8, lim(d), 8, lim(k), 8, mode, 256, cw, 3, out, 4, None, 0, None,
                                                C.byref(q), C.byref(lv), None, 0, C.byref(f), None) == 0
        assert sum(out[i] << (64 * i) for i in range(4)) == (k + e * d) % N
        print(f"  public operands, {name}: {q.value} / {lv.value} / {f.value}")


STEPS = {"sign": step_sign, "reduce": step_reduce, "counts": step_counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", default="sign,reduce,counts")
    ap.add_argument("--unreduced-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # child mode: run one step in this process
    a = ap.parse_args()
    if a.step:
        STEPS[a.step](a)
        return 0
    steps = [s for s in a.steps.split(",") if s]
    if a.unreduced_only:
        steps = [s for s in steps if s == "sign"]
    text = []
    for name in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps), "--warmup", str(a.warmup)]
        if a.unreduced_only:
            cmd.append("--unreduced-only")
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {LIMITS[name]} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        text.append(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            print(f"step {name}: exit status {p.returncode}; stopping", file=sys.stderr)
            return p.returncode if p.returncode > 0 else 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
