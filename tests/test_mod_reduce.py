"""x mod (2^k - c) under encryption (radix_rem_pseudo_mersenne, csrc/radix.cpp) on the CPU: the engine's
simulated runs (every encrypted code path, each bootstrap evaluated from its lookup table and range-checked)
against Python's %, and its dry runs for the fold counts, the schedule and the recording order.  No GPU, no key.

The fold count is public: B <- (2^k - 1) + (B >> k) c from B = 2^width - 1 while B >= 2 n, so 3 folds for
secp256k1's n from 512 or 514 bits, 2 for its p, none for an operand no wider than k."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import pytest

import ref_semantics as R
from conftest import ROOT
from fhe_sign import COMPAT, FAST, PUBLIC, SECP256K1_N_C, SECP256K1_P_C, Schnorr, _lib, compute_nonce
from fhe_sign.schnorr import CURVE_ORDER

N, NC, PC = CURVE_ORDER, SECP256K1_N_C, SECP256K1_P_C
P = 2**256 - PC
M64 = 2**64 - 1
MUL_THEN_FOLD = 0x800  # FHE_HOST_MUL_THEN_FOLD
ROWS = {r["index"]: r for r in __import__("csv").DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))}


def _words(x, n):
    return (C.c_uint64 * max(1, n))(*[(x >> (64 * i)) & M64 for i in range(n)])


def _cwords(c):
    n = max(1, (c.bit_length() + 63) // 64)
    return _words(c, n), n


def sim_rem(bits, x, k, c, check=True):
    """(result, bootstraps, levels, folds) of the simulated reduction, or (rc, message) with check=False"""
    lib = _lib.load()
    cw, nc = _cwords(c)
    no = (k + 63) // 64
    out = (C.c_uint64 * max(1, no))()
    p, lev, f = C.c_uint64(), C.c_uint64(), C.c_uint32()
    rc = lib.fhe_host_sim_rem_pseudo_mersenne(bits, _words(x, (bits + 63) // 64), k, cw, nc, out, no, C.byref(p),
                                              C.byref(lev), C.byref(f))
    if not check:
        return rc, (lib.fhe_last_error() or b"").decode()
    assert rc == 0, lib.fhe_last_error()
    return sum(out[i] << (64 * i) for i in range(no)), p.value, lev.value, f.value


def dry_rem(bits, k, c):
    lib = _lib.load()
    cw, nc = _cwords(c)
    p, lev, f, fp = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    sizes = (C.c_uint32 * 1024)()
    rc = lib.fhe_host_rem_pseudo_mersenne_stats(bits, k, cw, nc, C.byref(p), C.byref(lev), sizes, 1024, C.byref(f),
                                                C.byref(fp))
    assert rc == 0, lib.fhe_last_error()
    return {"pbs": p.value, "levels": lev.value, "folds": f.value, "fingerprint": fp.value,
            "sizes": list(sizes[:min(lev.value, 1024)])}


def fold_model(x, bits, k, c):
    """the algorithm on plain integers: (T before the conditional subtraction, folds)"""
    n, B, f = 2**k - c, 2**bits - 1, 0
    while B >= 2 * n:
        x = (x & (2**k - 1)) + (x >> k) * c
        B = (2**k - 1) + (B >> k) * c
        f += 1
    assert x <= B < 2 * n
    return x, f


# ------------------------------------------------------------------ the smallest shapes, exhaustively
@pytest.mark.parametrize("c", [3, 15])
def test_exhaustive_12_bits_k6(c):
    """n = 61 and n = 49 (c = 15 is the largest c < 2^(k-2) = 16): all 4096 inputs"""
    n = 64 - c
    for x in range(4096):
        got = sim_rem(12, x, 6, c)[0]
        assert got == x % n, (x, got)


def test_k8_c3_named_and_random():
    k, c, bits = 8, 3, 16
    n = 2**k - c
    rng = random.Random(0x8C3)
    cases = [0, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2**k - 1, 2**k, 2**k + c - 1, 2**16 - 1]
    for _ in range(8):
        q = rng.randrange(1, 2**16 // n + 1)
        cases += [q * n - 1, min(q * n, 2**16 - 1)]
    cases += [rng.getrandbits(16) for _ in range(200)]
    for x in cases:
        assert sim_rem(bits, x, k, c)[0] == x % n, x


# ------------------------------------------------------------------ secp256k1's moduli
def _unfold(T, c, folds, bits):
    """an input whose folds end at T, built backwards: x = low + 2^256 h with low + c h the next value; the last
    fold's high part is 1, the earlier ones the smallest that leave low below 2^256 (low then sits just under it)"""
    x = T
    for i in range(folds):
        h = 1 if i == 0 else (x - 2**256) // c + 1
        low = x - c * h
        assert 0 <= low < 2**256
        x = low + (h << 256)
    assert x < 2**bits
    return x


@pytest.mark.parametrize("c", [NC, PC], ids=["n", "p"])
@pytest.mark.parametrize("bits", [512, 514])
def test_secp256k1_moduli(bits, c):
    n = 2**256 - c
    folds = 3 if c == NC else 2
    rng = random.Random(bits + (c & 0xFFFF))
    cases = [0, n - 1, n, 2 * n - 1, 2**256 - 1, 2**256, 2**512 - 1, 2**bits - 1, (n - 1)**2 + (n - 1)]
    cases += [rng.getrandbits(bits) for _ in range(5)]
    for x in cases:
        got, _, _, f = sim_rem(bits, x, 256, c)
        assert got == x % n, hex(x)
        assert f == folds
    # the value before the conditional subtraction on both sides of 2^256, and at the interval ends
    for T, lo, hi in [(n, n, 2**256), (n + rng.randrange(c), n, 2**256), (2**256 - 1, n, 2**256),
                      (2**256, 2**256, 2 * n), (2**256 + (c >> 1), 2**256, 2 * n), (2**256 + c - 1, 2**256, 2 * n)]:
        x = _unfold(T, c, folds, bits)
        t_model, f_model = fold_model(x, bits, 256, c)
        assert f_model == folds and lo <= t_model < hi and t_model == T
        assert sim_rem(bits, x, 256, c)[0] == x % n == T - n


@pytest.mark.parametrize("bits,k,c", [(256, 256, NC), (200, 256, NC), (8, 8, 3), (6, 8, 3), (256, 256, PC)])
def test_operand_no_wider_than_k_takes_no_fold(bits, k, c):
    n = 2**k - c
    rng = random.Random(bits * k)
    for x in [0, 1, 2**bits - 1, min(n - 1, 2**bits - 1), min(n, 2**bits - 1)] + [rng.getrandbits(bits) for _ in range(6)]:
        got, _, _, f = sim_rem(bits, x, k, c)
        assert (got, f) == (x % n, 0)
    assert dry_rem(bits, k, c)["folds"] == 0


def test_preconditions_are_refused():
    for bits, k, c, what in [(12, 7, 3, "k must be even"), (12, 6, 0, "c must be positive"),
                             (12, 6, 16, "below 2^(k - 2)"), (12, 6, 2**64, "below 2^(k - 2)"),
                             (12, 2, 1, "below 2^(k - 2)"), (12, 0, 1, "k must be even"),
                             (4098, 6, 3, "width"), (13, 6, 3, "width"), (12, 4096, 3, "k must be even")]:
        rc, msg = sim_rem(bits, 5, k, c, check=False)
        assert rc == -1 and what in msg, (bits, k, c, msg)
    assert sim_rem(12, 5, 6, 15)[0] == 5  # the largest c still in


def test_fold_counts_and_schedule_from_the_dry_run():
    d514, p514, d256 = dry_rem(514, 256, NC), dry_rem(514, 256, PC), dry_rem(256, 256, NC)
    assert (d514["folds"], p514["folds"], d256["folds"]) == (3, 2, 0)
    assert dry_rem(512, 256, NC)["folds"] == 3 and dry_rem(4096, 256, NC)["folds"] == 31
    for d in (d514, p514, d256):
        assert sum(d["sizes"]) == d["pbs"] and len(d["sizes"]) == d["levels"]
    assert d256["pbs"] < p514["pbs"] < d514["pbs"] and d256["levels"] < p514["levels"] < d514["levels"]
    # the dry schedule is the simulated run's
    assert sim_rem(514, 12345, 256, NC)[1:] == (d514["pbs"], d514["levels"], 3)


# ------------------------------------------------------------------ the signer's block
def _limbs(x, n):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def block(sim, a, b, k, mode, la=8, lb=8, lk=8):
    """fhe_host_biguint_mul_add_rem on la / lb / lk limbs, mod n"""
    lib = _lib.load()
    A, B, K = ((C.c_uint32 * max(1, n))(*_limbs(v, n)) for v, n in ((a, la), (b, lb), (k, lk)))
    cw, nc = _cwords(NC)
    out, cols = (C.c_uint64 * 4)(), (C.c_uint64 * 32)()
    cb, p, lev, f, fp = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    rc = lib.fhe_host_biguint_mul_add_rem(sim, A, la, B, lb, K, lk, mode, 256, cw, nc, out, 4, cols, 32, C.byref(cb),
                                          C.byref(p), C.byref(lev), None, 0, C.byref(f), C.byref(fp))
    assert rc == 0, lib.fhe_last_error()
    return {"out": sum(out[i] << (64 * i) for i in range(4)), "cols": sum(cols[i] << (64 * i) for i in range(32)),
            "col_bits": cb.value, "pbs": p.value, "levels": lev.value, "folds": f.value, "fingerprint": fp.value}


def _vector_operands(idx):
    row = ROWS[idx]
    d = int(row["secret key"], 16) % N
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    k, e, _ = Schnorr().sign_prologue(msg, k0, d)
    return e, d, k, Schnorr().sign_with_k0(msg, k0, d)


def _sim_columns(a, b, k, mode, la, lb, lk):
    """the existing column sim: the value the unreduced signer decrypts"""
    lib = _lib.load()
    A, B, K = ((C.c_uint32 * max(1, n))(*_limbs(v, n)) for v, n in ((a, la), (b, lb), (k, lk)))
    words, bits = (C.c_uint64 * 32)(), C.c_uint32()
    rc = lib.fhe_host_sim_biguint_mul_add_columns(A, la, B, lb, K, lk, mode, words, 32, C.byref(bits), None, None)
    assert rc == 0, lib.fhe_last_error()
    return sum(words[i] << (64 * i) for i in range(32)), bits.value


@pytest.mark.parametrize("mode", [COMPAT, FAST])
def test_column_form_then_reduction(mode):
    """k + a * b in the signer's column form, then the reduction reading those columns unpropagated: the result
    is (the value of the columns) mod n -- in compat mode the limbs the existing column sim returns, lost carries
    included, so the reduced signer gives the reference's bytes, not the true product's."""
    ones = 2**256 - 1
    cases = []
    for idx in ("0", "1"):
        e, d, k, sig = _vector_operands(idx)
        cases.append((e, d, k, len(R.to_u32_digits(e)), len(R.to_u32_digits(d)), len(R.to_u32_digits(k)), sig))
    cases.append((ones, ones, ones, 8, 8, 8, None))
    rng = random.Random(77 + mode)
    cases.append((rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256), 8, 8, 8, None))
    lost = 0
    for a, b, k, la, lb, lk, sig in cases:
        r = block(1, a, b, k, mode, la, lb, lk)
        want, bits = _sim_columns(a, b, k, mode, la, lb, lk)
        assert (r["cols"], r["col_bits"]) == (want, bits)
        assert r["out"] == want % N < N
        if mode == FAST:
            assert want == k + a * b
        lost += want != k + a * b
        if sig is not None:  # a BIP-340 vector: the reduced value is the signature's s
            assert r["out"] == int.from_bytes(sig[32:], "big")
        if (la, lb, lk) == (8, 8, 8):
            assert r["folds"] == 3
    if mode == COMPAT:
        assert lost >= 1  # the all-ones limbs lose a carry in the reference's loop: the case above is not vacuous


def test_public_operand_variants():
    """(k + e d) mod n with clear e, k: the product reduced as it is formed (what eval_s_public records) against
    multiply-then-fold on the unreduced public signer's columns -- same values, and the former cheaper in
    bootstraps, levels and folds on every case (why it is the one the signer uses)"""
    rng = random.Random(0x9B)
    cases = [_vector_operands("1")[:3], (N - 1, 2**256 - 1, N - 1), (1, 2**256 - 1, 0), (0, 5, 7),
             tuple(rng.randrange(N) for _ in range(3))]
    for e, d, k in cases:
        a, b = block(1, e, d, k, PUBLIC), block(1, e, d, k, PUBLIC | MUL_THEN_FOLD)
        assert a["out"] == b["out"] == (k + e * d) % N
        assert b["cols"] == k + e * d and b["col_bits"] == 514
        if e.bit_length() > 200:
            assert a["pbs"] < b["pbs"] and a["levels"] < b["levels"] and a["folds"] <= 1 < b["folds"] == 3
    # the clear operands must be reduced already
    lib = _lib.load()
    cw, nc = _cwords(NC)
    big = (C.c_uint32 * 8)(*_limbs(N, 8))
    one = (C.c_uint32 * 8)(*_limbs(1, 8))
    out = (C.c_uint64 * 4)()
    assert lib.fhe_host_biguint_mul_add_rem(1, big, 8, one, 8, one, 8, PUBLIC, 256, cw, nc, out, 4, None, 0, None, None,
                                            None, None, 0, None, None) == -1
    assert b"below the modulus" in lib.fhe_last_error()


# ------------------------------------------------------------------ recording order
_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
import test_mod_reduce as t
e, d, k = (int(x, 16) for x in sys.argv[1:4])
print(json.dumps([t.dry_rem(514, 256, t.NC)["fingerprint"], t.dry_rem(512, 256, t.PC)["fingerprint"],
                  t.block(0, 1, 1, 1, t.COMPAT)["fingerprint"], t.block(0, 1, 1, 1, t.FAST)["fingerprint"],
                  t.block(0, e, d, k, t.PUBLIC)["fingerprint"]]))
"""


def test_recording_order_is_equal_across_processes():
    """the fan-out scatters the gathered slices by each rank's own recording order: the dry runs' fingerprints
    (a hash of every scheduled node in order, no addresses) are equal in two fresh processes"""
    e, d, k = _vector_operands("1")[:3]
    paths = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "fhe-sign_amd"), os.path.join(ROOT, "oracle")]
    code = _CHILD.format(paths=paths)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="")  # nothing here makes a GPU call
    outs = [subprocess.run([sys.executable, "-c", code, hex(e), hex(d), hex(k)], capture_output=True, text=True,
                           timeout=120, env=env) for _ in range(2)]
    for p in outs:
        assert p.returncode == 0, p.stderr
    a, b = (json.loads(p.stdout.strip().splitlines()[-1]) for p in outs)
    assert a == b and len(set(a)) == len(a)
    assert a[0] == dry_rem(514, 256, NC)["fingerprint"]


# ------------------------------------------------------------------ no GPU, no quiet fall-back
def test_reduced_signer_without_a_context_errors_loudly():
    from fhe_sign import set_server_key
    set_server_key(None)
    s = Schnorr()
    with pytest.raises(RuntimeError, match="no server key set"):
        s.sign_fhe_with_k0(bytes(32), 5, 3, None, None, COMPAT, reduce=True)
    with pytest.raises(RuntimeError, match="no server key set"):
        s.sign_fhe(bytes(32), bytes(32), 3, None, reduce=True)
    with pytest.raises(RuntimeError, match="no server key set"):
        s.sign_fhe_with_k0_batch([], None, COMPAT, reduce=True)
    with pytest.raises(RuntimeError, match="no server key set"):
        s.eval_s(1, 2, None, PUBLIC)
    # the C entry points themselves: a null context is an error with a message, never a CPU result
    lib = _lib.load()
    sig, h = (C.c_uint8 * 64)(), C.c_void_p()
    b32 = (C.c_uint8 * 32)()
    cw, nc = _cwords(NC)
    assert lib.fhe_schnorr_sign_fhe_with_k0_reduced(None, None, None, 0, b32, b32, None, COMPAT, sig) == -1
    assert lib.fhe_schnorr_sign_fhe_with_k0_rerand_reduced(None, None, None, 0, b32, b32, None, COMPAT, None, 0, sig) == -1
    assert lib.fhe_schnorr_eval_s(None, None, None, None, COMPAT, C.byref(h)) == -1
    assert lib.fhe_schnorr_eval_s_public(None, b32, b32, None, C.byref(h)) == -1
    assert lib.fhe_radix_rem_pseudo_mersenne(None, None, 256, cw, nc, C.byref(h)) == -1
    assert b"null context" in lib.fhe_last_error()
    assert lib.fhe_columns_rem_pseudo_mersenne(None, None, 256, cw, nc, C.byref(h)) == -1
    assert not h.value and bytes(sig) == bytes(64)
