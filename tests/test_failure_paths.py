"""What a failed call leaves behind, on the CPU (include/fhe_rocm.h, "Errors after validation"): programs run on a
simulated context with the host-side fault point armed (FHE_TUNE_FAULT_SITES / FHE_TUNE_FAULT_AFTER), so that one
call of the program fails after its arguments were accepted -- inside a flush, a partial flush (flush_for, the
batch tail) or a recording -- with FHE_ERR_HIP, "injected fault at <site>".  That same call is repeated and the
program runs to its end.

Per program: one clean run with every site enabled and k = 0 reads the crossing count C; then one run per chosen k
(every k when C <= 48, else the first 16, the last 16 and 16 evenly spaced).  The programs are
tests/test_launch_replay.py's and tests/test_sim_context.py's.

After each failed-and-retried run:
  - exactly one call failed, with FHE_ERR_HIP and "injected";
  - every decrypted value equals the Python big-integer reference;
  - fhe_ctx_pending_info shows nothing pending, armed or in flight after the final flush;
  - the launch trace covers the failed attempt and the retry: it parses and holds structurally
    (tests/launch_replay.py, which also holds it to fhe_ctx_level_log and the fhe_ctx_stats delta), and its
    plaintext replay gives, for every block of every value the program read, the reference digit.  The simulated
    context's shadow is right when a bootstrap is RECORDED, so a decryption alone cannot see a bootstrap that was
    marked written without being launched; the replay can: such a block has no NODE record;
  - the counters follow the rule "what is launched counts; a level launched twice counts twice; the level at which
    a flush failed was not launched and does not count": with the failure in a READ (a decryption: the failed call
    recorded nothing), the bootstraps, levels and level log of the run minus the clean run's are exactly the
    relaunched levels of the trace -- levels whose destinations an earlier level already wrote.  With the failure
    inside an OP (a recording, or the flush of a slice of FHE_TUNE_FLUSH_DEPTH levels), the op's own bootstraps
    are recorded again by the repeated call and the first recording is dropped as dead, launched or not: there
    the excess is at least the relaunched bootstraps and at most those plus what the run launched before the
    failure.

The mutation check takes the BigUintFHE call-site program's trace and removes the NODE records of the held
product's blocks, which is what the partial flush did before it put the set-aside nodes back (they were marked
written and dropped): the same assertions must then fail.  tools/faults_host_check.c runs the sweep through the C
ABI alone; its plain build runs here, its sanitized build by tools/asan_faults_host.sh."""
import ctypes as C
import gc
import os
import random
import subprocess
from collections import Counter

import pytest

import launch_replay as LR
import ref_semantics as R
import test_sim_context as TS
from conftest import ROOT
from fhe_sign import (COMPAT, FAST, FAULT_ALL, SECP256K1_N_C, FheUint, SimContext, SimKey, _lib, fault_arm,
                      pending_info, set_server_key, stats, tuning)
from test_launch_replay import Program, _limbs

FHE_ERR_HIP = -2
READS = ("fhe_radix_decrypt", "fhe_biguint_decrypt", "fhe_columns_decrypt", "fhe_radix_decrypt_bool", "fhe_ctx_sync")


@pytest.fixture(scope="module")
def sim():
    ctx = SimContext()
    set_server_key(ctx)
    yield ctx, SimKey()
    set_server_key(None)
    fault_arm(0)
    ctx.close()


class Retrying:
    """the loaded library with every status-returning entry point wrapped: a call that fails with the injected
    fault is noted and made again, with the same arguments"""

    def __init__(self, lib):
        self._lib, self.failures = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if fn.restype is not C.c_int or name == "fhe_host_set_tuning":
            return fn

        def call(*args):
            rc = fn(*args)
            if rc != 0 and b"injected fault" in (self._lib.fhe_last_error() or b""):
                self.failures.append((name, rc, self._lib.fhe_last_error().decode()))
                rc = fn(*args)
            return rc

        return call


def sweep_points(count):
    if count <= 48:
        return list(range(1, count + 1))
    mid = [16 + (i * (count - 32)) // 16 + 1 for i in range(16)]
    return sorted(set(list(range(1, 17)) + mid + list(range(count - 15, count + 1))))


class Run:
    """one run of a program under the recorder with the fault armed at crossing k (0: count only)"""

    def __init__(self, sim, program, k, monkeypatch):
        ctx, ck = sim
        rec = LR.Recorder(ctx)
        self.P = P = Program(rec, ck)
        levels0 = stats(ctx)[1]
        proxy = Retrying(_lib.load())
        fault_arm(FAULT_ALL, k)
        monkeypatch.setattr(_lib, "_lib", proxy)
        try:
            program(P, monkeypatch)
            gc.collect()
            # the final flush: every handle of the program is gone, what they left pending is swept as dead
            P.read(P.enc(1, 4) + P.enc(2, 4), 3, "final flush")
        finally:
            monkeypatch.undo()
            self.crossings = fault_arm(0)
            rec.close()
        self.failures = proxy.failures
        self.pending = pending_info(ctx)
        self.levels = stats(ctx)[1] - levels0
        # parses, holds structurally and to the level log and the bootstrap count; values and replayed digits
        self.records, self.tables, self.val = P.check()
        self.level_sizes = [len(r.nodes) for r in self.records if isinstance(r, LR.Level)]
        assert self.levels == len(self.level_sizes)

    def relaunched(self):
        """(sizes of the levels whose every destination an earlier level wrote, bootstraps launched again,
        levels that are partly new and partly relaunched)"""
        seen, whole, again, mixed = set(), [], 0, 0
        for r in self.records:
            if not isinstance(r, LR.Level):
                continue
            old = sum(n.dst in seen for n in r.nodes)
            again += old
            if old == len(r.nodes):
                whole.append(old)
            elif old:
                mixed += 1
            seen.update(n.dst for n in r.nodes)
        return whole, again, mixed


def sweep(sim, program, monkeypatch, want_read_failures=0):
    clean = Run(sim, program, 0, monkeypatch)
    assert clean.failures == [] and clean.pending == (0, 0, 0)
    assert clean.relaunched() == ([], 0, 0)
    count = clean.crossings
    assert count >= 2, "the program crossed no fault site"
    in_reads = 0
    runs = []
    for k in sweep_points(count):
        run = Run(sim, program, k, monkeypatch)
        what = (k, count, run.failures)
        assert len(run.failures) == 1, what
        name, rc, msg = run.failures[0]
        assert rc == FHE_ERR_HIP and "injected fault at " in msg, what
        assert run.pending == (0, 0, 0), what
        whole, again, mixed = run.relaunched()
        extra_pbs = sum(run.level_sizes) - sum(clean.level_sizes)
        if name in READS:
            in_reads += 1
            assert mixed == 0, what
            assert extra_pbs == again == sum(whole), what
            assert run.levels - clean.levels == len(whole), what
            assert Counter(run.level_sizes) - Counter(clean.level_sizes) == Counter(whole), what
            assert not Counter(clean.level_sizes) - Counter(run.level_sizes), what
        else:
            launched_before = sum(run.level_sizes)  # an upper bound that needs no position in the trace
            assert again <= extra_pbs <= again + launched_before, what
        run.records = run.val = run.P = None  # a run holds tens of thousands of records: only its summary is kept
        runs.append(run)
    assert in_reads >= want_read_failures, (in_reads, count)
    return clean, runs


# ---------------------------------------------------------------------------------------------- the programs
# test_sim_context.py's chain generator, shortened: a run is repeated 49 times here.  80 steps still meet every
# (op, kind) pair, which the generator asserts; at 18 and 34 bits, where a step costs thousands of bootstraps, fewer
# steps over fewer kinds of second operand (the aliased kinds are test_sim_context.py's subject, not this file's)
CHAIN_STEPS = {6: 80, 8: 80, 18: 40, 34: 30}
CHAIN_KINDS = {18: ("independent", "self"), 34: ("independent",)}


@pytest.mark.parametrize("bits,depth", [(6, 0), (8, 0), (8, 7), (18, 0), (34, 7)],
                         ids=["6-on-demand", "8-on-demand", "8-slices-of-7", "18-on-demand", "34-slices-of-7"])
def test_chains_with_a_failed_call(sim, monkeypatch, bits, depth):
    def program(P, mp):
        mp.setattr(TS, "enc", lambda v, _ck, b: P.enc(v, b))
        mp.setitem(TS.CHAIN_STEPS, bits, CHAIN_STEPS[bits])
        mp.setattr(TS, "KINDS", CHAIN_KINDS.get(bits, TS.KINDS))
        decrypt = FheUint.decrypt

        def noting(self, key):
            got = decrypt(self, key)
            P.results.append((P.rec.addrs(self), self.bits, got, got, ("chain", bits, len(P.results))))
            return got

        mp.setattr(FheUint, "decrypt", noting)
        with tuning(flush_depth=depth):
            TS.test_chains_through_the_abi(sim, bits)  # asserts every value against the Python integer itself

    sweep(sim, program, monkeypatch, want_read_failures=1)


@pytest.mark.parametrize("kara", [8, None], ids=["kara8", "default"])
@pytest.mark.parametrize("bits", [34, 66])
def test_products_with_a_failed_call(sim, monkeypatch, bits, kara):
    """mul (wrapping) and MUL_FULL (the 2 x bits product of operands cast up) with the Karatsuba split on and off"""
    rng = random.Random(0xFA17 * bits + (kara or 0))
    x, y = rng.getrandbits(bits) | 1 << (bits - 1), (1 << bits) - 1

    def program(P, mp):
        import contextlib
        with (tuning(kara_min=kara, kara_compat_min=kara) if kara else contextlib.nullcontext()):
            X, Y = P.enc(x, bits), P.enc(y, bits)
            P.read(X * Y, x * y % (1 << bits), ("mul", bits))
            P.read(TS.cast(X, 2 * bits) * TS.cast(Y, 2 * bits), x * y, ("mul_full", bits))

    sweep(sim, program, monkeypatch, want_read_failures=1)


@pytest.mark.parametrize("depth", [0, 7], ids=["on-demand", "slices-of-7"])
def test_encrypted_divrem_with_a_failed_call(sim, monkeypatch, depth):
    def program(P, mp):
        with tuning(flush_depth=depth):
            for x, y in ((0xE7, 0x0B), (0xFF, 0x00), (0x80, 0xFF)):
                q, r = P.enc(x, 8).div_rem(P.enc(y, 8))
                P.read(q, x // y if y else 0xFF, ("q", x, y))
                P.read(r, x % y if y else x, ("r", x, y))

    sweep(sim, program, monkeypatch, want_read_failures=1)


def _call_site(n, mode, seed=0):
    """p = a * b (held), t = p + k, decrypt(t) -- the partial flush: t's column form is launched, p's own carry
    propagation is set aside -- then decrypt(p)"""
    rng = random.Random(0xCA11 * n + mode + seed)
    al, bl, kl = TS.limb_values(n, rng)[1], _limbs(rng, n), _limbs(rng, n)
    pl = TS.mul_ref(al, bl, mode)
    tl = R.biguint_add(pl, kl)
    marks = {}

    def program(P, mp):
        a, b, k = P.big(al), P.big(bl), P.big(kl)
        p = a.mul(b, mode)
        t = p.add(k)
        marks["p"] = P.rec.addrs(p)[0]
        assert TS.same_limbs(t.decrypt_limbs(P.ck), tl, mode)
        assert TS.same_limbs(p.decrypt_limbs(P.ck), pl, mode)
        P.read_limbs(p, pl, mode, ("p", n, mode))
        P.read_limbs(t, tl, mode, ("t", n, mode))

    return program, marks


@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_biguint_call_site_with_a_failed_call(sim, monkeypatch, n, mode):
    program, _ = _call_site(n, mode)
    clean, runs = sweep(sim, program, monkeypatch, want_read_failures=1)
    # the partial flush itself failed in some of them: the first decryption, which launches a part of the graph
    assert any(r.failures[0][0] == "fhe_biguint_decrypt" for r in runs)


def test_rem_pseudo_mersenne_with_a_failed_call(sim, monkeypatch):
    m = (1 << 8) - 3

    def program(P, mp):
        for x in ((1 << 12) - 1, 0x9C5, m * 7 - 1):
            P.read(P.enc(x, 12).rem_pseudo_mersenne(8, 3), x % m, ("rem_pm", hex(x)))

    sweep(sim, program, monkeypatch, want_read_failures=1)


def test_signature_order_modulus_with_a_failed_call(sim, monkeypatch):
    """the signer's own reduction, once: 512 bits mod the curve order"""
    n = (1 << 256) - SECP256K1_N_C
    x = n * n - 1

    def program(P, mp):
        P.read(P.enc(x, 512).rem_pseudo_mersenne(256, SECP256K1_N_C), x % n, "rem_pm n")

    clean = Run(sim, program, 0, monkeypatch)
    for k in (1, clean.crossings // 2, clean.crossings - 1):
        run = Run(sim, program, k, monkeypatch)
        assert len(run.failures) == 1 and run.pending == (0, 0, 0), (k, run.failures)


# ---------------------------------------------------------------------------------------------- the mutation
def test_a_product_marked_written_without_its_launch_fails_the_replay(sim, monkeypatch):
    """Before the partial flush put its set-aside nodes back, a failure inside it dropped them marked as written:
    the held product then decrypted right on a simulated context (the shadow) and read unwritten slots on a
    device.  The same trace without the NODE records of the product's blocks: the replay finds no digit there."""
    program, marks = _call_site(2, COMPAT)
    clean = Run(sim, program, 0, monkeypatch)
    failed = None
    for k in sweep_points(clean.crossings):
        run = Run(sim, program, k, monkeypatch)
        if run.failures[0][0] == "fhe_biguint_decrypt" and "LEVEL" in run.failures[0][2]:
            failed = run
            break
    assert failed is not None
    mine = {a for a in marks["p"] if a}
    assert mine and all(a in {n.dst for n in LR.nodes_of(failed.records)} for a in mine)
    mutated = []
    for r in failed.records:
        if isinstance(r, LR.Level):
            r = LR.Level(r.number, r.split, [n for n in r.nodes if n.dst not in mine])
        mutated.append(r)
    mutated = LR.parse(LR.unparse(mutated))
    with pytest.raises(LR.ReplayError):
        # the reads of p's digits come after the records that are gone: either a later node reads an address the
        # replay does not know, or the result's block has no value
        inputs = LR.Inputs()
        val, _ = LR.replay_plain(mutated, failed.tables, _noted_again(failed))
        for (addrs, triv), bits, want, got, what in failed.P.results:
            assert LR.value_of(val, addrs, triv, bits) == want, what


def _noted_again(run):
    """the inputs of a finished run once more (a replay consumes them): the values the first replay took"""
    fresh = LR.Inputs()
    for r in run.records:
        if isinstance(r, LR.Write):
            for a in r.addrs:
                fresh.note([a], [run.val.get(a)])
    return fresh


# ---------------------------------------------------------------------------------------------- the hook itself
def test_fault_point_is_off_by_default_counts_and_fires_once(sim):
    ctx, ck = sim
    x = FheUint.try_encrypt(0x2B, ck, bits=8)
    assert fault_arm(0) >= 0
    assert (x * x).decrypt(ck) == 0x2B * 0x2B % 256
    assert fault_arm(0) == 0  # no site enabled: nothing is counted
    fault_arm(FAULT_ALL, 0)
    assert (x * x).decrypt(ck) == 0x2B * 0x2B % 256
    count = fault_arm(FAULT_ALL, 1)
    assert count >= 2
    from fhe_sign import FheError
    with pytest.raises(FheError, match="injected fault at RECORD") as e:
        x * x
    assert e.value.code == FHE_ERR_HIP
    assert (x * x).decrypt(ck) == 0x2B * 0x2B % 256  # disarmed by firing
    assert fault_arm(0) == count + 1  # the crossing that fired, and the clean run's
    assert pending_info(ctx)[1:] == (0, 0)


def test_pending_info_entry_point(sim):
    ctx, ck = sim
    lib = _lib.load()
    out = (C.c_uint64 * 3)()
    assert lib.fhe_ctx_pending_info(None, out) != 0
    assert lib.fhe_ctx_pending_info(ctx.handle, None) != 0
    x = FheUint.try_encrypt(0x2B, ck, bits=8)
    y = x * x
    assert pending_info(ctx)[0] > 0
    assert y.decrypt(ck) == 0x2B * 0x2B % 256
    del y
    assert (x + x).decrypt(ck) == 0x56
    assert pending_info(ctx) == (0, 0, 0)


# ---------------------------------------------------------------------------------------------- the C program
HIPCC = "/opt/rocm/bin/hipcc"


def test_faults_host_check(tmp_path):
    """tools/faults_host_check.c, plain build: the sweep through the C ABI alone (exit 1: a wrong value, or a
    missing or extra error)"""
    exe = tmp_path / "faults_host_check"
    lib = os.path.join(ROOT, "fhe-sign_amd", "lib")
    subprocess.run([HIPCC, "-x", "c", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "faults_host_check.c"), "-L", lib, "-lfhe_rocm", "-Wl,-rpath," + lib,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "faults host check: ok" in r.stdout
