"""The threading contract (include/fhe_rocm.h, "Threading") on the GPU: device contexts on concurrent host threads,
one thread per context, each with its own keys at LWE dimension 16 (classic and multi-bit, as
tests/test_handle_owner_gpu.py).

What is pinned is results, in one pass: a thread's program -- the encrypted shift first, as the first op of a fresh
context -- runs sequentially on the main thread (module fixture, once), its contexts are closed, and fresh contexts
under the same key seeds and encryption seeds run it again on two and on four threads behind a barrier.  Every
exported block must equal the sequential pass's 64-bit words, the digest and the modulus-switched list its bytes,
every decrypted value the Python integer.  Beside the radix path the raw one: ctx.pbs on the latency and the
throughput kernel against the oracle's words while another thread runs the radix program.  And a context that
moves: made on the main thread, used by a worker, read by the main thread again.

No repetition to make a race show: tools/tsan_host.sh (CPU, simulated contexts) is the race detector.  One process,
at most four contexts; a worker that is not back within max(60 s, 10 x the sequential pass) fails the test, and the
test then starts nothing further on the GPU (its contexts are left as they are)."""
import threading
import time

import numpy as np
import pytest
import torch

import oracle
from fhe_sign import Context, FheUint, generate_keys, set_server_key
from lwe_dims import CLASSIC, MULTIBIT, oracle_params, product_params
from test_keyswitch_gpu import _assert_words
from test_lwe_dims_gpu import _pbs_case

pytestmark = pytest.mark.gpu
SEED = 0x7EAD5
# (grouping, key seed, encryption seed, operand seed): two classic, two multi-bit; all seeds differ
SPECS = [(CLASSIC, SEED, 11, 1), (MULTIBIT, SEED + 1, 12, 2), (CLASSIC, SEED + 2, 13, 3), (MULTIBIT, SEED + 3, 14, 4)]


class Hung(Exception):
    pass


class Side:
    """a device context with its own keys; the client key's encryption stream is seeded: two Sides of one spec
    encrypt the same words"""

    def __init__(self, spec, device=0):
        self.spec = spec
        grouping, key_seed, enc_seed, _ = spec
        self.ck, self.sk = generate_keys(product_params(16, grouping), seed=key_seed)
        self.ck.seed_encryption(enc_seed)
        self.ctx = Context(device)
        self.ctx.set_server_key(self.sk)


def operands(spec, bits):
    rng = np.random.RandomState(spec[3] * 1000 + bits)
    x = (int(rng.randint(0, 1 << 31)) * 8 + 5) & ((1 << bits) - 1)
    y = (int(rng.randint(0, 1 << 31)) >> (31 - bits // 2)) | 1  # half the width: a quotient of several blocks
    return x, y, int(rng.randint(1, bits // 2))  # the shifted values keep several blocks


def program(side, decrypt=True):
    """On the calling thread, under side.ctx: at 16 and 34 bits X << S first, then (X + Y) * X, that >> S, that
    .min(Y); at 16 bits X // Y; then digest() and compress_switched().serialize() of the last value, export() of
    every result.  Returns the handles, the words, the bytes, the expected integers and (decrypt) the values."""
    set_server_key(side.ctx)
    try:
        got, want = [], []
        for bits in (16, 34):
            M = (1 << bits) - 1
            x, y, s = operands(side.spec, bits)
            X, Y, S = (FheUint.try_encrypt(v, side.ck, bits=bits) for v in (x, y, s))
            got.append(X << S), want.append((x << s) & M)
            got.append((X + Y) * X), want.append(((x + y) * x) & M)
            got.append(got[-1] >> S), want.append(want[-1] >> s)
            got.append(got[-1].min(Y)), want.append(min(want[-1], y))
            if bits == 16:
                got.append(X // Y), want.append(x // y)
        last = got[-1]
        out = {"handles": got, "want": want, "digest": last.digest(), "switched": last.compress_switched().serialize(),
               "words": [g.export() for g in got]}
        if decrypt:
            out["values"] = [g.decrypt(side.ck) for g in got]
        return out
    finally:
        set_server_key(None)


def run_threads(targets, limit):
    """one daemon thread per target; an exception in a worker is carried here and raised again; Hung if a worker is
    not back within the limit"""
    errors = [None] * len(targets)

    def guarded(i, fn):
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 - carried to the main thread
            errors[i] = e

    threads = [threading.Thread(target=guarded, args=(i, fn), daemon=True) for i, fn in enumerate(targets)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + limit
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        raise Hung(f"a worker is not back after {limit:.0f} s")
    for e in errors:
        if e is not None:
            raise e


def close_all(sides):
    set_server_key(None)
    for s in sides:
        s.ctx.close()


@pytest.fixture(scope="module")
def sequential():
    """the reference pass, once for the module: every spec's program on the main thread on a context of its own,
    closed before the next; spec -> (result without its handles, wall seconds)"""
    ref = {}
    for spec in SPECS:
        t0 = time.perf_counter()
        side = Side(spec)
        try:
            out = program(side)
            del out["handles"]
        finally:
            close_all([side])
        ref[spec] = (out, time.perf_counter() - t0)
        assert out["values"] == out["want"], spec  # the reference itself computes the integers
    return ref


def limit_for(sequential, specs):
    return max(60.0, 10.0 * sum(sequential[s][1] for s in specs))


def assert_same(out, ref, what):
    assert len(out["words"]) == len(ref["words"]) == 9
    for k, (got, want) in enumerate(zip(out["words"], ref["words"])):
        assert got.dtype == want.dtype == np.uint64 and np.array_equal(got, want), f"{what}: result {k}: words differ"
    assert out["digest"] == ref["digest"], f"{what}: digest"
    assert out["switched"] == ref["switched"], f"{what}: switched list bytes"
    assert out["values"] == out["want"] == ref["want"], f"{what}: values"


def threaded_pass(sequential, specs):
    """fresh contexts under the specs' seeds, one thread each behind a barrier"""
    sides = [Side(s) for s in specs]
    barrier = threading.Barrier(len(sides))
    outs = [None] * len(sides)

    def worker(i):
        try:
            barrier.wait(60)
            outs[i] = program(sides[i])
        except BaseException:
            barrier.abort()  # a worker that fails before the barrier does not keep the others waiting
            raise

    try:
        run_threads([lambda i=i: worker(i) for i in range(len(sides))], limit_for(sequential, specs))
    except Hung as e:
        pytest.fail(str(e))  # nothing further on the GPU: the contexts are not closed
    try:
        for i, s in enumerate(specs):
            assert_same(outs[i], sequential[s][0], f"thread {i} (grouping {s[0]})")
        assert len({o["digest"] for o in outs}) == len(outs)  # different keys and operands: different values
    finally:
        outs.clear()
        close_all(sides)


def test_two_contexts_on_two_threads(sequential):
    """one classic, one multi-bit"""
    threaded_pass(sequential, SPECS[:2])


def test_four_contexts_on_four_threads(sequential):
    """two classic, two multi-bit"""
    threaded_pass(sequential, SPECS)


def test_raw_pbs_beside_the_radix_program(sequential):
    """one thread bootstraps batches of 8 (latency kernel) and 300 (throughput kernel) rows on a classic context,
    word for word against the oracle at n = 16; the other runs the radix program on a multi-bit context meanwhile"""
    spec = SPECS[1]
    ck, sk = generate_keys(product_params(16, CLASSIC), seed=SEED + 7)
    ok = oracle.OracleKeys(SEED + 7, oracle_params(16, CLASSIC))
    tables, cts, lut_of, ref, want = _pbs_case(ok, 37)
    raw = Context(0)
    raw.set_server_key(sk)
    side = Side(spec)
    ids = np.array([raw.lut(t) for t in tables], np.uint32)
    barrier = threading.Barrier(2)
    got = {}

    def pbs_worker():
        try:
            barrier.wait(60)
            for b in (8, 300):
                got[b] = raw.pbs(np.resize(cts, (b, 2049)), ids[np.resize(lut_of, b)])
        except BaseException:
            barrier.abort()
            raise

    def radix_worker():
        try:
            barrier.wait(60)
            got["radix"] = program(side)
        except BaseException:
            barrier.abort()
            raise

    try:
        run_threads([pbs_worker, radix_worker], limit_for(sequential, [spec]))
    except Hung as e:
        pytest.fail(str(e))
    try:
        for b in (8, 300):
            _assert_words(got[b], np.resize(ref, (b, 2049)), f"batch of {b} beside the radix program")
            assert [ok.decrypt(o) for o in got[b]] == [want[i % len(want)] for i in range(b)]
        assert_same(got["radix"], sequential[spec][0], "radix program beside the raw bootstraps")
    finally:
        got.clear()
        raw.close()
        close_all([side])


def moved_context(sequential, device):
    """made with its key on the main thread, used by a worker while the main thread waits, read by the main thread"""
    spec = SPECS[0]
    side = Side(spec, device)
    outs = []

    def worker():
        if device:
            torch.cuda.set_device(0)  # the worker's current device is not the context's
        outs.append(program(side, decrypt=False))

    try:
        run_threads([worker], limit_for(sequential, [spec]))
    except Hung as e:
        pytest.fail(str(e))
    try:
        out = outs.pop()
        set_server_key(side.ctx)
        out["values"] = [g.decrypt(side.ck) for g in out["handles"]]
        assert_same(out, sequential[spec][0], f"context on device {device}, used by a worker")
        # the main thread goes on with the worker's values
        h = out["handles"]
        assert (h[0] + h[3]).decrypt(side.ck) == (out["want"][0] + out["want"][3]) & 0xFFFF
    finally:
        outs.clear()
        out = h = None
        close_all([side])


def test_context_moves_between_threads(sequential):
    moved_context(sequential, 0)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_context_on_device_1_used_from_a_thread_on_device_0(sequential):
    """every entry point sets the context's device itself"""
    moved_context(sequential, 1)
