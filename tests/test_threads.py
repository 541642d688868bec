"""The threading contract (include/fhe_rocm.h, "Threading") on the CPU: contexts are independent across host threads.

tools/threads_host_check.c -- four pthreads, a simulated context each, the first use of every radix algorithm behind a
barrier, then the same programs sequentially -- is built as a plain program (no sanitizer here; tools/tsan_host.sh is
the race detector) and run: status 0 and every threaded line equal to its sequential line.  The same through the
Python layer, whose set_server_key is thread-local: four threading.Threads with a SimContext and a SimKey each
(ctypes releases the GIL around every call, so the calls overlap), every result against Python integers; a thread
without a server key; fhe_last_error() per thread.  And a source check of what made the first encrypted shift on two
threads corrupt the heap: a function-local static that is filled after its declaration."""
import ctypes as C
import os
import random
import re
import subprocess
import threading

import pytest

from conftest import ROOT
from fhe_sign import FheError, FheUint, SimContext, SimKey, _lib, set_server_key
from test_kernel_resources import CSRC, HIPCC

T = 4
JOIN_LIMIT = 120  # seconds; the four chains together are a few seconds of CPU


def run_threads(targets, limit=JOIN_LIMIT):
    """one daemon thread per target (the targets bring their own barrier); an exception in a worker is carried
    here and raised again; a worker that is not back within the limit fails the test"""
    errors = [None] * len(targets)

    def guarded(i, fn):
        try:
            fn()
        except BaseException as e:  # noqa: BLE001 - carried to the main thread
            errors[i] = e

    threads = [threading.Thread(target=guarded, args=(i, fn), daemon=True) for i, fn in enumerate(targets)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(limit)
    assert not any(t.is_alive() for t in threads), f"a worker is not back after {limit} s"
    for e in errors:
        if e is not None:
            raise e


# ---------------------------------------------------------------- the stand-alone program
def test_threads_host_check(tmp_path):
    exe = tmp_path / "threads_host_check"
    lib = os.path.join(ROOT, "fhe-sign_amd", "lib")
    subprocess.run([HIPCC, "-x", "c", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "threads_host_check.c"), "-L", lib, "-lfhe_rocm", "-Wl,-rpath," + lib,
                    "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "threaded host check: ok"
    threaded = [ln.split(": ", 1) for ln in lines if re.match(r"threaded +\d+: ", ln)]
    sequential = [ln.split(": ", 1) for ln in lines if re.match(r"sequential +\d+: ", ln)]
    # per thread: 4 shifts, 11 ops at two widths, 5 scalar ops and casts, the 64-bit product, the pseudo-Mersenne
    # remainder, 8 BigUintFHE products, the audit and the refusal
    assert len(threaded) == len(sequential) == T * 43 and len(lines) == 2 * T * 43 + 1
    for (tid, tline), (sid, sline) in zip(threaded, sequential):
        assert tid.split() == ["threaded", sid.split()[1]] and tline == sline, (tid, tline, sid, sline)
    assert not any("EXPECTED" in ln for ln in lines)
    per_thread = [[ln for tid, ln in threaded if tid.split()[1] == str(i)] for i in range(T)]
    assert len({tuple(p) for p in per_thread}) == T  # operands differ per thread: so do the lines
    for i, p in enumerate(per_thread):
        assert p[0].startswith("shl bits=32") and p[2].startswith("shl bits=34")  # the shifts come first
        want = "division by zero" if i % 2 == 0 else "operands must have the same bit width"
        assert p[-1] == f"refusal rc=-1 ({want})", p[-1]


# ---------------------------------------------------------------- the Python layer
def chain(ck, rng, bits):
    """shift first, then add, mul, min, div, each result feeding the next; (handles, expected values)"""
    M = (1 << bits) - 1
    x, y, s = rng.getrandbits(bits), rng.getrandbits(bits // 2) | 1, rng.randrange(1, bits)
    X, Y, S = (FheUint.try_encrypt(v, ck, bits=bits) for v in (x, y, s))
    got, want = [X << S], [(x << s) & M]
    got.append(got[-1] + Y), want.append((want[-1] + y) & M)
    got.append(got[-1] * X), want.append((want[-1] * x) & M)
    got.append(got[-1].min(X)), want.append(min(want[-1], x))
    got.append(got[-1] // Y), want.append(want[-1] // y)
    return got, want


def test_sim_contexts_on_four_threads():
    barrier = threading.Barrier(T)
    seen = [None] * T

    def worker(i):
        ctx, ck = SimContext(), SimKey()
        set_server_key(ctx)
        try:
            rng = random.Random(0x7EAD + i)
            barrier.wait(JOIN_LIMIT)
            out = []
            for bits in (16, 34):
                got, want = chain(ck, rng, bits)
                out.append(([g.decrypt(ck) for g in got], want))
            seen[i] = out
        except BaseException:
            barrier.abort()  # a worker that fails before the barrier does not keep the others waiting
            raise
        finally:
            set_server_key(None)
            ctx.close()

    run_threads([lambda i=i: worker(i) for i in range(T)])
    for i in range(T):
        for got, want in seen[i]:
            assert got == want, i
    assert len({str(s) for s in seen}) == T  # four different programs


def test_thread_without_server_key():
    """set_server_key is per thread: the main thread's context is not the worker's"""
    ctx = SimContext()
    set_server_key(ctx)
    caught = []

    def worker():
        try:
            FheUint.encrypt_trivial(5, bits=8)
        except RuntimeError as e:
            caught.append(e)

    try:
        run_threads([worker])
        assert FheUint.encrypt_trivial(5, bits=8).decrypt(SimKey()) == 5  # the main thread's key is in place
    finally:
        set_server_key(None)
        ctx.close()
    assert len(caught) == 1 and type(caught[0]) is RuntimeError and "no server key set on this thread" in str(caught[0])


def test_last_error_is_per_thread():
    """two threads provoke different refusals, wait for each other, and only then read their messages"""
    barrier = threading.Barrier(2)
    messages = [None, None]

    def worker(i):
        ctx, ck = SimContext(), SimKey()
        set_server_key(ctx)
        try:
            x, a10 = FheUint.try_encrypt(0x5A, ck, bits=8), FheUint.try_encrypt(0x5A, ck, bits=10)
            h = C.c_void_p()
            if i == 0:
                rc = _lib.load().fhe_radix_scalar_div(ctx.handle, x.handle, 0, C.byref(h))
            else:
                rc = _lib.load().fhe_radix_add(ctx.handle, x.handle, a10.handle, C.byref(h))
            barrier.wait(JOIN_LIMIT)  # both refusals have happened
            with pytest.raises(FheError) as e:
                _lib.check(rc)
            messages[i] = (e.value.code, str(e.value))
            assert (x * 3).decrypt(ck) == (3 * 0x5A) & 0xFF  # the context works after its refusal
        except BaseException:
            barrier.abort()
            raise
        finally:
            set_server_key(None)
            ctx.close()

    run_threads([lambda: worker(0), lambda: worker(1)])
    assert messages[0] == (-1, "fhe error -1: division by zero")
    assert messages[1] == (-1, "fhe error -1: operands must have the same bit width")


# ---------------------------------------------------------------- the source
# The one function-local static that is neither const nor initialised where it is declared: the size rules a test
# moves through fhe_host_set_tuning.  Process-wide by design and documented so (include/fhe_rocm.h, "Threading"):
# set before any op runs, only read afterwards.
MUTABLE_STATICS = {("engine.cpp", "static Tuning t;")}


def static_objects(text):
    """(statement, offending) for every `static` object declaration of a .cpp file: a line that starts with
    `static` after any indentation and declares an object -- its first delimiter is `=`, `;`, `[` or `{`, where a
    function's is `(`.  thread_local objects are per thread and left out.  Offending: not const/constexpr, or no
    initialiser in the declaration."""
    out = []
    for m in re.finditer(r"^[ \t]*(static\b[^;=({\[]*)([;=({\[])", text, re.M):
        head, delim = m.group(1), m.group(2)
        if delim == "(" or "thread_local" in head:
            continue
        stmt = text[m.start():text.index("\n", m.start())].strip()
        const = re.search(r"\b(const|constexpr)\b", head) is not None
        initialised = delim != ";" and not (delim == "[" and re.match(r"[^=;]*;", text[m.end():]))
        out.append((stmt, not (const and initialised)))
    return out


def test_static_scanner_sees_the_shapes():
    src = ("int f() {\n    static std::vector<int> v;\n    static const auto t = g();\n    static int n = 0;\n"
           "    static constexpr int k[2] = {1, 2};\n    static const int z[4];\n    static bool h(int);\n}\n"
           "static double g_ns = 0.0;\nstatic thread_local int e;\n")
    assert static_objects(src) == [("static std::vector<int> v;", True), ("static const auto t = g();", False),
                                   ("static int n = 0;", True), ("static constexpr int k[2] = {1, 2};", False),
                                   ("static const int z[4];", True), ("static double g_ns = 0.0;", True)]


def test_static_objects_are_const_and_initialised_in_their_declaration():
    """csrc/*.cpp: a static object that is filled after its declaration (`static T x; if (x.empty()) ...`) or
    written later is shared mutable state between contexts on different threads; one that is const and built in
    its declaration is initialised once, under the compiler's guard"""
    offending, seen = [], 0
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith(".cpp"):
            continue
        for stmt, bad in static_objects(open(os.path.join(CSRC, name)).read()):
            seen += 1
            if bad and (name, stmt) not in MUTABLE_STATICS:
                offending.append((name, stmt))
    assert seen >= 40  # radix.cpp's and compat_chain.cpp's tables alone
    assert offending == []
    text = open(os.path.join(CSRC, "engine.cpp")).read()
    assert all(stmt in text for name, stmt in MUTABLE_STATICS)  # the exception still names something
