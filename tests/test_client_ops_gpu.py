"""Resident client key on the GPU: client_ops.hip's two kernels word for word against the host
definitions, and every routed path against a twin that takes the host path.

The twin: one client key, deserialized twice, both at seed_encryption(42, 100) and moved to the same stream
position; context A holds the key resident, context B holds none.  Whatever A computes on the device B computes on
the host, and words, plaintexts and the serialized client keys (encryption-stream state included) must be equal.
Keys are at n = 16 (tests/lwe_dims.py) except for the signer, which runs BIP-340 vector 0 at the default 834.
Nothing here asserts a time."""
import csv
import os

import numpy as np
import pytest

import ref_semantics as R
from conftest import ROOT
from fhe_sign import (COMPAT, FAULT_CLIENT, FAULT_DEFERRED, BigUintFHE, ClientKey, Context, FheError, FheUint, FheUint8,
                      FheUint32, Schnorr, _lib, compute_nonce, fault_arm, generate_keys, pending_info, set_server_key)
from lwe_dims import CLASSIC, MULTIBIT, product_params
from test_client_ops import BIG, COUNTS, W0S, advance

pytestmark = pytest.mark.gpu
FHE_ERR_INVALID, FHE_ERR_HIP, FHE_ERR_NO_KEY = -1, -2, -3
ROW0 = next(r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv"))) if r["index"] == "0")


class Env:
    def __init__(self, params, seed):
        self.params = params
        ck, self.sk = generate_keys(params, seed=seed)
        self.key_bytes = ck.serialize()
        self.A, self.B = Context(0), Context(0)
        self.A.set_server_key(self.sk)
        self.B.set_server_key(self.sk)
        self.A.set_client_key(ck)

    def twins(self, w0=0):
        out = []
        for _ in range(2):
            ck = ClientKey.deserialize(self.key_bytes)
            ck.seed_encryption(42, 100)
            advance(ck, w0)
            out.append(ck)
        return out

    def close(self):
        set_server_key(None)
        fault_arm(0)
        self.A.close()
        self.B.close()


@pytest.fixture(scope="module", params=[CLASSIC, MULTIBIT], ids=["classic", "multibit"])
def env(request):
    e = Env(product_params(16, request.param), 0xC11E + request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def env834():
    e = Env(None, 0x5A0C)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def disarmed():
    fault_arm(0)
    yield
    fault_arm(0)
    set_server_key(None)


def _same_words(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, f"first differing (row, word): {bad[0]} of {len(bad)}"


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("w0", W0S)
@pytest.mark.parametrize("count", COUNTS + [1024])
def test_rows(env, count, w0):
    ka, kb = env.twins(w0)
    values = (np.arange(count, dtype=np.uint64) * 5 + 1) % 16
    info0 = env.A.client_ops_info()
    got = env.A.client_encrypt_rows(ka, values)
    _same_words(got, kb.encrypt_blocks(values))
    assert ka.serialize() == kb.serialize()
    assert np.array_equal(ka.encrypt_blocks([9]), kb.encrypt_blocks([9]))
    assert env.A.client_ops_info() == info0  # a hook is not a path


def test_phases(env):
    ka, _ = env.twins(3)
    values = np.arange(320, dtype=np.uint64) % 16
    rows = env.A.client_encrypt_rows(ka, values)
    table = [(5 * m + 2) % 16 for m in range(16)]
    boots = env.A.pbs(rows, env.A.lut(table))
    for cts in (rows, boots, np.concatenate([boots[:7], rows[:2]])):
        got = env.A.client_phase_rows(cts)
        assert np.array_equal(got, ka.decrypt_phase_host(cts))
    assert [ka.decrypt_block(c) for c in boots] == [table[int(v)] for v in values]


# ------------------------------------------------------------------------------------------------ routed paths
def _on(ctx):
    set_server_key(ctx)
    return ctx


def _exp(ctx, x):
    set_server_key(ctx)
    return x.export()


def _ser(ctx, x):
    set_server_key(ctx)
    return x.serialize()


def test_radix(env):
    ka, kb = env.twins(3)
    A, B = env.A, env.B
    res0, enc0, ph0 = A.client_ops_info()
    assert res0 and B.client_ops_info() == (False, 0, 0)
    made = {}
    for name, (cls, bits, x, y) in {"u8": (FheUint8, 8, 0xB7, 0x6D), "u32": (FheUint32, 32, 0xDEADBEEF, 0x12345677),
                                    "u10": (FheUint, 10, 0x2F3, 0x1D9)}.items():
        for ctx, ck in ((A, ka), (B, kb)):
            _on(ctx)
            made[name, ctx] = (cls.try_encrypt(x, ck, bits=bits), cls.try_encrypt(y, ck, bits=bits))
        _same_words(_exp(A, made[name, A][0]), _exp(B, made[name, B][0]))
        _same_words(_exp(A, made[name, A][1]), _exp(B, made[name, B][1]))
        enc0 += bits
        assert A.client_ops_info() == (True, enc0, ph0), name
        M = 1 << bits
        for op, want in ((lambda a, b: a + b, (x + y) % M), (lambda a, b: a * b, (x * y) % M)):
            _on(A)
            ra = op(*made[name, A])
            assert ra.decrypt(ka) == want, name
            ph0 += bits // 2
            assert A.client_ops_info() == (True, enc0, ph0), name
            _on(B)
            rb = op(*made[name, B])
            assert rb.decrypt(kb) == want, name
            _same_words(_exp(A, ra), _exp(B, rb))
    assert ka.serialize() == kb.serialize()
    assert B.client_ops_info() == (False, 0, 0)


def test_biguint(env):
    ka, kb = env.twins(2049 + 5)
    A, B = env.A, env.B
    x, y, z = 0xFFFFFFFF_FFFFFFFE_00000001, 0xFFFFFFFF_80000001, 0xFFFFFFFF_FFFFFFFF_FFFFFFFF
    xl, yl, zl = (R.to_u32_digits(v) for v in (x, y, z))
    _, enc0, ph0 = A.client_ops_info()
    big = {}
    for ctx, ck in ((A, ka), (B, kb)):
        _on(ctx)
        big[ctx] = [BigUintFHE.new(v, ck) for v in (x, y, z)]
    assert A.client_ops_info() == (True, enc0 + 16 * (3 + 2 + 3), ph0)
    for a, b in zip(big[A], big[B]):
        assert _ser(A, a) == _ser(B, b)
    got = {}
    for ctx, ck in ((A, ka), (B, kb)):
        _on(ctx)
        bx, by, bz = big[ctx]
        s = bx.add(bz)  # a sum: read from its column form, only what that needs is launched (only_needed)
        limbs = s.decrypt_limbs(ck)
        pend = pending_info(ctx)
        got[ctx] = (limbs, pend, bx.mul(by).decrypt_limbs(ck), bx.mul_add_value(by, bz, ck))
    assert got[A] == got[B]
    limbs, _, prod, cols = got[A]
    assert limbs == R.biguint_add(xl, zl)  # carries through every limb
    assert prod == R.biguint_mul(xl, yl)
    assert cols == R.from_limbs(R.biguint_add(zl, R.biguint_mul(xl, yl)))
    # (exact counts are test_radix's: a column form reads each slot it names once, however often it names it)
    assert A.client_ops_info()[2] > ph0 and B.client_ops_info() == (False, 0, 0)
    assert ka.serialize() == kb.serialize()


def test_mismatch_and_clear(env):
    ka, kb = env.twins(0)
    other, _ = generate_keys(env.params, seed=0x0DD)
    ob = other.serialize()
    o1, o2 = ClientKey.deserialize(ob), ClientKey.deserialize(ob)
    A, B = env.A, env.B
    info0 = A.client_ops_info()
    # key B's words through the context where key A is resident: the host path, B's words, no counter moves.  (The
    # server key is A's: the value is not computed on, only encrypted, exported and read back.)
    _on(A)
    xa = FheUint32.try_encrypt(0xA5A55A5A, o1)
    _on(B)
    xb = FheUint32.try_encrypt(0xA5A55A5A, o2)
    _same_words(_exp(A, xa), _exp(B, xb))
    assert o1.serialize() == o2.serialize()
    _on(A)
    assert xa.decrypt(o1) == 0xA5A55A5A
    assert A.client_ops_info() == info0
    with pytest.raises(FheError) as e:
        A.client_encrypt_rows(o1, [1])
    assert e.value.code == FHE_ERR_INVALID
    # cleared: the host path's results, and nothing counts
    A.clear_client_key()
    try:
        assert A.client_ops_info() == (False,) + info0[1:]
        A.clear_client_key()  # twice is fine
        ya = FheUint8.try_encrypt(0x5C, ka)
        assert ya.decrypt(ka) == 0x5C
        _on(B)
        yb = FheUint8.try_encrypt(0x5C, kb)
        _same_words(_exp(A, ya), _exp(B, yb))
        assert A.client_ops_info() == (False,) + info0[1:]
        with pytest.raises(FheError) as e:
            A.client_encrypt_rows(ka, [1])
        assert e.value.code == FHE_ERR_NO_KEY
        with pytest.raises(FheError) as e:
            A.client_phase_rows(np.zeros((1, BIG), np.uint64))
        assert e.value.code == FHE_ERR_NO_KEY
    finally:
        A.set_client_key(ka)
    assert A.client_ops_info() == (True,) + info0[1:]


def test_install_refusals_and_rekey(env):
    lib = _lib.load()
    ka, _ = env.twins(0)
    bare = Context(0)
    try:
        assert lib.fhe_ctx_set_client_key(bare.handle, ka.handle) == FHE_ERR_NO_KEY
        assert bare.client_ops_info() == (False, 0, 0)
        bare.clear_client_key()
        # parameters that differ from the installed server key's
        p = product_params(15 if env.params.grouping == CLASSIC else 2, env.params.grouping)
        ck2, sk2 = generate_keys(p, seed=7)
        bare.set_server_key(env.sk)
        assert lib.fhe_ctx_set_client_key(bare.handle, ck2.handle) == FHE_ERR_INVALID
        assert b"lwe_dimension" in lib.fhe_last_error()
        assert lib.fhe_ctx_set_client_key(bare.handle, None) == FHE_ERR_INVALID
        bare.set_client_key(ka)
        assert bare.client_ops_info()[0]
        bare.set_server_key(env.sk)  # the same parameters again: the key stays
        assert bare.client_ops_info()[0]
        set_server_key(bare)
        assert FheUint8.try_encrypt(0x3C, ka).decrypt(ka) == 0x3C
        assert bare.client_ops_info() == (True, 4, 4)
        bare.set_server_key(sk2)     # other parameters: wiped and gone
        assert bare.client_ops_info() == (False, 4, 4)
    finally:
        set_server_key(None)
        bare.close()


# ------------------------------------------------------------------------------------------------ failure
def _injected(call):
    with pytest.raises(FheError, match="injected fault at CLIENT") as e:
        call()
    assert e.value.code == FHE_ERR_HIP
    fault_arm(0)


def test_failed_encryption_and_decryption(env):
    ka, kb = env.twins(3)
    A, B = env.A, env.B
    info0 = A.client_ops_info()
    _on(A)
    pend0 = pending_info(A)
    fault_arm(FAULT_CLIENT, 1)
    _injected(lambda: FheUint32.try_encrypt(0x0BADF00D, ka))
    assert A.client_ops_info() == info0 and pending_info(A) == pend0 and pend0[1:] == (0, 0)
    xa = FheUint32.try_encrypt(0x0BADF00D, ka)  # the call again
    ya = FheUint32.try_encrypt(0x00C0FFEE, ka)
    # the host path's failed call has drawn its words before it fails: the twin makes the call twice
    _on(B)
    FheUint32.try_encrypt(0x0BADF00D, kb)
    xb = FheUint32.try_encrypt(0x0BADF00D, kb)
    yb = FheUint32.try_encrypt(0x00C0FFEE, kb)
    assert ka.serialize() == kb.serialize()
    _same_words(_exp(A, xa), _exp(B, xb))
    want = (0x0BADF00D * 0x00C0FFEE) % (1 << 32)
    _on(A)
    ra = xa * ya
    fault_arm(FAULT_CLIENT, 1)
    _injected(lambda: ra.decrypt(ka))  # after its flush, before its launch
    assert pending_info(A) == (0, 0, 0)  # the flush went through: nothing is left to launch
    assert ra.decrypt(ka) == want
    assert A.client_ops_info() == (True, info0[1] + 32, info0[2] + 16)
    _on(B)
    rb = xb * yb
    assert rb.decrypt(kb) == want
    _same_words(_exp(A, ra), _exp(B, rb))


@pytest.mark.parametrize("k", [1, 2], ids=["encrypt", "phase"])
def test_failed_signer(env, k):
    d, msg, aux = int(ROW0["secret key"], 16), bytes.fromhex(ROW0["message"]), bytes.fromhex(ROW0["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    ka, kb = env.twins(0)
    s = Schnorr()
    _on(env.A)
    da = BigUintFHE.new(d, ka)
    fault_arm(FAULT_CLIENT, k)
    _injected(lambda: s.sign_fhe_with_k0(msg, k0, d, da, ka, COMPAT))
    assert pending_info(env.A)[1:] == (0, 0)
    assert da.to_biguint(ka) == d
    sig = s.sign_fhe_with_k0(msg, k0, d, da, ka, COMPAT)
    assert sig.hex().upper() == ROW0["signature"].upper()
    # the twin: a successful call with the same inputs, then the call again
    _on(env.B)
    db = BigUintFHE.new(d, kb)
    assert s.sign_fhe_with_k0(msg, k0, d, db, kb, COMPAT) == sig
    assert db.to_biguint(kb) == d
    assert s.sign_fhe_with_k0(msg, k0, d, db, kb, COMPAT) == sig
    assert ka.serialize() == kb.serialize()


# ------------------------------------------------------------------------------------------------ the signer, n = 834
@pytest.mark.parametrize("form", ["plain", "reduced", "callsite"])
def test_signer(env834, form):
    e = env834
    d, msg, aux = int(ROW0["secret key"], 16), bytes.fromhex(ROW0["message"]), bytes.fromhex(ROW0["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    ka, kb = e.twins(3)
    s = Schnorr()

    def sign(ck, dk):
        if form == "callsite":
            return s.sign_fhe_with_k0_callsite(msg, k0, d, dk, ck, COMPAT)
        return s.sign_fhe_with_k0(msg, k0, d, dk, ck, COMPAT, reduce=(form == "reduced"))

    _on(e.A)
    _, enc0, ph0 = e.A.client_ops_info()
    da = BigUintFHE.new(d, ka)
    fault_arm(FAULT_DEFERRED, 0)  # counts the deferred uploads that run: none may
    sig_a = sign(ka, da)
    assert fault_arm(0) == 0
    assert pending_info(e.A)[1:] == (0, 0)
    _, enc1, ph1 = e.A.client_ops_info()
    # 16 blocks per limb: d as many limbs as it has (vector 0's is 3: one), e and k eight each
    assert enc1 - enc0 == 16 * (len(R.to_u32_digits(d)) + 8 + 8) and ph1 > ph0
    _on(e.B)
    db = BigUintFHE.new(d, kb)
    sig_b = sign(kb, db)
    assert sig_a == sig_b and sig_a.hex().upper() == ROW0["signature"].upper()
    assert ka.serialize() == kb.serialize()
    assert e.B.client_ops_info() == (False, 0, 0)
