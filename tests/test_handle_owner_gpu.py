"""Handle ownership on the GPU: two device contexts live on device 0 with different keys (one classic, one
multi-bit, LWE dimension 16 as tests/test_lwe_dims_gpu.py::test_radix_layer_at_n16).

The positive control first -- both contexts hold pending graphs at once, their op chains and decryptions
interleaved, every value used only under its maker, every result exact against Python integers.  Then every
device-only entry point (tests/test_handle_owner.py's DEVICE_ONLY class) refuses a value of the other context with
FHE_ERR_INVALID and a message that says "another context", and both contexts compute correctly afterwards.  Then a
context goes while its handles live.

Every foreign value here sits in valid device memory of the other context and has been decrypted under its maker, so
nothing of it is pending.  A simulated value or a value pending in another engine is never passed to a device
context: those two directions are the CPU file's and tools/engine_host_check.c's, through the same engine check."""
import ctypes as C

import pytest

import compress_ref as KR
from fhe_sign import (COMPAT, FAST, PUBLIC, BigUintFHE, CompactPublicKey, CompressionKeys, CompressionParams, Context,
                      FheError, FheUint, ReRandomizationContext, Schnorr, _lib, generate_keys, set_server_key, stats)
from fhe_sign.schnorr import CURVE_ORDER
from lwe_dims import CLASSIC, MULTIBIT, product_params

pytestmark = pytest.mark.gpu
FHE_ERR_INVALID = -1
SEED = 0x0B0E5
D_PRIV = 0xB7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFEF  # BIP-340 vector 1's secret key
K0 = 0x1D2DC1652FEE3AD08434469F9AD30536A5787FEB2C7A3F7F6B3D3E3F1E0F1A2B
MSG = bytes(range(32))


class Under:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        set_server_key(self.ctx)

    def __exit__(self, *exc):
        set_server_key(None)


class Side:
    """a device context with its own keys"""

    def __init__(self, grouping, seed):
        self.ck, self.sk = generate_keys(product_params(16, grouping), seed=seed)
        self.ctx = Context(0)
        self.ctx.set_server_key(self.sk)

    def enc(self, v, bits):
        with Under(self.ctx):
            return FheUint.try_encrypt(v, self.ck, bits=bits)

    def dec(self, x):
        with Under(self.ctx):
            return x.decrypt(self.ck)


@pytest.fixture(scope="module")
def sides():
    a, b = Side(CLASSIC, SEED), Side(MULTIBIT, SEED + 1)
    yield a, b
    set_server_key(None)
    a.ctx.close()
    b.ctx.close()


def test_two_live_contexts_interleaved(sides):
    """add, mul, shift by an encrypted amount and min at 16 and 34 bits, recorded alternately under the two
    contexts so that both hold pending graphs at once; the decryptions alternate too"""
    unread = []
    for bits in (16, 34):
        M = (1 << bits) - 1
        chains = []
        for i, s in enumerate(sides):
            x, y, sh = (0x1234_5678_9 * (i + 3)) & M, (0x0FED_CBA9_87 * (i + 5)) & M, 3 + i
            chains.append({"s": s, "x": x, "y": y, "sh": sh,
                           "X": s.enc(x, bits), "Y": s.enc(y, bits), "S": s.enc(sh, bits)})
        steps = [  # (name, encrypted form, python semantics)
            ("add", lambda c: c["X"] + c["Y"], lambda c: (c["x"] + c["y"]) & M),
            ("mul", lambda c: c["add"][0] * c["X"], lambda c: (c["add"][1] * c["x"]) & M),
            ("shr", lambda c: c["mul"][0] >> c["S"], lambda c: c["mul"][1] >> c["sh"]),
            ("min", lambda c: c["shr"][0].min(c["Y"]), lambda c: min(c["shr"][1], c["y"])),
        ]
        for name, f, ref in steps:
            for c in chains:  # A records a step, then B records the same step: neither has been flushed
                with Under(c["s"].ctx):
                    c[name] = (f(c), ref(c))
        for name, _, _ in steps:
            for c in chains:
                unread.append((c["s"], c[name][0], c[name][1], (bits, name)))
    for s, got, want, what in unread:  # A, B, A, B, ...
        assert s.dec(got) == want, what


def refused(fn, *a, **kw):
    with pytest.raises(FheError, match="another context") as e:
        fn(*a, **kw)
    assert e.value.code == FHE_ERR_INVALID, e.value


def test_device_only_entry_points_refuse_foreign_values(sides):
    A, B = sides
    xa, xb_val = A.enc(0xA5C3, 16), 0x3C5A
    with Under(A.ctx):
        Da = BigUintFHE.new(D_PRIV, A.ck)
        assert Da.to_biguint(A.ck) == D_PRIV  # read once under its maker: nothing of it is pending
    assert A.dec(xa) == 0xA5C3
    xb = B.enc(xb_val, 16)
    # what the entry points need besides the handle, on B: a compression key at a small set, the public key
    cp = KR.SMALL_A
    priv, ckey = CompressionKeys.generate(B.ck, CompressionParams(cp.k, cp.N, cp.L, cp.beta, cp.ell, cp.noise, 12))
    B.ctx.set_compression_key(ckey)
    B.ctx.set_public_key(CompactPublicKey.new(B.ck))
    seed = bytes(range(32))
    sch = Schnorr()
    calls = []  # the bcast / allgather / min callbacks of the test transport: a refused broadcast makes none

    def transport():
        cbs = (_lib.TX_BCAST(lambda user, host, n, root: calls.append("bcast") or 1),
               _lib.TX_ALLGATHER(lambda user, host, seg: calls.append("allgather") or 1),
               _lib.TX_MIN_U8(lambda user, host, n: calls.append("min") or 0))
        tx = _lib.TestTransport(None, *cbs)
        _lib.check(_lib.load().fhe_ctx_attach_test_transport(B.ctx.handle, C.byref(tx), 2, 0))
        return tx, cbs

    with Under(B.ctx):
        Db = BigUintFHE.new(D_PRIV, B.ck)
        e_b, k_b = BigUintFHE.new(0x1234567, B.ck), BigUintFHE.new(0x7654321, B.ck)
        assert Db.to_biguint(B.ck) == D_PRIV
        before = stats(B.ctx)
        for x in (xa, Da):
            refused(x.serialize)
            refused(x.compress)
            refused(x.compress_switched)
            refused(x.compress_switched, rekey=True)
            refused(x.re_randomize, seed)
            refused(x.digest)
            refused(ReRandomizationContext(b"owner").add, x)
        refused(xa.export)
        refused(BigUintFHE.broadcast, Da, 0, B.ctx)  # no communicator: the root's receiving path, locally
        refused(FheUint.broadcast, xa, 0, B.ctx)
        keep = transport()
        try:
            refused(FheUint.broadcast, xa, 0, B.ctx)
            refused(BigUintFHE.broadcast, Da, 0, B.ctx)
        finally:
            B.ctx.detach_comm()
        assert calls == [], calls
        del keep
        for mode in (COMPAT, FAST, PUBLIC):
            refused(sch.sign_fhe_with_k0, MSG, K0, D_PRIV, Da, B.ck, mode)
            refused(sch.sign_fhe_with_k0, MSG, K0, D_PRIV, Da, B.ck, mode, reduce=True)
            refused(sch.sign_fhe_with_k0, MSG, K0, D_PRIV, Da, B.ck, mode, rerandomize_domain=b"owner")
            refused(sch.sign_fhe_with_k0, MSG, K0, D_PRIV, Da, B.ck, mode, rerandomize_domain=b"owner", reduce=True)
            for reduce in (False, True):  # the foreign key second: the first job's operands are B's own
                jobs = [(MSG, K0, D_PRIV, Db), (MSG, K0 + 1, D_PRIV, Da)]
                refused(sch.sign_fhe_with_k0_batch, jobs, B.ck, mode, reduce)
        refused(sch.eval_s, 5, 7, Da, PUBLIC)
        for mode in (COMPAT, FAST):
            refused(sch.eval_s, e_b, k_b, Da, mode)
            refused(sch.eval_s, Da, k_b, Db, mode)
            refused(sch.eval_s, e_b, Da, Db, mode)
        assert stats(B.ctx) == before  # not one bootstrap for any refusal
        # B's own values go through the same entry points: the keys are in place, the refusals were about ownership
        assert len(xb.digest()) == 32 and xb.export().shape[0] == 8
        assert xb.compress().decrypt(priv) == xb_val
        assert (xb * xb + xb).decrypt(B.ck) == (xb_val * xb_val + xb_val) & 0xFFFF
        assert sch.eval_s(5, 7, Db, PUBLIC).decrypt(B.ck) == (7 + 5 * D_PRIV) % CURVE_ORDER
    with Under(A.ctx):
        assert (xa * xa + xa).decrypt(A.ck) == (0xA5C3 * 0xA5C3 + 0xA5C3) & 0xFFFF
        assert Da.add(Da).to_biguint(A.ck) == 2 * D_PRIV


def test_handles_outlive_their_context(sides):
    """the first context goes while its handles live (the slots keep its block pool alive); they are dropped after
    the close, and the second context keeps computing"""
    _, B = sides
    first = Side(CLASSIC, SEED + 2)
    x = first.enc(0x1357, 16)
    with Under(first.ctx):
        y = x * x + x
        assert y.decrypt(first.ck) == (0x1357 * 0x1357 + 0x1357) & 0xFFFF
        z = y + x  # recorded, never read: pending when the context goes
        big = BigUintFHE.new(D_PRIV, first.ck)
    vb = 0x2468
    xb = B.enc(vb, 16)
    with Under(B.ctx):
        pend = xb * xb
    first.ctx.close()
    with Under(B.ctx):
        refused(x.digest)
        assert pend.decrypt(B.ck) == (vb * vb) & 0xFFFF
    del x, y, z, big
    with Under(B.ctx):
        assert ((xb + xb) * xb).decrypt(B.ck) == (2 * vb * vb) & 0xFFFF
        assert xb.min(pend).decrypt(B.ck) == min(vb, (vb * vb) & 0xFFFF)
