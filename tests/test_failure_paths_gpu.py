"""What a failed call leaves behind, on the GPU (include/fhe_rocm.h, "Errors after validation").  Every induced error
is a host exception of the fault point (FHE_TUNE_FAULT_SITES: it throws before a launch, it never changes one) or
an ordinary argument refusal; no device fault is provoked.

Keys at n = 16 (tests/lwe_dims.py), classic and multi-bit, one module fixture per grouping.  Each scenario uses two
contexts under the same server key: the one whose call fails, and a twin that computes the same program from the same
input words (the operands are serialized once and deserialized under both) and never fails.  Bootstraps are
deterministic, so every comparison is exact equality of exported u64 words, plus the decryption.

  plain flush     a 34-bit a * b + c; the decryption's flush fails at its first, middle and last level, before
                  the descriptors are staged, and before the workspace is sized; the retry's words equal the twin's
  partial flush   p = a * b held, t = p + k at 2 and 3 limbs; decrypt(t) launches only what t's column form needs
                  and fails at its second level; then p decrypts to a * b and exports the twin's words (what the
                  partial flush set aside used to be dropped marked "written": unwritten slots), t to the sum
  signer          a mode the block refuses after the helper thread that encrypts e and k was started; the fault
                  point inside the upload of e and k and inside the flush; compat and reduced.  After each error:
                  no upload armed, no helper in flight (fhe_ctx_pending_info), the client key serializes to the bytes
                  of a twin key (same seeds) after a SUCCESSFUL signature of the same inputs, its next encryption
                  gives the twin's words, and a correct signature of BIP-340 vector 0 follows
  batch signer    the same refusal in a batch of three; a recording that fails in the second job and a level that
                  fails in its eager tail flush: the private keys still decrypt, a rerun signs all three"""
import csv
import os
import random

import numpy as np
import pytest

import ref_semantics as R
from conftest import ROOT
from fhe_sign import (COMPAT, FAST, FAULT_DEFERRED, FAULT_LEVEL, FAULT_RECORD, FAULT_STAGE, FAULT_WORKSPACE, BigUintFHE,
                      Context, FheError, FheUint, Schnorr, compute_nonce, fault_arm, generate_keys, pending_info,
                      set_server_key, stats)
from lwe_dims import CLASSIC, MULTIBIT, product_params
from test_keyswitch_gpu import _assert_words

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
FHE_ERR_INVALID, FHE_ERR_HIP = -1, -2
ROWS = {r["index"]: r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv")))}


class Env:
    def __init__(self, grouping):
        self.params = product_params(16, grouping)
        self.ck, self.sk = generate_keys(self.params, seed=SEED)
        self.A, self.B = Context(0), Context(0)
        self.A.set_server_key(self.sk)
        self.B.set_server_key(self.sk)

    def close(self):
        set_server_key(None)
        fault_arm(0)
        self.A.close()
        self.B.close()


@pytest.fixture(scope="module", params=[CLASSIC, MULTIBIT], ids=["classic", "multibit"])
def env(request):
    e = Env(request.param)
    yield e
    e.close()


@pytest.fixture(autouse=True)
def disarmed():
    fault_arm(0)
    yield
    fault_arm(0)
    set_server_key(None)


def _injected(call, site):
    with pytest.raises(FheError, match="injected fault at " + site) as e:
        call()
    assert e.value.code == FHE_ERR_HIP
    fault_arm(0)


def _both(env, values, bits):
    """the same ciphertext words under both contexts"""
    set_server_key(env.A)
    blobs = [FheUint.try_encrypt(v, env.ck, bits=bits).serialize() for v in values]
    out = []
    for ctx in (env.A, env.B):
        set_server_key(ctx)
        out.append([FheUint.deserialize(b) for b in blobs])
    return out


def _both_big(env, limb_lists):
    set_server_key(env.A)
    blobs = [BigUintFHE.new(R.from_limbs(l), env.ck).serialize() for l in limb_lists]
    out = []
    for ctx in (env.A, env.B):
        set_server_key(ctx)
        out.append([BigUintFHE.deserialize(b) for b in blobs])
    return out


# ------------------------------------------------------------------------------------------------ plain flush
def test_plain_flush_failed_and_retried(env):
    bits = 34
    M = 1 << bits
    rng = random.Random(0xF1A5)
    x, y, z = rng.getrandbits(bits) | M // 2, rng.getrandbits(bits) | 1, rng.getrandbits(bits)
    want = (x * y + z) % M
    (XA, YA, ZA), (XB, YB, ZB) = _both(env, (x, y, z), bits)
    # the twin, with the LEVEL site counting: the levels of the decryption's flush
    set_server_key(env.B)
    RB = XB * YB + ZB
    fault_arm(FAULT_LEVEL, 0)
    assert RB.decrypt(env.ck) == want
    levels = fault_arm(0)
    assert levels >= 3
    twin = RB.export()
    set_server_key(env.A)
    for site, name, k in ((FAULT_LEVEL, "LEVEL", 1), (FAULT_LEVEL, "LEVEL", (levels + 1) // 2), (FAULT_LEVEL, "LEVEL", levels),
                          (FAULT_STAGE, "STAGE", 1), (FAULT_WORKSPACE, "WORKSPACE", 1)):
        RA = XA * YA + ZA
        pbs0, lv0 = stats(env.A)
        fault_arm(site, k)
        _injected(lambda: RA.decrypt(env.ck), name)
        launched = k - 1 if site == FAULT_LEVEL else 0
        assert stats(env.A)[1] - lv0 == launched, (name, k)  # the level that failed does not count
        assert pending_info(env.A)[0] > 0, (name, k)           # everything recorded is still pending
        assert RA.decrypt(env.ck) == want, (name, k)
        assert stats(env.A)[1] - lv0 == launched + levels, (name, k)  # relaunched levels count again
        assert pending_info(env.A) == (0, 0, 0), (name, k)
        _assert_words(RA.export(), twin, f"a * b + c after a failed flush at {name} {k} against the twin")
        del RA


# ------------------------------------------------------------------------------------------------ partial flush
@pytest.mark.parametrize("mode", [COMPAT, FAST], ids=["compat", "fast"])
@pytest.mark.parametrize("n", [2, 3])
def test_partial_flush_failed_keeps_the_held_product(env, n, mode):
    rng = random.Random(0xCA11 * n + mode)
    al = [rng.getrandbits(32) | 1 << 31 for _ in range(n)]
    bl, kl = ([rng.getrandbits(32) | 1 for _ in range(n)] for _ in range(2))
    pl = R.biguint_mul(al, bl) if mode == COMPAT else R.to_u32_digits(R.from_limbs(al) * R.from_limbs(bl))
    tl = R.biguint_add(pl, kl)

    def same(got, want_limbs):
        return got == want_limbs if mode == COMPAT else R.from_limbs(got) == R.from_limbs(want_limbs)

    (aA, bA, kA), (aB, bB, kB) = _both_big(env, (al, bl, kl))
    set_server_key(env.B)
    pB = aB.mul(bB, mode)
    tB = pB.add(kB)
    assert same(tB.decrypt_limbs(env.ck), tl)
    assert same(pB.decrypt_limbs(env.ck), pl)
    set_server_key(env.A)
    pA = aA.mul(bA, mode)
    tA = pA.add(kA)
    fault_arm(FAULT_LEVEL, 2)
    _injected(lambda: tA.decrypt_limbs(env.ck), "LEVEL")
    assert pending_info(env.A)[0] > 0
    assert same(pA.decrypt_limbs(env.ck), pl), "the held product after the failed partial flush"
    assert same(tA.decrypt_limbs(env.ck), tl)
    for what, hA, hB in (("p", pA, pB), ("t", tA, tB)):
        set_server_key(env.A)
        wordsA = hA.to_radix(32 * len(hA)).export()
        set_server_key(env.B)
        wordsB = hB.to_radix(32 * len(hB)).export()
        _assert_words(wordsA, wordsB, f"{what} after the failed partial flush against the twin ({n} limbs)")
    set_server_key(env.A)
    del pA, tA
    x = FheUint.try_encrypt(5, env.ck, bits=4)
    assert (x + x).decrypt(env.ck) == 10
    assert pending_info(env.A) == (0, 0, 0)


# ------------------------------------------------------------------------------------------------ the signer
def _vector(idx="0"):
    row = ROWS[idx]
    d = int(row["secret key"], 16)
    msg, aux = bytes.fromhex(row["message"]), bytes.fromhex(row["aux_rand"])
    return row, d, msg, compute_nonce(d, msg, aux)


def _client_keys(env, stream_seed):
    """the context's client key twice, made anew: the same secret key, the same history (a serialized key holds
    its stream's buffered block too, which a reseeding keeps), each with a stream of its own"""
    ck, ck2 = (generate_keys(env.params, seed=SEED)[0] for _ in range(2))
    assert ck.serialize() == ck2.serialize()
    assert all(np.array_equal(u, v) for u, v in zip(ck.export(), env.ck.export()))  # the installed key's secret
    ck.seed_encryption(stream_seed)
    ck2.seed_encryption(stream_seed)
    return ck, ck2


def _twin_after_success(env, ck2, jobs, reduce=False, batch=False):
    """the twin key after the same encryptions and a SUCCESSFUL call with the same inputs under the twin context"""
    set_server_key(env.B)
    keys = [BigUintFHE.new(d, ck2) for _, _, d in jobs]
    s = Schnorr()
    if batch:
        sigs = s.sign_fhe_with_k0_batch([(m, k0, d, f) for (m, k0, d), f in zip(jobs, keys)], ck2, COMPAT, reduce=reduce)
    else:
        (m, k0, d), = jobs
        sigs = [s.sign_fhe_with_k0(m, k0, d, keys[0], ck2, COMPAT, reduce=reduce)]
    for (m, k0, d), sig in zip(jobs, sigs):
        assert sig == s.sign_with_k0(m, k0, d)
    return ck2.serialize()


def _after_the_error(env, ck, ck2, twin_bytes, keys, jobs, reduce=False):
    """the post-conditions of a signer entry point that returned an error"""
    info = pending_info(env.A)
    assert info[1:] == (0, 0), f"armed upload / helper in flight after the error: {info}"
    assert ck.serialize() == twin_bytes, "the client key's stream is not where a successful call leaves it"
    _assert_words(ck.encrypt_blocks([1, 2, 3]), ck2.encrypt_blocks([1, 2, 3]), "the next encryption against the twin key's")
    for (m, k0, d), f in zip(jobs, keys):
        assert f.to_biguint(ck) == d  # the encrypted private key reads what it read before
    s = Schnorr()
    for (m, k0, d), f in zip(jobs, keys):
        assert s.sign_fhe_with_k0(m, k0, d, f, ck, COMPAT, reduce=reduce) == s.sign_with_k0(m, k0, d)


def test_signer_refusal_after_the_helper_started(env):
    """mode 7 is refused by the multiply-add inside the FHE block, after sign_prepare started the encryption of e and
    k on its helper thread and armed their upload"""
    row, d, msg, k0 = _vector("0")
    jobs = [(msg, k0, d)]
    ck, ck2 = _client_keys(env, 0x51)
    twin = _twin_after_success(env, ck2, jobs)
    set_server_key(env.A)
    d_fhe = BigUintFHE.new(d, ck)
    with pytest.raises(FheError) as e:
        Schnorr().sign_fhe_with_k0(msg, k0, d, d_fhe, ck, 7)
    assert e.value.code == FHE_ERR_INVALID
    _after_the_error(env, ck, ck2, twin, [d_fhe], jobs)
    assert Schnorr().sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT).hex().upper() == row["signature"].upper()


def test_batch_signer_refusal(env):
    jobs = [_vector(i)[1:] for i in ("0", "1", "2")]
    jobs = [(m, k0, d) for d, m, k0 in jobs]
    ck, ck2 = _client_keys(env, 0x52)
    twin = _twin_after_success(env, ck2, jobs, batch=True)
    set_server_key(env.A)
    keys = [BigUintFHE.new(d, ck) for _, _, d in jobs]
    with pytest.raises(FheError) as e:
        Schnorr().sign_fhe_with_k0_batch([(m, k0, d, f) for (m, k0, d), f in zip(jobs, keys)], ck, 7)
    assert e.value.code == FHE_ERR_INVALID
    _after_the_error(env, ck, ck2, twin, keys, jobs)


@pytest.mark.parametrize("reduce", [False, True], ids=["compat", "reduced"])
@pytest.mark.parametrize("site,name,k", [(FAULT_DEFERRED, "DEFERRED", 1), (FAULT_LEVEL, "LEVEL", 1), (FAULT_LEVEL, "LEVEL", 3)])
def test_signer_with_an_injected_fault(env, site, name, k, reduce):
    row, d, msg, k0 = _vector("0")
    jobs = [(msg, k0, d)]
    ck, ck2 = _client_keys(env, 0x53 + k)
    twin = _twin_after_success(env, ck2, jobs, reduce=reduce)
    set_server_key(env.A)
    d_fhe = BigUintFHE.new(d, ck)
    fault_arm(site, k)
    _injected(lambda: Schnorr().sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT, reduce=reduce), name)
    _after_the_error(env, ck, ck2, twin, [d_fhe], jobs, reduce=reduce)
    assert Schnorr().sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT, reduce=reduce).hex().upper() == row["signature"].upper()


def test_batch_signer_with_an_injected_fault(env):
    """a recording that fails in the second job, and a level that fails in the second job's eager tail flush (the
    first job's block products are launched by a plain flush as they are recorded: LEVEL crossing 1; the second
    job's by flush_tail, behind the first job's pending graph: crossing 2)"""
    jobs = [_vector(i)[1:] for i in ("0", "1", "2")]
    jobs = [(m, k0, d) for d, m, k0 in jobs]
    set_server_key(env.A)
    keys = [BigUintFHE.new(d, env.ck) for _, _, d in jobs]
    s = Schnorr()
    batch = [(m, k0, d, f) for (m, k0, d), f in zip(jobs, keys)]
    want = [s.sign_with_k0(m, k0, d) for m, k0, d in jobs]
    # recordings of one job's block: counted on a single signature
    fault_arm(FAULT_RECORD, 0)
    assert s.sign_fhe_with_k0(jobs[0][0], jobs[0][1], jobs[0][2], keys[0], env.ck, COMPAT) == want[0]
    per_job = fault_arm(0)
    assert per_job >= 2
    for site, name, k in ((FAULT_RECORD, "RECORD", per_job + 2), (FAULT_LEVEL, "LEVEL", 2)):
        fault_arm(site, k)
        _injected(lambda: s.sign_fhe_with_k0_batch(batch, env.ck, COMPAT), name)
        assert pending_info(env.A)[1:] == (0, 0), name
        for (m, k0, d), f in zip(jobs, keys):
            assert f.to_biguint(env.ck) == d, name
        assert s.sign_fhe_with_k0_batch(batch, env.ck, COMPAT) == want, name
    assert want[0].hex().upper() == ROWS["0"]["signature"].upper()
