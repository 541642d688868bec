"""Modulus-switched stored ciphertexts on the GPU (include/fhe_rocm.h): the two kernels of
switched.hip through their hooks against the host definitions, byte for byte and word for word;
x.compress_switched() against fhe_switched_compress_host of the exported blocks in both modulus-switch modes;
decompress() against the direct bootstrap of the blocks and against the oracle's blind rotation of the stored
rows; x.compress_switched(rekey=True) against the host definition under the re-keying key, read by the
destination's client key and bootstrapped by the destination's server key.  Keys at the dimensions of
tests/lwe_dims.py where a row has a pad nibble (16, 256) or none (15, 255), a tail unit or none (255: n + 1 = 256 is
whole units), classic and multi-bit, plus the default parameters once.

Decode checks compare against the host definition on fixed seeds (tests/test_switched.py asserts that the
restatement decodes these inputs), not against a probability.

Not covered here, because no public entry point hands back such a block: a lazy block (it goes through the same
realize() as re_randomize's and digest's inputs) and a block whose noise label is above the budget of a lookup
(the radix layer and the deserializers keep every label at or below it; the engine refuses such a block)."""
import numpy as np
import pytest

import compress_ref as R
import oracle
import switched_ref as S
from fhe_sign import (BigUintFHE, Context, FheError, FheUint, RekeyKey, SwitchedCiphertextList, generate_keys, set_server_key,
                      switched_pack_host, switched_unpack_host)
from fhe_sign.core import MS_PAD_WORD, SWITCHED_GAP_BYTE
from lwe_dims import CLASSIC, MULTIBIT, oracle_params, product_params

pytestmark = pytest.mark.gpu
KEY_SEED = 0x5317C4ED
RADIX, BIGUINT = S.RADIX, S.BIGUINT
MODES = ("standard", "centered")
COUNTS = (1, 2, 3, 255, 257)
KEY_SETS = [(15, CLASSIC), (16, MULTIBIT), (255, CLASSIC), (256, CLASSIC)]
DEFAULT = (834, CLASSIC)

_envs = {}


class Env:
    def __init__(self, n, g):
        default = (n, g) == DEFAULT
        self.n, self.g = n, g
        self.ck, self.sk = generate_keys(None if default else product_params(n, g), seed=KEY_SEED)
        self.ok = oracle.OracleKeys(KEY_SEED, None if default else oracle_params(n, g))
        assert np.array_equal(self.ck.export()[0], self.ok.lwe_sk)
        self.main = S.main_bytes(n, g)
        self.ctx = Context(0)
        self.ctx.set_server_key(self.sk)
        self.ident = self.ctx.lut(list(range(16)))

    def use(self, mode="standard"):
        set_server_key(self.ctx)
        self.ctx.set_modulus_switch(mode)
        return self

    def raw(self, cts, degree, noise=1):
        """an FheUint around given block ciphertexts (through the radix wire format)"""
        return FheUint.deserialize(R.raw_radix_blob(self.main, cts, degree, noise))

    def host(self, cts, lst, mode):
        """fhe_switched_compress_host on exported blocks, with the form, count and degrees the GPU list carries"""
        form, count, degrees, _ = S.parse_list(self.n, lst.serialize())
        return SwitchedCiphertextList.compress_host(self.sk, cts, degrees, form, count, mode)


def env(n, g, mode="standard"):
    if (n, g) not in _envs:
        _envs[(n, g)] = Env(n, g)
    return _envs[(n, g)].use(mode)


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    set_server_key(None)
    for e in _envs.values():
        e.ctx.close()
    _envs.clear()


@pytest.fixture(scope="module")
def bare():
    ctx = Context(0)  # no server key: the hooks need none
    yield ctx
    ctx.close()


def _value(bits, salt=0):
    return int.from_bytes(np.random.default_rng(bits + salt).bytes((bits + 7) // 8), "little") % (1 << bits)


def exported(x):
    return x.export() if isinstance(x, FheUint) else np.concatenate([d.export() for d in x.digits])


# ---------------------------------------------------------------- the kernels alone
@pytest.mark.parametrize("n", S.N_LIST)
def test_pack_rows_equal_host(bare, n):
    rb, ws = S.row_bytes(n), S.ws_stride(n)
    rows = S.edge_rows(n, max(COUNTS))
    for stride in (n + 1, ws, ws + 5):
        wide = np.full((max(COUNTS), stride), 0xFFFFFFFFFFFFFFFF, np.uint64)  # a reader of the padding would pack ones
        wide[:, :n + 1] = rows
        for bs in (rb, rb + 3):
            ref = switched_pack_host(wide, n, bs)
            for count in COUNTS:
                got = bare.switched_pack_rows(wide[:count], n, bs)
                bad = np.flatnonzero((got != ref[:count]).any(axis=1))
                assert bad.size == 0, f"n {n}, {count} rows, stride {stride}, byte stride {bs}: rows {bad[:5]} differ"
                assert (got[:, rb:] == SWITCHED_GAP_BYTE).all(), "bytes between the rows were written"


@pytest.mark.parametrize("n", S.N_LIST)
def test_unpack_rows_equal_host(bare, n):
    rb, ws = S.row_bytes(n), S.ws_stride(n)
    tight = switched_pack_host(S.edge_rows(n, max(COUNTS), seed=1), n)
    for bs in (rb, rb + 3):
        packed = np.full((max(COUNTS), bs), 0xFF, np.uint8)  # set bits behind a row: not the row's
        packed[:, :rb] = tight
        for stride in (n + 1, ws, ws + 5):
            ref = switched_unpack_host(packed, n, stride)
            for count in COUNTS:
                got = bare.switched_unpack_rows(packed[:count], n, stride)
                bad = np.flatnonzero((got != ref[:count]).any(axis=1))
                assert bad.size == 0, f"n {n}, {count} rows, stride {stride}, byte stride {bs}: rows {bad[:5]} differ"
                assert (got[:, n + 1:] == np.uint64(MS_PAD_WORD)).all()


def test_hooks_refuse_bad_shapes(bare):
    with pytest.raises(FheError):
        bare.switched_pack_rows(np.zeros((1, 16), np.uint64), 16)
    with pytest.raises(FheError):
        bare.switched_pack_rows(np.zeros((1, 17), np.uint64), 16, S.row_bytes(16) - 1)
    with pytest.raises(FheError):
        bare.switched_unpack_rows(np.zeros((1, 26), np.uint8), 16, 16)
    assert bare.switched_pack_rows(np.zeros((0, 17), np.uint64), 16).shape == (0, 26)


# ---------------------------------------------------------------- compression
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,g", KEY_SETS + [DEFAULT], ids=lambda v: str(v))
def test_compress_is_byte_identical_to_the_host(n, g, mode):
    e = env(n, g, mode)
    B = 128 if (n, g) == DEFAULT else 21
    v = _value(2 * B, n)
    x = FheUint.try_encrypt(v, e.ck, bits=2 * B)
    lst = x.compress_switched()
    blob = lst.serialize()
    assert (lst.nblocks, lst.bits, lst.params.lwe_dimension, lst.params.grouping) == (B, 2 * B, n, g)
    assert len(blob) == S.wire_len(n, B)
    assert blob == e.host(x.export(), lst, mode).serialize()
    assert lst.decrypt(e.ck) == v


@pytest.mark.parametrize("n,g", KEY_SETS, ids=lambda v: str(v))
def test_compress_biguint_trivial_and_high_degrees(n, g):
    e = env(n, g)
    # BigUintFHE form: two limbs
    v = _value(64, n) | 1 << 63
    x = BigUintFHE.new(v, e.ck)
    lst = x.compress_switched()
    assert (lst.nblocks, lst.bits) == (32, 64)
    assert lst.serialize() == e.host(exported(x), lst, "standard").serialize()
    assert lst.decrypt(e.ck) == v
    # a trivial value enters as (0, delta value): the stored row is zero but for the body, value * 128
    t = FheUint.encrypt_trivial(0xE4, bits=8)
    form, count, degrees, rows = S.parse_list(n, t.compress_switched().serialize())
    assert (form, count) == (RADIX, 8)
    for k, row in enumerate(rows):
        vals = R.unpack12(row, n + 1)
        assert not vals[:n].any() and vals[n] == 128 * ((0xE4 >> (2 * k)) & 3)
    assert t.compress_switched().decrypt(e.ck) == 0xE4
    # blocks of every value at degree 15: they carry into their neighbours
    vals = [(5 * i + 3) % 16 for i in range(16)]
    y = e.raw(e.ck.encrypt_blocks(vals), 15)
    lst = y.compress_switched()
    assert S.parse_list(n, lst.serialize())[2] == [15] * 16
    assert lst.serialize() == e.host(y.export(), lst, "standard").serialize()
    assert lst.decrypt(e.ck) == sum(b << (2 * k) for k, b in enumerate(vals)) % (1 << 32)


def test_compress_refusals():
    e = env(15, CLASSIC)
    x = FheUint.try_encrypt(5, e.ck, bits=8)
    lst = x.compress_switched()
    other = env(16, MULTIBIT)
    with pytest.raises(FheError, match="lwe_dimension"):
        lst.decompress()
    big = BigUintFHE.new(5, other.ck).compress_switched()
    with pytest.raises(FheError, match="BigUintFHE"):
        _lib_expand_radix(other, big)
    bare = Context(0)
    try:
        with pytest.raises(FheError) as err:
            lst.decompress(bare)
        assert err.value.code == -3  # FHE_ERR_NO_KEY
    finally:
        bare.close()


def _lib_expand_radix(e, lst):
    import ctypes as C

    from fhe_sign._lib import check, load
    h = C.c_void_p()
    check(load().fhe_switched_expand_radix(e.ctx.handle, lst.handle, C.byref(h)))


# ---------------------------------------------------------------- decompression
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,g", KEY_SETS + [DEFAULT], ids=lambda v: str(v))
def test_decompress_equals_direct_bootstrap_and_oracle(n, g, mode):
    e = env(n, g, mode)
    B = 128 if (n, g) == DEFAULT else 21
    v = _value(2 * B, n + 1)
    x = FheUint.try_encrypt(v, e.ck, bits=2 * B)
    cts = x.export()
    lst = SwitchedCiphertextList.deserialize(x.compress_switched().serialize())
    y = lst.decompress()
    got = y.export()
    # word for word the bootstrap of the blocks themselves through the identity table, in the same mode
    direct = e.ctx.pbs(cts, e.ident)
    bad = np.flatnonzero((got != direct).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {B} blocks differ from fhe_pbs_batch, first {bad[:5]}"
    # and the oracle's blind rotation of the stored rows as they are: in the centered mode too nothing touches
    # them between the unpacking and the rotation
    rows = S.parse_list(n, lst.serialize())[3]
    idx = np.arange(B) if B <= 21 else np.unique(np.r_[0, B - 1, np.arange(14) * (B - 3) // 13 + 1])
    ref = R.oracle_decompress(e.ok, S.unpack_rows([rows[i] for i in idx], n))
    bad = np.flatnonzero((got[idx] != ref).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {len(idx)} blocks differ from the oracle, first {idx[bad[:5]]}"
    # a clean operand again
    assert y.decrypt(e.ck) == v
    assert (y + 1).decrypt(e.ck) == (v + 1) % (1 << (2 * B))
    assert (y + x).decrypt(e.ck) == 2 * v % (1 << (2 * B))


def test_decompress_biguint_and_degrees():
    e = env(256, CLASSIC)
    v = _value(64, 7) | 1 << 63
    y = BigUintFHE.new(v, e.ck).compress_switched().decompress()
    assert isinstance(y, BigUintFHE) and y.to_biguint(e.ck) == v
    vals = [(7 * i + 2) % 16 for i in range(8)]
    x = e.raw(e.ck.encrypt_blocks(vals), 15)
    z = x.compress_switched().decompress()
    assert [e.ck.decrypt_block(c) for c in z.export()] == vals
    # the degree byte is the block's degree again: a sum that is legal for degree-3 blocks must not be taken
    w = SwitchedCiphertextList.deserialize(z.compress_switched().serialize())
    assert S.parse_list(256, w.serialize())[2] == [15] * 8


# ---------------------------------------------------------------- more than one workspace chunk
def test_chunked_list_round_trips():
    """257 limbs = 4112 blocks at n = 15: the chunk of a fresh context is 4096 rows, so both directions take two"""
    ctx = Context(0)
    try:
        e = env(15, CLASSIC)
        ctx.set_server_key(e.sk)
        set_server_key(ctx)
        v = _value(257 * 32, 3) | (1 << (257 * 32 - 1))
        x = BigUintFHE.new(v, e.ck)
        lst = x.compress_switched()
        assert lst.nblocks == 4112
        assert lst.serialize() == e.host(exported(x), lst, "standard").serialize()
        assert lst.decrypt(e.ck) == v
        y = lst.decompress()
        assert y.to_biguint(e.ck) == v
        direct = ctx.pbs(exported(x), ctx.lut(list(range(16))))
        assert np.array_equal(exported(y), direct)
    finally:
        set_server_key(None)
        ctx.close()


# ---------------------------------------------------------------- re-keying through the stored form
RK_SEED = bytes(range(9, 41))
REKEY_SETS = [((16, CLASSIC), (15, CLASSIC)), ((256, CLASSIC), (256, MULTIBIT)), (DEFAULT, (256, CLASSIC))]


@pytest.mark.parametrize("src,dst", REKEY_SETS, ids=lambda v: str(v))
def test_rekeyed_store_is_the_destinations(src, dst):
    b = env(*dst)
    a = env(*src)  # the thread's context from here on
    B = 21
    v, w = _value(2 * B, 11), _value(2 * B, 12)
    x, y = FheUint.try_encrypt(v, a.ck, bits=2 * B), FheUint.try_encrypt(w, a.ck, bits=2 * B)
    cts = x.export()
    ks_before, sum_before = a.ctx.keyswitch(cts), (x + y).export()
    with pytest.raises(FheError) as err:
        x.compress_switched(rekey=True)
    assert err.value.code == -3  # FHE_ERR_NO_KEY: none installed yet
    key = RekeyKey.new(a.ck, b.ck, RK_SEED)
    a.ctx.set_rekey_key(key)
    try:
        # nothing else of the context changes
        assert np.array_equal(a.ctx.keyswitch(cts), ks_before)
        assert np.array_equal((x + y).export(), sum_before)
        assert x.compress_switched().serialize() == e_host_plain(a, x)
        for mode in MODES:
            a.use(mode)
            lst = x.compress_switched(rekey=True)
            assert (lst.params.lwe_dimension, lst.params.grouping, lst.nblocks) == (*dst, B)
            form, count, degrees, _ = S.parse_list(dst[0], lst.serialize())
            host = SwitchedCiphertextList.compress_host(key, cts, degrees, form, count, mode)
            assert lst.serialize() == host.serialize(), f"{mode}: the re-keyed bytes differ from the host definition"
            assert lst.decrypt(b.ck) == v
            # under B an ordinary stored value: B's server key bootstraps it
            b.use()
            z = lst.decompress()
            assert z.decrypt(b.ck) == v
            assert (z + 1).decrypt(b.ck) == (v + 1) % (1 << (2 * B))
            with pytest.raises(FheError):
                lst.decompress(a.ctx)  # not a value of A's any more
            a.use(mode)
        a.use()
        # every server-key install drops the key
        a.ctx.set_server_key(a.sk)
        a.ident = a.ctx.lut(list(range(16)))
        with pytest.raises(FheError) as err:
            x2 = FheUint.try_encrypt(v, a.ck, bits=2 * B)
            x2.compress_switched(rekey=True)
        assert err.value.code == -3
    finally:
        a.use()


def e_host_plain(e, x):
    lst = x.compress_switched()
    return e.host(x.export(), lst, "standard").serialize()


def test_rekey_install_refusals():
    a = env(16, CLASSIC)
    p = product_params(15)
    p.glwe_noise_log2 = 16  # one of the shared fields a key generation lets differ
    c4, _ = generate_keys(p, seed=KEY_SEED)
    d4, _ = generate_keys(p, seed=KEY_SEED + 1)
    with pytest.raises(FheError, match="glwe_noise_log2"):
        a.ctx.set_rekey_key(RekeyKey.new(c4, d4, RK_SEED))
    bare = Context(0)
    try:
        with pytest.raises(FheError) as err:
            bare.set_rekey_key(RekeyKey.new(a.ck, env(15, CLASSIC).ck, RK_SEED))
        assert err.value.code == -3
    finally:
        bare.close()
        a.use()
