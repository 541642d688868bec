"""Every raw entry point at message spaces other than 4 x 4, and the radix layer's refusal of them.

Params::from_c admits any message_modulus in {2 .. 64} and carry_modulus in {1 .. 64}, powers of two, with product
mc <= 64; keys.h, make_lut_poly, register_lut, decode_block, the OPRF accumulator and the client-key kernels are
written for a general mc, and every other GPU file runs 4 x 4 (mc 16, delta 2^59, a box of 2048 / 16 = 128
accumulator coefficients per value).  The spaces of tests/msg_spaces.py reach what 4 x 4 does not:

    space          mc   box    reaches
    2x1            2    1024   the widest box, half-box 512; one OPRF bit
    2x2            4    512    tfhe-rs' 1_1
    4x2            8    256
    2x8 8x2 16x1   16   128    delta as 4 x 4: LUT ids survive a re-key from 4 x 4; 1 / 3 / 4 OPRF bits
    4x8            32   64     tables above the radix layer's 16 entries
    8x8 64x1       64   32     the narrowest box, half-box 16; 64-entry tables; 6 OPRF bits

The blind-rotation kernels never see mc -- it enters through the accumulator polynomial, delta and the host-side
checks -- so one ragged batch per kernel path suffices; what is pinned per space is the polynomial (box width,
half-box rotation, sign), the registry, the OPRF staircase, the client-key kernels' scaling and the door of the radix
layer.  All comparisons are exact equality of 64-bit words against the oracle (oracle/tfhe_oracle.c).

Keys are n = 16 for every space and n = 834 for 2x2 and 8x8.  At n = 834 the decode is asserted for mc <= 16 only:
at mc = 64 the half-box is 16 grid steps of the 2N = 4096 grid against the modulus switch's sigma of about 6 steps
(DESIGN.md 6g), a margin of 2.7 sigma, so wrong decodes are expected there -- the reference decodes the same wrong
values, and the words still have to be equal.
"""
import csv
import os

import numpy as np
import pytest

import ks_ref
import oprf_ref as O
import oracle
from fhe_sign import (COMPAT, LUT_INTEGER, BigUintFHE, ClientKey, CompactCiphertextList, CompactPublicKey, CompressedFheUint32,
                      Context, FheError, FheUint32, Schnorr, compute_nonce, generate_keys, lut_table, pending_info,
                      set_server_key)
from msg_spaces import (CLASSIC, DEFAULT, MULTIBIT, SPACES, box_of, delta_of, mc_of, oprf_max_bits, oracle_params, product_params,
                        space_id, tables)
from test_keyswitch_gpu import _assert_words
from test_oprf_gpu import oracle_blocks

pytestmark = pytest.mark.gpu
SEED = 0x5ACE5
OPRF_SEED = bytes(range(7, 39))
MASK_SEED = bytes(range(40, 72))
M64 = (1 << 64) - 1
FHE_ERR_INVALID = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_made = {}


def _keys(space, n=16, g=CLASSIC):
    """(client key bytes, server key, oracle keys), made once per (space, n, grouping)"""
    k = (space, n, g)
    if k not in _made:
        ck, sk = generate_keys(product_params(space, n, g), seed=SEED)
        _made[k] = (ck.serialize(), sk, oracle.OracleKeys(SEED, oracle_params(space, n, g)))
    return _made[k]


def _ck(space, n=16, g=CLASSIC):
    """a fresh copy of the space's client key, its encryption stream re-seeded"""
    ck = ClientKey.deserialize(_keys(space, n, g)[0])
    ck.seed_encryption(42, 100)
    return ck


@pytest.fixture(scope="module", autouse=True)
def _drop_keys():
    yield
    set_server_key(None)
    _made.clear()


class Env:
    def __init__(self, space, n=16, g=CLASSIC):
        self.space, self.n, self.g = space, n, g
        self.mc, self.delta = mc_of(space), delta_of(space)
        _, self.sk, self.ok = _keys(space, n, g)
        self.ctx = Context(0)
        self.ctx.set_server_key(self.sk)

    def ck(self):
        return _ck(self.space, self.n, self.g)


@pytest.fixture(scope="module", params=list(SPACES), ids=space_id)
def env(request):
    """oracle keys and a context with the key installed, one per space, n = 16 classic"""
    e = Env(request.param)
    yield e
    e.ctx.close()


def _refused(call, word="message_modulus"):
    with pytest.raises(FheError, match=word) as e:
        call()
    assert e.value.code == FHE_ERR_INVALID


# ---------------------------------------------------------------- raw PBS
def _pbs_case(ok, mc):
    """37 encryptions (ragged, odd) of (5 i + 3) % mc -- every value where mc <= 32 -- through table i % 4"""
    tabs = tables(mc)
    r = ok.rng(777)
    msgs = [(5 * i + 3) % mc for i in range(37)]
    cts = np.stack([ok.encrypt(r, m) for m in msgs])
    lut_of = np.arange(37, dtype=np.uint32) % len(tabs)
    ref = ok.pbs_batch(cts, np.stack([ok.make_lut(t) for t in tabs]), lut_of)
    want = [tabs[int(lut_of[i])][m] for i, m in enumerate(msgs)]
    return tabs, cts, lut_of, ref, want


def _paths(g):
    """(name, wide threshold, blind-rotate kind): the latency kernel and the throughput selection"""
    return [("latency", 1 << 30, 7), ("qy", 0, 4)] + ([("qz", 0, 9)] if g == CLASSIC else [])


def _check_pbs(e, decode):
    tabs, cts, lut_of, ref, want = _pbs_case(e.ok, e.mc)
    ref_decodes = [e.ok.decrypt(o) for o in ref]
    if decode:
        assert ref_decodes == want  # the reference itself computes f(m) here
    ids = np.array([e.ctx.lut(t) for t in tabs], np.uint32)
    assert len(set(ids.tolist())) == (len(tabs) if e.mc > 2 else 3)  # mc 2: the affine map (3 m + 1) % 2 is the reversal
    what = f"{space_id(e.space)} n {e.n} g {e.g}"
    try:
        for name, threshold, kind in _paths(e.g):
            e.ctx.set_wide_threshold(threshold)
            e.ctx.set_br_kernel(kind)
            for b in (37, 1):
                out = e.ctx.pbs(cts[:b], ids[lut_of[:b]])
                _assert_words(out, ref[:b], f"{what}: {name}, batch of {b}")
                assert [e.ok.decrypt(o) for o in out] == (want[:b] if decode else ref_decodes[:b])
    finally:
        e.ctx.set_wide_threshold(256)
        e.ctx.set_br_kernel(7)


def test_pbs_words_every_path(env):
    _check_pbs(env, decode=True)


@pytest.mark.parametrize("space,n,g", [((2, 2), 16, MULTIBIT), ((8, 8), 16, MULTIBIT), ((2, 2), 834, CLASSIC), ((8, 8), 834, CLASSIC)],
                         ids=lambda v: space_id(v) if isinstance(v, tuple) else str(v))
def test_pbs_words_multibit_and_production_depth(space, n, g):
    """multi-bit at n = 16, classic at n = 834.  At n = 834 and mc = 64 only the words are asserted (the module's
    docstring: a half-box of 16 grid steps against sigma 6)"""
    e = Env(space, n, g)
    try:
        _check_pbs(e, decode=(n == 16 or e.mc <= 16))
    finally:
        e.ctx.close()


# ---------------------------------------------------------------- box edges, deterministic
def _edge_rows(space, far):
    """trivial rows (zero mask): body = m delta + k 2^52 for every m and k in {-box / 2, -1, 0, box / 2 - 1}, the
    first and the last grid step of m's box and the two around its centre; far: 2^63 added (the negacyclic half)"""
    mc, box, delta = mc_of(space), box_of(space), delta_of(space)
    ks = (-(box // 2), -1, 0, box // 2 - 1)
    rows = np.zeros((mc * len(ks), 2049), np.uint64)
    for m in range(mc):
        for j, k in enumerate(ks):
            rows[m * len(ks) + j, 2048] = np.uint64((m * delta + k * (1 << 52) + (1 << 63 if far else 0)) & M64)
    return rows, [m for m in range(mc) for _ in ks]


def test_box_edges(env):
    """pins make_lut_poly's box width, half-box rotation and the sign of the wrapped half-box at boxes of 1024 .. 32
    coefficients: an off-by-one in `box` or `half` moves an edge row into the neighbouring value, which the
    128-coefficient box of 4 x 4 alone cannot tell from a shifted table.  A trivial row's mask is zero, so the
    bootstrap's output is the accumulator's coefficient itself: the phase is table[m] delta exactly, and its negation
    on the far half."""
    e = env
    ck = e.ck()
    tabs = tables(e.mc)
    near, ms = _edge_rows(e.space, False)
    far, _ = _edge_rows(e.space, True)
    rows = np.concatenate([near, far])
    for t in (tabs[1], tabs[3]):
        lid = e.ctx.lut(t)
        ref = e.ok.pbs_batch(rows, e.ok.make_lut(t)[None, :], np.zeros(len(rows), np.uint32))
        out = e.ctx.pbs(rows, lid)
        _assert_words(out, ref, f"{space_id(e.space)}: box edges through {t[:4]}..")
        ph = [int(p) for p in ck.decrypt_phase_host(out)]
        half = len(near)
        assert [((p + e.delta // 2) // e.delta) % e.mc for p in ph[:half]] == [t[m] for m in ms]
        assert ph[:half] == [t[m] * e.delta for m in ms]
        assert ph[half:] == [(-p) & M64 for p in ph[:half]]


# ---------------------------------------------------------------- the LUT registry
def test_lut_registry(env):
    e = env
    mc = e.mc
    for bad in sorted({2, 4, 16, 64, mc - 1, mc + 1} - {mc}):
        _refused(lambda: e.ctx.lut(list(range(bad))), "message_modulus")
    t = tables(mc)[1]
    lid = e.ctx.lut(t)
    assert e.ctx.lut([v + mc for v in t]) == lid == e.ctx.lut([v + 5 * mc for v in t])  # congruent mod mc: one id
    assert e.ctx.lut([(v + 1) % mc for v in t]) != lid
    # the table read-back hook: the radix layer's 16 entries; a larger table is refused by name, not misreported
    if mc <= 16:
        kind, entries = lut_table(e.ctx, lid)
        assert kind == LUT_INTEGER and list(entries[:mc]) == t and not any(entries[mc:])
    else:
        _refused(lambda: lut_table(e.ctx, lid), "at most 16")


def test_lut_length_refusals_of_the_issue():
    """16 entries under 2 x 2, 4 under 4 x 4, 64 under 4 x 8"""
    for space, length in (((2, 2), 16), (DEFAULT, 4), ((4, 8), 64)):
        e = Env(space)
        try:
            _refused(lambda: e.ctx.lut(list(range(length))), "message_modulus")
            assert e.ctx.lut(list(range(mc_of(space)))) == 0  # the refusal registered nothing
        finally:
            e.ctx.close()


# ---------------------------------------------------------------- pbs_lincomb
@pytest.mark.parametrize("space", [(2, 2), (8, 8)], ids=space_id)
def test_lincomb_words(space):
    """five items 2 a + b + c + cst delta over a pool of 9 encryptions: the keyswitched words and the bootstrapped
    words equal ks_ref.lincomb_np followed by the oracle, on both keyswitch kernels; where the combination, taken
    mod 2 mc, stays below mc it decodes to table[value] (item 3 lands in the padding bit's half: words only;
    item 4's constant wraps once around the torus)"""
    e = Env(space)
    try:
        mc = e.mc
        r = e.ok.rng(31)
        u = max(mc // 8, 1)
        vals = [(i // 2) % 2 * u for i in range(9)]  # the items' sums 2 a + b + c: u, u, 3 u, 3 u, u
        pool = np.stack([e.ok.encrypt(r, v) for v in vals])
        csts = [0, 1, 0, mc - 1, 2 * mc - 1]
        items = [([(i, 2), (i + 2, 1), (i + 4, 1)], c * e.delta) for i, c in enumerate(csts)]
        comb = np.stack([ks_ref.lincomb_np(pool, t, c) for t, c in items])
        small_ref = e.ok.keyswitch_batch(comb)
        tabs = tables(mc)
        lut_of = np.arange(5, dtype=np.uint32) % len(tabs)
        out_ref = e.ok.pbs_batch(comb, np.stack([e.ok.make_lut(t) for t in tabs]), lut_of)
        ids = np.array([e.ctx.lut(t) for t in tabs], np.uint32)
        in_range = 0
        for name, kind in (("valu", 0), ("mfma", 1)):
            e.ctx.set_ks_kernel(kind)
            small, out = e.ctx.pbs_lincomb(pool, items, ids[lut_of])
            _assert_words(small, small_ref, f"{space_id(space)}: {name} keyswitch of the combinations")
            _assert_words(out, out_ref, f"{space_id(space)}: bootstraps behind the {name} keyswitch")
            for i, c in enumerate(csts):
                v = (2 * vals[i] + vals[i + 2] + vals[i + 4] + c) % (2 * mc)
                if v < mc:
                    in_range += 1
                    assert e.ok.decrypt(out[i]) == tabs[int(lut_of[i])][v], (name, i)
        assert in_range == 8
    finally:
        e.ctx.set_ks_kernel(1)
        e.ctx.close()


# ---------------------------------------------------------------- OPRF through the staircase
@pytest.mark.parametrize("space", [(2, 1), (8, 2), (16, 1), (64, 1), (8, 8)], ids=space_id)
def test_oprf_blocks(space):
    """bits the default space never runs (message_modulus 4 caps them at 2): 1 and oprf_max_bits of each space, 65
    blocks (the latency kernel's ragged batch): words == the oracle's blind rotation of the reference rows through
    the reference staircase, decode == the prediction from the small secret, exactly; one bit more is refused"""
    e = Env(space)
    try:
        lwe_sk = e.ok.lwe_sk
        top = oprf_max_bits(space)
        rows = O.rows(OPRF_SEED, e.n, 65)
        for bits in sorted({1, top}):
            got = e.ctx.oprf_blocks(OPRF_SEED, 65, bits)
            want = oracle_blocks(e.ok, rows, O.lut(bits, e.delta), O.body_const(bits, e.delta))
            _assert_words(got, want, f"{space_id(space)}: {bits}-bit OPRF blocks")
            assert [e.ok.decrypt(b) for b in got] == [int(v) for v in O.values(rows, lwe_sk, bits)]
        for bits in (0, top + 1):
            _refused(lambda: e.ctx.oprf_blocks(OPRF_SEED, 65, bits), "bits")
    finally:
        e.ctx.close()


# ---------------------------------------------------------------- the resident client key
@pytest.mark.parametrize("space", [(2, 2), (8, 8)], ids=space_id)
def test_resident_client_key(space):
    """client_ops.hip scales a value by the key's own delta: every value of the space, twice over, encrypted on the
    device == the host's indexed restatement; the phases of those rows and of their bootstraps == the host's; both
    twins' streams end at one position"""
    e = Env(space)
    try:
        ka, kb = e.ck(), e.ck()
        e.ctx.set_client_key(ka)
        assert e.ctx.client_ops_info()[0]
        values = np.arange(2 * e.mc + 1, dtype=np.uint64) % e.mc
        got = e.ctx.client_encrypt_rows(ka, values)
        _assert_words(got, kb.encrypt_rows_indexed_host(values), f"{space_id(space)}: device encryption")
        assert ka.serialize() == kb.serialize()
        _refused(lambda: e.ctx.client_encrypt_rows(ka, [e.mc]), "range")
        assert ka.serialize() == kb.serialize()
        t = tables(e.mc)[1]
        boots = e.ctx.pbs(got, e.ctx.lut(t))
        for cts in (got, boots):
            assert np.array_equal(e.ctx.client_phase_rows(cts), kb.decrypt_phase_host(cts))
        assert [kb.decrypt_block(c) for c in got] == [int(v) for v in values]
        assert [kb.decrypt_block(c) for c in boots] == [t[int(v)] for v in values]
    finally:
        e.ctx.close()


# ---------------------------------------------------------------- re-keying one context across spaces
def _raw_check(ctx, ok, ids, tabs, what):
    """12 bootstraps through the given ids == the oracle's words under `ok` and decode to the tables' values"""
    mc = ok.params.message_modulus * ok.params.carry_modulus
    r = ok.rng(99)
    msgs = [(3 * i + 1) % mc for i in range(12)]
    cts = np.stack([ok.encrypt(r, m) for m in msgs])
    lut_of = np.arange(12, dtype=np.uint32) % len(tabs)
    want = ok.pbs_batch(cts, np.stack([ok.make_lut(t) for t in tabs]), lut_of)
    out = ctx.pbs(cts, np.asarray(ids, np.uint32)[lut_of])
    _assert_words(out, want, what)
    assert [ok.decrypt(o) for o in out] == [tabs[int(lut_of[i])][m] for i, m in enumerate(msgs)]


def _known_answers(ck):
    x, y = 0xDEADBEEF, 0x12345677
    a, b = FheUint32.try_encrypt(x, ck), FheUint32.try_encrypt(y, ck)
    assert (a + b).decrypt(ck) == (x + y) % 2**32
    assert (a * b).decrypt(ck) == (x * y) % 2**32


def test_rekey_across_spaces():
    """one context through 4 x 4 -> 2 x 8 -> 2 x 2 -> 4 x 4.  2 x 8 has 4 x 4's mc and delta, so the accumulator
    polynomials are the same words and the ids registered under 4 x 4 bootstrap under it (fhe_ctx::adopt_key_params
    compares mc and delta); 2 x 2 drops them; back under 4 x 4 the radix layer computes again"""
    ctx = Context(0)
    try:
        tabs = tables(16)
        _, sk44, ok44 = _keys(DEFAULT)
        ctx.set_server_key(sk44)
        set_server_key(ctx)
        _known_answers(_ck(DEFAULT))
        ids = [ctx.lut(t) for t in tabs]
        _raw_check(ctx, ok44, ids, tabs, "4x4")
        _, sk28, ok28 = _keys((2, 8))
        ctx.set_server_key(sk28)
        _raw_check(ctx, ok28, ids, tabs, "4x4 -> 2x8, the ids of 4x4")
        assert [ctx.lut(t) for t in tabs] == ids
        _refused(lambda: FheUint32.try_encrypt(7, _ck((2, 8))))
        _, sk22, ok22 = _keys((2, 2))
        ctx.set_server_key(sk22)
        cts = np.stack([ok22.encrypt(ok22.rng(5), m) for m in range(4)])
        for lid in ids:
            with pytest.raises(FheError) as e:
                ctx.pbs(cts, lid)
            assert e.value.code == FHE_ERR_INVALID
        tabs4 = tables(4)
        ids4 = [ctx.lut(t) for t in tabs4]
        assert ids4[0] == 0
        _raw_check(ctx, ok22, ids4, tabs4, "2x8 -> 2x2")
        ctx.set_server_key(sk44)
        _known_answers(_ck(DEFAULT))
        ids = [ctx.lut(t) for t in tabs]
        _raw_check(ctx, ok44, ids, tabs, "2x2 -> 4x4")
    finally:
        set_server_key(None)
        ctx.close()


# ---------------------------------------------------------------- the radix layer refuses at the door
ROW0 = next(r for r in csv.DictReader(open(os.path.join(ROOT, "tests", "golden", "bip340_vectors.csv"))) if r["index"] == "0")


@pytest.mark.parametrize("space", [(2, 2), (2, 8), (8, 2), (16, 1), (8, 8)], ids=space_id)
def test_radix_layer_refuses_at_the_door(space):
    """One rule: the radix layer needs message_modulus 4 and carry_modulus 4 (Params::radix_space) -- another split
    of 16 is refused like any other space.  With such a server key installed every way into the layer answers
    FHE_ERR_INVALID naming message_modulus, before anything is encrypted, recorded or launched: nothing is pending,
    the client key's stream has not moved, and a raw bootstrap afterwards gives the oracle's words."""
    d = int(ROW0["secret key"], 16)
    msg, aux = bytes.fromhex(ROW0["message"]), bytes.fromhex(ROW0["aux_rand"])
    k0 = compute_nonce(d, msg, aux)
    ck44 = _ck(DEFAULT)
    _, sk44, _ = _keys(DEFAULT)
    _, sk, ok = _keys(space)
    ck = _ck(space)
    # host objects of the default space (same n): what a client of another key set might send
    pk44 = CompactPublicKey.new(ck44, seed=MASK_SEED)
    clist = CompactCiphertextList.builder(pk44).push(7, 32).build_packed(seed=MASK_SEED)
    seeded = CompressedFheUint32.try_encrypt(7, ck44, seed=MASK_SEED)
    ctx = Context(0)
    try:
        ctx.set_server_key(sk44)
        set_server_key(ctx)
        d_fhe = BigUintFHE.new(d, ck44)  # a handle of this context, from before the re-key
        assert d_fhe.to_biguint(ck44) == d
        ctx.set_server_key(sk)
        stream = ck.serialize()
        signer = Schnorr()
        mc = mc_of(space)
        tabs = tables(mc)
        ids = [ctx.lut(t) for t in tabs]
        doors = {
            "FheUint32.try_encrypt": lambda: FheUint32.try_encrypt(7, ck),
            "FheUint32.encrypt_trivial": lambda: FheUint32.encrypt_trivial(7),
            "FheUint32.random": lambda: FheUint32.random(seed=OPRF_SEED),
            "BigUintFHE.random": lambda: BigUintFHE.random(64, seed=OPRF_SEED),
            "BigUintFHE.new": lambda: BigUintFHE.new(7, ck),
            "CompactCiphertextList.expand": clist.expand,
            "CompressedFheUint.decompress": seeded.decompress,
            "Schnorr.sign_fhe_with_k0": lambda: signer.sign_fhe_with_k0(msg, k0, d, d_fhe, ck, COMPAT),
        }
        for name, call in doors.items():
            _refused(call)
            assert pending_info(ctx) == (0, 0, 0), name
            assert ck.serialize() == stream, name
            _raw_check(ctx, ok, ids, tabs, f"{space_id(space)}: raw bootstraps after {name} was refused")
        del d_fhe
    finally:
        set_server_key(None)
        ctx.close()
