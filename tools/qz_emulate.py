#!/usr/bin/env python3
"""CPU emulation of k_blind_rotate_qz's data movement (br_qy.hip; no GPU): the forward transform
phases A -> B -> E and the inverse E -> B -> A of one workgroup (two ciphertexts, one wave per
polynomial in A and B), transcribed from the kernel -- registers, the LDS map zq, both exchanges, the
LDS zeta / twiddle tables and the lane-ordered table of the inverse-A twiddles -- and checked against
the oracle's transforms (oracle/tfhe_oracle.c forward_twisted, fho_fft_inverse, restated in
tools/qy_emulate.py) in numpy complex128.  The constants below are the kernel's; tests/test_qz_layout.py pins both.
usage: python3 tools/qz_emulate.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_layout_qx import RG, WG  # noqa: E402
from qy_emulate import QE, QW0, QW1, W, ZETA, bfly, bt, mul_i, ref_forward, ref_inverse  # noqa: E402

ZW = [2, 16, 1, 4, 32, 8, 276, 550, 136, 71]  # additive weights of index bits b0..b9
ZA = [4, 1, 5, 3, 0, 2]                       # index bits on lane bits 5..0, phase A
ZB = [7, 8, 1, 9, 6, 0]                       # ... phase B
ZR_SZ = sum(ZW) + 1
REGION_BOUND = 1100                            # two workgroups per CU: 2 x (4 regions + tables) <= 160 KiB
NC = 2
Lv = np.arange(64)
ZZ_SZ, ZT_SZ = 16 * 9, 4 * 9                   # the stride-9 tables s_z, s_t
WT_ROWS = 8                                    # rows of the lane-ordered inverse-A twiddle table s_w
ZW_SZ = WT_ROWS * 64
ZL_W = 2 * NC * ZR_SZ + ZZ_SZ + ZT_SZ          # s_w's offset in complex entries: behind the regions, s_z and s_t
LDS_BYTES = 16 * (ZL_W + ZW_SZ)                # the kernel's whole static LDS


def zq(idx):
    return sum(ZW[k] for k in range(10) if idx >> k & 1)


def idx_zA(L, r):  # r = (b9 b8 b7 b6)
    v = (r & 15) << 6
    for m in range(6):
        v |= bt(L, 5 - m) << ZA[m]
    return v


def idx_zB(L, r):  # r = (b5 b4 b3 b2)
    v = (r & 15) << 2
    for m in range(6):
        v |= bt(L, 5 - m) << ZB[m]
    return v


def idx_E(e, L, k):
    v = (bt(e, 1) << QW1) | (bt(e, 0) << QW0) | (k & 3)
    for m in range(6):
        v |= bt(L, 5 - m) << QE[m]
    return v


def tables():
    """the kernel's LDS tables: forward zetas by U4 = (b9..b6), inverse twiddles by m2 = (b1 b0), stride 9"""
    s_z, s_t = np.zeros(16 * 9, complex), np.zeros(4 * 9, complex)
    for t in range(128):
        U4, k = t >> 3, t & 7
        zi = 16 + U4 if k == 0 else 32 + 2 * U4 if k == 1 else 64 + 4 * U4 + 2 * (k - 2) if k < 4 else 128 + 8 * U4 + 2 * (k - 4)
        s_z[9 * U4 + k] = ZETA[zi]
    for t in range(32):
        m, k = t >> 3, t & 7
        wi = 128 * m if k == 0 else 64 * m if k == 1 else 32 * m + 128 * (k - 2) if k < 4 else 16 * m + 64 * (k - 4)
        s_t[9 * m + k] = W[wi]
    return s_z, s_t


def w_index(k, v):
    """the W index row k of s_w holds for the lane whose A index is v: what the CMUX loop loaded from global
    memory every step before the table existed (W[8 v], W[4 v], W[2 v + 128 j], W[v + 64 j])"""
    return 8 * v if k == 0 else 4 * v if k == 1 else 2 * v + 128 * (k - 2) if k < 4 else v + 64 * (k - 4)


def lane_twiddle_indices():
    """the prologue's fill of s_w as W indices: thread t = 64 w + L writes entries 64 k + L of rows
    k = 2 w, 2 w + 1 with v = idx_zA(L, 0); -1 where nothing was written"""
    idx = np.full(ZW_SZ, -1)
    for t in range(256):
        w, L = t >> 6, t & 63
        for k in (2 * w, 2 * w + 1):
            idx[64 * k + L] = w_index(k, idx_zA(L, 0))
    return idx


def lane_twiddle_read(k, L):
    """the entry of s_w the CMUX loop reads for row k in lane L"""
    return 64 * k + L


def pairs16(X, K, tw):
    for r in range(16):
        if not r >> K & 1:
            bfly(X, r, r | 1 << K, tw(r))


def sel_i(base, flag):
    return mul_i(base) if flag else base


def store(lds, region, base_idx, X):
    """X[r][L] -> lds[region][zq(base_idx(L, r))]; every position written exactly once per call"""
    for r in range(16):
        for L in range(64):
            lds[region * ZR_SZ + zq(base_idx(L, r))] = X[r][L]


def load(lds, region, base_idx):
    return [np.array([lds[region * ZR_SZ + zq(base_idx(L, r))] for L in range(64)]) for r in range(16)]


def forward_AB(X, lds, w):
    """phases A and B of wave w = 2 c + p on x[16][64] in the A layout; leaves the B layout in region w"""
    s_z, _ = tables()
    pairs16(X, 3, lambda r: ZETA[1])
    pairs16(X, 2, lambda r: sel_i(ZETA[2], r >> 3))
    pairs16(X, 1, lambda r: sel_i(ZETA[4 + 2 * (r >> 3)], r >> 2 & 1))
    pairs16(X, 0, lambda r: sel_i(ZETA[8 + 2 * (r >> 2)], r >> 1 & 1))
    store(lds, w, idx_zA, X)
    X[:] = load(lds, w, idx_zB)
    U4 = np.array([idx_zB(L, 0) >> 6 for L in range(64)])
    zt = [s_z[9 * U4 + k] for k in range(8)]
    pairs16(X, 3, lambda r: zt[0])
    pairs16(X, 2, lambda r: sel_i(zt[1], r >> 3))
    pairs16(X, 1, lambda r: sel_i(zt[2 + (r >> 3)], r >> 2 & 1))
    pairs16(X, 0, lambda r: sel_i(zt[4 + (r >> 2)], r >> 1 & 1))
    store(lds, w, idx_zB, X)


def phase_E_forward(lds, e, c):
    """wave e's 8 registers (poly, b1, b0) of ciphertext c after stages 8, 9"""
    ie = np.array([idx_E(e, L, 0) for L in range(64)])
    V = ie >> 2
    z8, z9 = ZETA[256 + V], ZETA[512 + 2 * V]
    Y = [np.array([lds[(2 * c + (r >> 2)) * ZR_SZ + zq(idx_E(e, L, r & 3))] for L in range(64)]) for r in range(8)]
    for r in range(8):
        if not r & 2:
            bfly(Y, r, r + 2, z8)
    for r in range(0, 8, 2):
        bfly(Y, r, r + 1, mul_i(z9) if r & 2 else z9)
    return Y


def phase_E_inverse(lds, e, c, Y):
    for r in range(0, 8, 2):
        a0, c0 = Y[r].copy(), Y[r + 1].copy()
        Y[r], Y[r + 1] = a0 + c0, a0 - c0
    for r in range(8):
        if r & 2:
            continue
        t = -1j * Y[r + 2] if r & 1 else Y[r + 2]
        a = Y[r].copy()
        Y[r], Y[r + 2] = a + t, a - t
    for r in range(8):
        for L in range(64):
            lds[(2 * c + (r >> 2)) * ZR_SZ + zq(idx_E(e, L, r & 3))] = Y[r][L]


def inverse_BA(lds, w):
    """phases B and A (inverse) of wave w; returns x[16][64] in the A layout"""
    _, s_t = tables()
    X = load(lds, w, idx_zB)
    m2 = np.array([idx_zB(L, 0) & 3 for L in range(64)])
    tt = [s_t[9 * m2 + k] for k in range(8)]
    pairs16(X, 0, lambda r: np.conj(tt[0]))
    pairs16(X, 1, lambda r: np.conj(sel_i(tt[1], r & 1)))
    pairs16(X, 2, lambda r: np.conj(sel_i(tt[2 + (r & 1)], r & 2)))
    pairs16(X, 3, lambda r: np.conj(sel_i(tt[4 + (r & 3)], r & 4)))
    store(lds, w, idx_zB, X)
    X = load(lds, w, idx_zA)
    s_w = W[lane_twiddle_indices()]
    wl = [s_w[lane_twiddle_read(k, Lv)] for k in range(WT_ROWS)]
    w6, w7 = wl[0], wl[1]
    w8 = [wl[2], wl[3]]
    w9 = [wl[4 + j] for j in range(4)]
    pairs16(X, 0, lambda r: np.conj(w6))
    pairs16(X, 1, lambda r: np.conj(sel_i(w7, r & 1)))
    pairs16(X, 2, lambda r: np.conj(sel_i(w8[r & 1], r & 2)))
    pairs16(X, 3, lambda r: np.conj(sel_i(w9[r & 3], r & 4)))
    return X


def a_layout(poly):
    return [np.array([poly[idx_zA(L, r)] for L in range(64)]) for r in range(16)]


def run(seed=5):
    """one workgroup's transforms; returns (forward error, inverse error) against the oracle restatement"""
    rng = np.random.default_rng(seed)
    poly = [rng.standard_normal(1024) + 1j * rng.standard_normal(1024) for _ in range(2 * NC)]  # [2 c + p]
    lds = np.full(2 * NC * ZR_SZ, np.nan + 0j)
    for w in range(4):
        forward_AB(a_layout(poly[w]), lds, w)
    ref = [ref_forward(q) for q in poly]
    ferr, E = 0.0, {}
    for e in range(4):
        for c in range(NC):
            Y = phase_E_forward(lds, e, c)
            for r in range(8):
                want = np.array([ref[2 * c + (r >> 2)][idx_E(e, L, r & 3)] for L in range(64)])
                ferr = max(ferr, np.abs(Y[r] - want).max())
            E[e, c] = Y
    inv_ref = [ref_inverse(q) for q in ref]
    lds[:] = np.nan
    for (e, c), Y in E.items():
        phase_E_inverse(lds, e, c, Y)
    ierr = 0.0
    for w in range(4):
        X = inverse_BA(lds, w)
        for r in range(16):
            want = np.array([inv_ref[w][idx_zA(L, r)] for L in range(64)])
            ierr = max(ierr, np.abs(X[r] - want).max())
    return ferr, ierr


def exchange_maps():
    """the index every (wave, lane, register) holds in each layout: A [4][64][16] and B [4][64][16] are per
    polynomial region w; E [4 waves][64][8 = (poly, b1, b0)] per ciphertext"""
    A = np.array([[idx_zA(L, r) for r in range(16)] for L in range(64)])
    B = np.array([[idx_zB(L, r) for r in range(16)] for L in range(64)])
    E = np.array([[[idx_E(e, L, k) for k in range(4)] for L in range(64)] for e in range(4)])
    return A, B, E


def conflict_score():
    """array cycles per LDS instruction as tools/lds_layout_qx.py scores them (ds_read_b128: four 16-lane
    groups over pos mod 16; ds_write_b128: eight 8-lane groups over pos mod 8), per layout:
    {layout: (read, write)} with 4 / 8 conflict-free, and the mean of read + write over the three"""
    A, B, E = exchange_maps()
    rows = {"A": A.T, "B": B.T, "E": E.transpose(0, 2, 1).reshape(16, 64)}
    out = {}
    for name, idx in rows.items():
        pos = np.vectorize(zq)(idx)
        rd = sum(np.array([[np.bincount(p[g] % 16, minlength=16).max() for g in RG] for p in pos]).sum(1)) / len(pos)
        wr = sum(np.array([[np.bincount(p[g] % 8, minlength=8).max() for g in WG] for p in pos]).sum(1)) / len(pos)
        out[name] = (float(rd), float(wr))
    return out, sum(a + b for a, b in out.values()) / 3.0


def twiddle_table_conflicts():
    """extra LDS-array cycles of the eight ds_read_b128 of s_w (0: conflict-free), over the four 16-lane groups"""
    extra = 0
    for k in range(WT_ROWS):
        pos = np.array([ZL_W + lane_twiddle_read(k, L) for L in range(64)])
        extra += sum(int(np.bincount(pos[g] % 16, minlength=16).max()) - 1 for g in RG)
    return extra


def main():
    ferr, ierr = run()
    print(f"forward: max |kernel layout - oracle forward_twisted| = {ferr:.3e}")
    print(f"inverse: max |kernel layout - oracle fft_inverse| = {ierr:.3e}")
    assert ferr < 1e-9 and ierr < 1e-6
    per, mean = conflict_score()
    print(f"LDS array cycles per instruction (read, write; 4 / 8 conflict-free): {per}; mean read + write {mean:.2f}")
    assert twiddle_table_conflicts() == 0 and 2 * LDS_BYTES <= 160 * 1024
    print(f"inverse-A twiddle table: {ZW_SZ} entries at {ZL_W}, conflict-free; LDS {LDS_BYTES} B a workgroup")
    print("qz layouts OK")


if __name__ == "__main__":
    main()
