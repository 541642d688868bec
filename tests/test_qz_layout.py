"""k_blind_rotate_qz's layouts on the CPU (tools/qz_emulate.py, a transcription of the kernel's data
movement): the LDS map, the two exchanges, the table indices against the oracle's transforms, and the
bank-conflict score DESIGN.md 5 states, for the constants committed in br_qy.hip."""
import os
import re
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import qz_emulate as Q  # noqa: E402


def test_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "fhe-sign_amd", "csrc", "br_qy.hip")).read()
    for name, want in (("ZW", Q.ZW), ("ZA", Q.ZA), ("ZB", Q.ZB), ("QE", Q.QE)):
        m = re.search(r"constexpr int %s\[\d+\] = \{([^}]*)\}" % name, src)
        assert m and [int(v) for v in m.group(1).split(",")] == list(want), name
    assert (Q.QW1, Q.QW0) == (2, 3) and "constexpr int QW1 = 2, QW0 = 3;" in src


def test_map_is_injective_and_fits_the_region():
    pos = np.array([Q.zq(i) for i in range(1024)])
    assert len(np.unique(pos)) == 1024
    assert pos.max() == Q.ZR_SZ - 1 < Q.REGION_BOUND
    # two workgroups per CU: 2 x (four regions + the zeta and twiddle tables), 16 bytes an entry
    assert 2 * 16 * (4 * Q.ZR_SZ + 16 * 9 + 4 * 9) <= 160 * 1024


def test_exchanges_are_bijections_onto_the_next_phase():
    A, B, E = Q.exchange_maps()
    every = np.arange(1024)
    # one wave holds a whole polynomial in A and in B, each index in exactly one (lane, register)
    assert np.array_equal(np.sort(A.ravel()), every) and np.array_equal(np.sort(B.ravel()), every)
    # the four E waves together hold each polynomial once; (b3, b2) come from the wave, (b1, b0) from the register
    assert np.array_equal(np.sort(E.ravel()), every)
    for e in range(4):
        assert np.all((E[e] >> 2 & 3) == 2 * (e & 1) + (e >> 1))
        assert np.all((E[e] & 3) == np.arange(4))
    # register bits: A holds (b9 b8 b7 b6), B (b5 b4 b3 b2), the rest on lanes
    assert np.all(A >> 6 == np.arange(16)) and np.all((B >> 2 & 15) == np.arange(16))
    # written through one layout and read through the next, every value lands where that phase indexes it
    lds = np.full(Q.ZR_SZ, -1)
    Q.store(lds, 0, Q.idx_zA, [A[:, r] for r in range(16)])
    got = Q.load(lds, 0, Q.idx_zB)
    assert all(np.array_equal(got[r], B[:, r]) for r in range(16))
    for e in range(4):
        for k in range(4):
            assert np.array_equal([lds[Q.zq(Q.idx_E(e, L, k))] for L in range(64)], E[e][:, k])


def test_transforms_agree_with_the_oracle():
    """complex128 against the restated forward_twisted / fft_inverse: the bound is rounding over ten stages
    of growth 2 on unit-variance inputs (qy_emulate.py's)"""
    ferr, ierr = Q.run()
    assert ferr < 1e-9 and ierr < 1e-6


def test_conflict_score_is_the_one_design_states():
    per, mean = Q.conflict_score()
    assert per == {"A": (4.0, 8.0), "B": (4.0, 8.0), "E": (4.0, 8.0)}  # every ds_read_b128 / ds_write_b128 conflict-free
    assert mean == 12.0
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "qz LDS map score 12.00" in design
