"""The centered modulus switch on the host (CPU): fhe_ms_center_host, the word-for-word definition of
k_ms_center (ms_center.hip), against the numpy restatement tests/ms_center_ref.py; the extremes of the sum; and
the statistics the feature exists for -- the exact modulus-switch error of random rows under a random binary key
has standard deviation sqrt(hw / 12 + 1 / 12) grid steps as the keyswitch leaves them and sqrt(n / 48 + 1 / 12)
after centering.  Deterministic: every input comes from a seeded numpy generator."""
import ctypes as C

import numpy as np
import pytest

import ms_center_ref as M
from fhe_sign import FheError, _lib, ms_center_host, ms_stride
from fhe_sign.core import MS_PAD_WORD, modulus_switch_mode

DIMS = (1, 2, 63, 64, 65, 834, 2048)
COUNTS = (1, 3, 4, 5)
U64 = (1 << 64) - 1


def _rows(n, count, seed=0):
    rng = np.random.default_rng(0x5EED + 4099 * n + count + seed)
    return rng.integers(0, 1 << 64, (count, n + 1), dtype=np.uint64)


def check_layout(got, rows, ref, n, what):
    """`got` (count, stride): the reference's body, the input's mask words, the padding marker"""
    assert got.shape[0] == rows.shape[0] and got.shape[1] >= n + 1, what
    assert np.array_equal(got[:, :n], rows[:, :n]), f"{what}: a mask word changed"
    bad = np.flatnonzero(got[:, n] != ref[:, n])
    assert bad.size == 0, f"{what}: {bad.size} bodies differ, first row {bad[:5]}"
    assert (got[:, n + 1:] == np.uint64(MS_PAD_WORD)).all(), f"{what}: a padding word changed"


def test_reference_against_python_integers():
    for n in (1, 2, 65, 834):
        rows = _rows(n, 3, seed=7)
        ref = M.center_ref(rows)
        for r in range(3):
            assert [int(v) for v in ref[r]] == M.center_ref_int(rows[r], n)
    assert M.res(np.array([0, 1 << 51, (1 << 51) - 1, 1 << 52, U64], np.uint64)).tolist() == \
        [0, -(1 << 51), (1 << 51) - 1, 0, -1]


@pytest.mark.parametrize("n", DIMS)
def test_host_equals_reference(n):
    for count in COUNTS:
        rows = _rows(n, count)
        ref = M.center_ref(rows)
        assert not np.array_equal(ref[:, n], rows[:, n])
        for stride in (n + 1, ms_stride(n)):
            got = ms_center_host(rows, stride)
            assert got.shape == (count, stride)
            check_layout(got, rows, ref, n, f"n {n}, {count} rows, stride {stride}")
        assert np.array_equal(ms_center_host(rows), ref)


def extreme_rows():
    """n = 2048: (name, rows) with the expected body spelled out where it is a closed form"""
    n = 2048
    rng = np.random.default_rng(0xE87)
    body = rng.integers(0, 1 << 64, 4, dtype=np.uint64)
    lo = np.full((4, n + 1), 1 << 51, np.uint64)        # res = -2^51 everywhere: S = -2^62
    hi = np.full((4, n + 1), (1 << 51) - 1, np.uint64)  # res = 2^51 - 1: S = 2048 (2^51 - 1)
    grid = rng.integers(0, 1 << 12, (4, n + 1), dtype=np.uint64) << np.uint64(52)  # multiples of 2^52: res = 0
    odd = grid.copy()                                   # S = -1, -3, -5, -7: floor, not truncation
    for r in range(4):
        odd[r, 5:5 + 2 * r + 1] -= np.uint64(1)
    for a in (lo, hi, grid, odd):
        a[:, n] = body
    return n, body, {"lo": lo, "hi": hi, "grid": grid, "odd": odd}


def check_extremes(run):
    """`run(rows)` -> centered (count, n + 1) rows; shared with the GPU test"""
    n, body, sets = extreme_rows()
    exp = {"lo": [(int(b) + (1 << 61)) & U64 for b in body],
           "hi": [(int(b) - 1024 * ((1 << 51) - 1)) & U64 for b in body],
           "grid": [int(b) for b in body],
           "odd": [(int(b) + r + 1) & U64 for r, b in enumerate(body)]}  # -(S >> 1) = -floor(-(2r+1)/2) = r + 1
    for name, rows in sets.items():
        got = run(rows)
        assert np.array_equal(got, M.center_ref(rows)), name
        assert np.array_equal(got[:, :n], rows[:, :n]), name
        assert [int(v) for v in got[:, n]] == exp[name], name
    assert np.array_equal(run(sets["grid"]), sets["grid"])


def test_extremes():
    check_extremes(ms_center_host)


@pytest.mark.parametrize("n", (16, 255, 834, 2048))
def test_error_statistics(n):
    rng = np.random.default_rng(0xC3A7 + n)
    rows = rng.integers(0, 1 << 64, (16384, n + 1), dtype=np.uint64)
    key = rng.integers(0, 2, n, dtype=np.uint64)
    hw = int(key.sum())
    centered = ms_center_host(rows)
    assert np.array_equal(centered, M.center_ref(rows))
    # the two descriptions of the centered error agree: the formula on the input rows, and the standard
    # formula plus the body's shift on the centered rows
    shift = (rows[:, n] - centered[:, n]).astype(np.int64)
    e_std = M.ms_error(rows, key, centered=False)
    e_cen = M.ms_error(rows, key, centered=True)
    assert np.allclose(M.ms_error(centered, key, centered=False) - shift / float(1 << 52), e_cen, rtol=0, atol=1e-9)
    s_std, s_cen = float(e_std.std()), float(e_cen.std())
    print(f"n {n} hw {hw}: standard sigma {s_std:.4f} (formula {M.sigma_standard(hw):.4f}), "
          f"centered sigma {s_cen:.4f} (formula {M.sigma_centered(n):.4f})")
    assert abs(s_std / M.sigma_standard(hw) - 1) < 0.04
    assert abs(s_cen / M.sigma_centered(n) - 1) < 0.04
    assert abs(float(e_cen.mean())) < 5 * M.sigma_centered(n) / 128  # no bias left: 5 sigma of the mean


def test_invalid_arguments():
    lib = _lib.load()
    buf = np.zeros(4100, np.uint64)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.fhe_ms_center_host(p, 1, 0, 8) == -1
    assert lib.fhe_ms_center_host(p, 1, 2049, 2056) == -1
    assert b"2048" in lib.fhe_last_error()
    assert lib.fhe_ms_center_host(p, 1, 16, 16) == -1
    assert b"stride" in lib.fhe_last_error()
    assert lib.fhe_ms_center_host(None, 1, 16, 17) == -1
    assert lib.fhe_ms_center_host(None, 0, 16, 17) == 0
    assert not buf.any()
    with pytest.raises(ValueError):
        ms_center_host(np.zeros((2, 5), np.uint64), stride=4)


def test_unknown_mode_is_invalid():
    """the name check of Context.set_modulus_switch and the library's entry points without a context (the mode
    of a live context, its default and the library's own refusal of an unknown value: test_ms_center_gpu.py)"""
    assert modulus_switch_mode("standard") == 0 and modulus_switch_mode("centered") == 1
    with pytest.raises(FheError) as e:
        modulus_switch_mode("central")
    assert e.value.code == -1 and "central" in str(e.value)
    lib = _lib.load()
    m = C.c_int(7)
    assert lib.fhe_ctx_set_modulus_switch(None, 1) == -1
    assert lib.fhe_ctx_get_modulus_switch(None, C.byref(m)) == -1 and m.value == 7
