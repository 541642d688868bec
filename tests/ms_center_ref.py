"""Test-only numpy restatement of the centered modulus switch (include/fhe_rocm.h), in wrapping
uint64 / int64 arithmetic.  For a keyswitched small LWE row a[0 .. n-1], b = a[n]:

    res(x) = (int64)((x + 2^51) & (2^52 - 1)) - 2^51      the signed distance of x from the multiple of 2^52
                                                          that modswitch_2n / fho_modswitch rounds it to
    S      = sum_{i < n} res(a[i])                        int64; |S| <= n 2^51 <= 2^62 for n <= 2048
    b'     = b - (uint64)(S >> 1)                         arithmetic shift (floor), wrapping mod 2^64

Mask words and whatever follows the body in a row are unchanged.  Never used by the product."""
import numpy as np

HALF = np.uint64(1 << 51)
MASK = np.uint64((1 << 52) - 1)


def res(x):
    """int64 residues of uint64 words, in [-2^51, 2^51)"""
    x = np.asarray(x, np.uint64)
    return ((x + HALF) & MASK).astype(np.int64) - np.int64(1 << 51)


def center_ref(rows, n=None):
    """a centered copy of (count, >= n + 1) rows; n defaults to the row width - 1"""
    rows = np.array(rows, dtype=np.uint64, ndmin=2)
    n = rows.shape[1] - 1 if n is None else n
    S = res(rows[:, :n]).sum(axis=1, dtype=np.int64)
    rows[:, n] -= (S >> np.int64(1)).astype(np.uint64)
    return rows


def center_ref_int(row, n):
    """the same on one row in Python integers: a check of the numpy arithmetic itself"""
    row = [int(v) for v in row]
    S = sum(((x + (1 << 51)) % (1 << 52)) - (1 << 51) for x in row[:n])
    row[n] = (row[n] - (S >> 1)) % (1 << 64)
    return row


def ms_error(rows, key, centered):
    """the exact modulus-switch error of every row under the binary `key`, in units of 2^52 (float64): the
    phase of the switched row minus the phase of the 64-bit row.  Standard: (sum res(a_i) s_i - res(b)) / 2^52;
    centered: (sum res(a_i) s_i - (S >> 1) - res(b')) / 2^52 with b' = b - (S >> 1)."""
    rows = np.asarray(rows, np.uint64)
    n = key.size
    r = res(rows[:, :n])
    rs = (r * key.astype(np.int64)[None, :]).sum(axis=1, dtype=np.int64)
    if not centered:
        return (rs - res(rows[:, n])) / float(1 << 52)
    half = r.sum(axis=1, dtype=np.int64) >> np.int64(1)
    return (rs - half - res(rows[:, n] - half.astype(np.uint64))) / float(1 << 52)


def sigma_standard(hw):
    return (hw / 12 + 1 / 12) ** 0.5


def sigma_centered(n):
    return (n / 48 + 1 / 12) ** 0.5
