"""Test-only: the input sets, the statistics and the caps that tests/test_exact_pbs.py (oracle against
tests/exact_pbs_ref.py, on the CPU) and tests/test_exact_pbs_gpu.py (kernels against it) share.

Inputs are recipes, not words: a key seed per (n, grouping), an encryption seed, messages i % 16 and the
table i % 3 of TABLES.  The oracle's and the product's keygen and encryption are word-identical under
one seed, so both files bootstrap the same ciphertexts under the same keys and the figures they print
are comparable one to one.

Caps (DESIGN.md 3, table "f64 against exact arithmetic": the measured values and seeds behind every
constant here).  They were measured on the oracle against the exact reference, never on a kernel:
  WORD_CAP        sharp tier, |f64 word - exact word|: 4 x the largest difference the oracle shows on the
                  committed sharp set (two bits: an honest re-association of the transform; more is a
                  change of precision class)
  WORD_CLAIM      the bound tfhe_oracle.c states for one update, 2^46
  RATIO_CAP, DIFF_CAP   multi-step tier, per set: R = rms f64 phase error / rms exact phase error, and
                  the largest |f64 phase - exact phase| in exact sigmas; (largest of three disjoint
                  encryption seeds + their spread) x 1.25
Never used by the product."""
import math

import numpy as np

CLASSIC, MULTIBIT = 1, 2
N = 2048
KEY_SEED = 0xE5AC7
SEEDS = (0x5EED1, 0x5EED2, 0x5EED3)  # disjoint encryption streams; the committed tests run the first
TABLES = ([(3 * m + 1) % 16 for m in range(16)], list(range(16)), [(m * m + 5) % 16 for m in range(16)])

SHARP_SETS = ((1, CLASSIC), (2, MULTIBIT))
SHARP_COUNT = 64
# (n, grouping): ciphertexts; one ciphertext = every one of the 2048 phase coefficients
MULTI_SETS = {(2, CLASSIC): 64, (3, CLASSIC): 64, (15, CLASSIC): 64, (16, CLASSIC): 64, (4, MULTIBIT): 64,
              (16, MULTIBIT): 64, (255, CLASSIC): 1, (834, CLASSIC): 1, (834, MULTIBIT): 1}

WORD_CLAIM = 1 << 46
# largest |oracle word - exact word| of the committed sharp sets (seed SEEDS[0]; n = 1 classic with its two
# hand-built rows): 2^40.56 and 2^41.74
WORD_MEASURED = {(1, CLASSIC): 1616957669376, (2, MULTIBIT): 3667809009664}
WORD_CAP = {s: 4 * v for s, v in WORD_MEASURED.items()}

# the oracle's R and worst |f64 - exact| / exact sigma under SEEDS[0], [1], [2]
RATIO_MEASURED = {
    (2, CLASSIC): (2.6740, 2.5316, 2.5929), (3, CLASSIC): (2.0822, 2.0847, 2.0066),
    (15, CLASSIC): (1.2536, 1.4460, 1.2545), (16, CLASSIC): (1.2938, 1.0485, 1.0500),
    (4, MULTIBIT): (4.7562, 6.7889, 4.4408), (16, MULTIBIT): (2.3703, 2.4286, 2.2056),
    (255, CLASSIC): (1.2166, 0.8131, 1.0698), (834, CLASSIC): (0.9889, 0.9857, 0.8968),
    (834, MULTIBIT): (1.5236, 1.2549, 1.2226),
}
DIFF_MEASURED = {
    (2, CLASSIC): (7.7570, 6.0172, 7.0234), (3, CLASSIC): (4.9465, 5.8797, 5.6303),
    (15, CLASSIC): (5.2727, 4.2173, 4.0183), (16, CLASSIC): (3.6637, 3.2919, 4.0874),
    (4, MULTIBIT): (12.2136, 17.4861, 10.4741), (16, MULTIBIT): (9.7510, 5.2039, 7.6256),
    (255, CLASSIC): (5.7503, 4.1236, 6.4570), (834, CLASSIC): (4.2641, 4.7546, 3.9281),
    (834, MULTIBIT): (6.4358, 5.7231, 5.4516),
}


def _cap(v):
    """(largest of the three seeds + their spread) x 1.25"""
    return (max(v) + (max(v) - min(v))) * 1.25


RATIO_CAP = {s: _cap(v) for s, v in RATIO_MEASURED.items()}
DIFF_CAP = {s: _cap(v) for s, v in DIFF_MEASURED.items()}


def set_id(s):
    return f"n{s[0]}-{'mb' if s[1] == MULTIBIT else 'cl'}"


def messages(count):
    return [i % 16 for i in range(count)]


def table_of(i):
    return TABLES[i % len(TABLES)]


def rms(err):
    """root mean square of int64 errors, as a float (statistics only: the errors themselves are exact)"""
    e = np.asarray(err, np.int64).astype(np.float64)
    return float(np.sqrt(np.mean(e * e)))


def log2(x):
    return math.log2(x) if x > 0 else float("-inf")


def phase_figures(err_exact, err_f64):
    """(rms exact, rms f64, R, worst |f64 - exact| in exact sigmas) of two int64 error arrays taken
    against the same ideal phases"""
    se, sf = rms(err_exact), rms(err_f64)
    with np.errstate(over="ignore"):
        diff = np.asarray(err_f64, np.int64) - np.asarray(err_exact, np.int64)
    return se, sf, sf / se, float(np.abs(diff).max()) / se
