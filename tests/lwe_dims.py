"""Test-only table of the LWE dimensions the suite pins besides the default 834, and the parameter
structs of the product and of the oracle at each.  The C ABI accepts any lwe_dimension in [1, 2048]
that the grouping divides (Params::from_c), and every kernel takes n at run time; each (n, grouping)
here is a shape at which something true at 834 is not (tests/test_lwe_dims_gpu.py's table says what).
Never used by the product."""
import oracle
from fhe_sign import default_params

CLASSIC, MULTIBIT = 1, 2
# mid-range first, the extremes last: the GPU file runs them in this order
SETS = [(255, CLASSIC), (256, CLASSIC), (256, MULTIBIT), (833, CLASSIC), (15, CLASSIC), (16, CLASSIC),
        (16, MULTIBIT), (2, CLASSIC), (2, MULTIBIT), (1, CLASSIC), (2048, CLASSIC), (2048, MULTIBIT)]


def set_id(s):
    return f"n{s[0]}-{'mb' if s[1] == MULTIBIT else 'cl'}"


def product_params(n, grouping=CLASSIC):
    p = default_params()
    p.lwe_dimension = n
    p.grouping = grouping
    return p


def oracle_params(n, grouping=CLASSIC):
    p = oracle.default_params()
    p.n = n
    p.grouping = grouping
    return p
