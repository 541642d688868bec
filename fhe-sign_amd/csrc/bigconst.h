// bigconst.h -- clear multi-word arithmetic on public constants (host only, a few hundred bits): the division
// magic numbers, the pseudo-Mersenne fold bounds, the random-below widths.  Results are normalized (no leading
// zero words) unless stated.
#pragma once
#include <cstdint>
#include <vector>

namespace fhe {

// Clear operand of any width: little-endian 64-bit words (tfhe's scalar ops take u64/u128/U256
// scalars; the wide forms back 256-bit division by a 128-bit clear divisor, BASELINE config 3).
using BigConst = std::vector<uint64_t>;

BigConst big_norm(BigConst v);
uint32_t big_bitlen(const BigConst& v);
bool big_bit(const BigConst& v, uint32_t i);
int big_cmp(const BigConst& a, const BigConst& b);
BigConst big_pow2(uint32_t e);
BigConst big_add(const BigConst& a, const BigConst& b);
void big_sub_inplace(BigConst& a, const BigConst& b);  // a >= b; a keeps its width
BigConst big_shr1(BigConst v);
BigConst big_shr(const BigConst& v, uint32_t s);
BigConst big_mul(const BigConst& x, const BigConst& y);
BigConst big_div(const BigConst& num, const BigConst& den);  // floor(num / den), binary long division
BigConst big_mod(const BigConst& a, const BigConst& n);
BigConst big_min(const BigConst& a, const BigConst& b);
BigConst big_from_digits(const std::vector<int64_t>& v);  // sum_q v[q] 4^q for nonnegative v

}  // namespace fhe
